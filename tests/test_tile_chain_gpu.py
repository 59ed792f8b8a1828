"""The data-independent links of a tile wavefront's chain (csrc/la_wave_tile_impl.h), bit for bit against the literal oracle.

The packed kernel takes its topic descriptors through scalar loads where the batch is plain and the wavefront full
(fetch_desc_uniform), the round count and the widest consumer list as maxima over ONE lane per group of L lanes
(wave_max_of_groups_i32), and the bit width of the largest lag from the OR of all lags (bits_of_or_u64).  The shapes below are
the smallest at which each of them can go wrong: groups of one wavefront that disagree, lags whose OR and whose maximum have
their top bit for different reasons, partly filled last wavefronts, topic lists.

Which kernel a batch runs (la_wave_tile.hip): L = consumers rounded up to a power of two (at least 8), E = records per lane;
a batch of at most 2 048 wavefronts is widened to a larger L while E >= 2.  So a batch runs its NARROW shape, several groups
per wavefront, when its topics fit one record per lane (P <= L) or when it is large enough (2 052 topics at L = 32, 8 200 at
L = 8); the resident single-launch form is always a small batch.
"""
import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import synth
from oracle import oracle
from gpu_helpers import Guarded, _batch_of, _same3
import packing_cases as PC

pytestmark = pytest.mark.gpu

PACKING = ["u40", "ties", "pareto", "zero", "u20"]                 # lag kinds of gpu_helpers._batch_of that pack (below 2^41)
PACK_BOUNDS = (1 << 41)


def _alternate(main, others, n):
    return [main if i % 2 == 0 else others[(i // 2) % len(others)] for i in range(n)]


def _with_lags(shapes, lags, seed):
    """The batch of `shapes` with the given per-topic lag arrays (precomputed-lag input)."""
    w = _batch_of(shapes, seed, kinds=["zero"])
    lag = np.concatenate([np.asarray(l, np.int64) for l in lags] + [np.empty(0, np.int64)])
    assert lag.size == w.n_partitions
    return synth.Workload("chain", w.n_topics, w.part_off, w.partition_id, np.zeros_like(lag), lag.copy(), np.zeros_like(lag), lag,
                          w.cons_off, w.cons_rank, w.max_partitions, w.max_consumers)


_expect_cache = {}


def _expect(key, w, use_lag=True):
    """oracle.assign_flat of the batch, computed once per case and shared (read-only).  use_lag: the call hands the lags over
    precomputed (`d_lag`), so the reference takes `w.lag` as it is -- a negative lag stays negative; otherwise the lags are
    oracle.compute_lags of the offsets, as the kernel computes them."""
    if key not in _expect_cache:
        lag = w.lag if use_lag else oracle.compute_lags(w.begin, w.end, w.committed, False)
        _expect_cache[key] = oracle.assign_flat(w.part_off, w.partition_id, lag, w.cons_off, w.cons_rank)
    return _expect_cache[key]


def _call(ctx, w, flags=0, bounds=None, wire=False, use_lag=True, hint=None):
    """One device call with guarded outputs.  Returns (pid, rank, totals); wire: the elements decoded by la_unpack_results_on.
    The guard bands around every output are checked whether the call succeeds or raises."""
    import ctypes
    import torch
    dev = torch.device("cuda", 0)
    n, k = w.n_partitions, w.cons_rank.size
    d = {key: torch.from_numpy(np.ascontiguousarray(getattr(w, key))).to(dev) for key in
         ("part_off", "partition_id", "begin", "end", "committed", "lag", "cons_off", "cons_rank")}
    fmt = N.wire_format_for(int(w.partition_id.max(initial=0)), int(w.cons_rank.max(initial=0)) + 1)
    g_pid = Guarded("device", max(n, 1), np.int32, name="out_partition")
    g_rank = Guarded("device", max(n, 1), np.int32, name="out_member_rank")
    g_tot = Guarded("device", max(k, 1), np.int64, name="out_total_lag")
    g_wire = Guarded("device", max(n, 1), np.int16 if fmt.elem_bytes == 2 else np.int32, shift=1, name="out_wire")      # element-aligned only
    b = N.DeviceBatch()
    b.n_topics, b.reset_mode, b.algo, b.flags = w.n_topics, N.LA_RESET_EARLIEST, N.LA_ALGO_AUTO, flags
    b.n_partitions, b.n_consumers = n, k
    b.max_partitions_per_topic, b.max_consumers_per_topic = hint or (w.max_partitions, w.max_consumers)
    b.d_part_off, b.d_partition_id = d["part_off"].data_ptr(), d["partition_id"].data_ptr()
    if use_lag:
        b.d_lag = d["lag"].data_ptr()
    else:
        b.d_begin_off, b.d_end_off, b.d_committed_off = d["begin"].data_ptr(), d["end"].data_ptr(), d["committed"].data_ptr()
    b.d_cons_off, b.d_cons_rank = d["cons_off"].data_ptr(), d["cons_rank"].data_ptr()
    b.d_out_total_lag = g_tot.ptr
    if wire:
        b.flags |= N.LA_FLAG_WIRE_OUT
        b.d_out_partition = b.d_out_member_rank = None
        b.d_out_wire = g_wire.ptr
        b.wire_elem_bytes, b.wire_id_bits = fmt.elem_bytes, fmt.id_bits
    else:
        b.d_out_partition, b.d_out_member_rank = g_pid.ptr, g_rank.ptr
    if bounds is not None:
        b.flags |= N.LA_FLAG_BOUNDS
        b.max_lag_hint, b.max_partition_id_hint = bounds
    po, co = np.ascontiguousarray(w.part_off, np.int64), np.ascontiguousarray(w.cons_off, np.int64)
    b.h_part_off = po.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    b.h_cons_off = co.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    stream = torch.cuda.current_stream().cuda_stream
    try:
        ctx.assign_batch_device(b, stream)
        ctx.sync(stream)
        if wire:
            ctx.unpack_results(n, g_wire.ptr, fmt, g_pid.ptr, g_rank.ptr, stream)
            ctx.sync(stream)
    finally:
        for g in (g_pid, g_rank, g_tot, g_wire):
            g.check_guards("flags %d bounds %s wire %s" % (flags, bounds, wire))
    return g_pid.values()[:n], g_rank.values()[:n], g_tot.values()[:k]


def _all_forms(ctx, key, w, packs, ragged=True):
    """Resident single-launch form where the batch is small (flags 0) and the two-launch form (LA_FLAG_DEFER_WIDE); the same
    topics through a topic list (LA_FLAG_RAGGED with host offsets); where every tile packs also bounded and bounded with wire
    elements out."""
    exp = _expect(key, w)
    for flags in (0, N.LA_FLAG_DEFER_WIDE):
        _same3(_call(ctx, w, flags), exp, "%s flags %d" % (key, flags))
        if ragged:
            _same3(_call(ctx, w, flags | N.LA_FLAG_RAGGED), exp, "%s topic list, flags %d" % (key, flags))
        if packs:
            bounds = (PACK_BOUNDS, int(w.partition_id.max(initial=0)))
            _same3(_call(ctx, w, flags, bounds), exp, "%s bounded, flags %d" % (key, flags))
            if flags:
                assert ctx.last_launches() == 1, key
            _same3(_call(ctx, w, flags, bounds, wire=True), exp, "%s bounded, wire out, flags %d" % (key, flags))


# ---- group-wise maxima ---------------------------------------------------------------------------------------------------
GROUP_CASES = {
    # (shapes, comment)
    "256x32 alternating, narrow": _alternate((256, 32), [(7, 3), (33, 32), (1, 1), (0, 5)], 2053),      # L = 32: 2 groups, last wave half full
    "256x32 alternating, small": _alternate((256, 32), [(7, 3), (33, 32), (1, 1), (0, 5)], 41),         # resident, widened to L = 64
    "64x8 alternating, narrow": _alternate((64, 8), [(64, 1), (9, 8)], 8203),                           # L = 8: 8 groups
    "64x8 alternating, small": _alternate((64, 8), [(64, 1), (9, 8)], 37),
    "1000x64 alternating": _alternate((1000, 64), [(65, 64)], 9),                                       # L = 64: one group
    # the largest C and the largest round count in different groups of one wavefront
    "split maxima, narrow": _alternate((256, 3), [(40, 32)], 2052),                                     # 86 rounds of 3 | 2 rounds of 32
    "split maxima, one record per lane": _alternate((8, 1), [(8, 8), (3, 2), (0, 5)], 27),              # L = 8, resident: 8 rounds of 1 | 1 of 8
}
for _L in (8, 16, 32, 64):
    # 3 * (64 / L) + 1 topics of at most one record per lane: the last wavefront is partly filled, one group has no topic
    GROUP_CASES["partial last wavefront, L=%d" % _L] = _alternate((_L, _L), [(max(_L - 3, 1), max(_L // 2, 1)), (1, 1), (_L, 1)], 3 * (64 // _L) + 1)


@pytest.mark.parametrize("name", list(GROUP_CASES))
def test_groups_of_one_wavefront_disagree_on_consumers_and_rounds(ctx, name):
    shapes = GROUP_CASES[name]
    w = _batch_of(shapes, len(shapes), kinds=PACKING)
    big = len(shapes) > 1000
    _all_forms(ctx, name, w, packs=True, ragged=not big or "256x32" in name)
    # and with lags that do not pack in some wavefronts (63-bit): the deferred / inline wide form beside the packed one
    w2 = _batch_of(shapes, len(shapes) + 1)
    if not big:
        _all_forms(ctx, name + " mixed", w2, packs=False)


# ---- lag widths -----------------------------------------------------------------------------------------------------------
def _width_topics(rng, p):
    zero = np.zeros(p, np.int64)
    carry = rng.integers(0, 1 << 20, p).astype(np.int64)
    carry[int(rng.integers(0, p))] = 1 << 31                        # the only bit at or above 2^20
    high = rng.integers(1 << 32, 1 << 40, p).astype(np.int64)
    low = rng.integers(0, 1 << 20, p).astype(np.int64)
    neg = low.copy()
    neg[int(rng.integers(0, p))] = -5
    return {"zero": zero, "carry": carry, "high": high, "low": low, "neg": neg}


@pytest.mark.parametrize("mix", [("zero", "carry", "high", "neg"), ("zero", "carry", "high", "low"), ("zero", "carry", "zero", "low"),
                                 ("zero", "zero", "zero", "zero"), ("low", "zero", "low", "carry")])
def test_lag_widths_mixed_in_one_wavefront(ctx, mix):
    """Four 16 x 16 topics = ONE wavefront of the L = 16 kernel (one record per lane: never widened); then the same four kinds
    at 256 x 32 in a batch large enough to stay at L = 32, two kinds per wavefront."""
    rng = np.random.default_rng(len("".join(mix)))
    t = _width_topics(rng, 16)
    w = _with_lags([(16, 16)] * 4, [t[k] for k in mix], 5)
    _all_forms(ctx, "widths16 " + "/".join(mix), w, packs="neg" not in mix)
    t = _width_topics(rng, 256)
    n = 2052
    w = _with_lags([(256, 32)] * n, [t[mix[i % 4]] for i in range(n)], 6)
    exp = _expect("widths256 " + "/".join(mix), w)
    _same3(_call(ctx, w, N.LA_FLAG_DEFER_WIDE), exp, "256 x 32 " + "/".join(mix))
    if "neg" not in mix:
        _same3(_call(ctx, w, 0, (PACK_BOUNDS, 255)), exp, "256 x 32 bounded " + "/".join(mix))
        assert ctx.last_launches() == 1
        _same3(_call(ctx, w, 0, (PACK_BOUNDS, 255), wire=True), exp, "256 x 32 bounded, wire " + "/".join(mix))


def test_negative_lag_from_hostile_offsets(ctx):
    """end < committed (tests/offset_cases.py builds such offsets): computePartitionLag clamps at 0, and a wrapping subtract gives
    lags with the top bit set before the clamp -- through the offset inputs, one such topic among tame ones in one wavefront."""
    import offset_cases as OC
    for regime in OC.REGIMES:
        w = OC.make_case(((16, 16),) * 4 + ((7, 3),), regime, "50%")
        exp = _expect("hostile " + regime, w, use_lag=False)
        for flags in (0, N.LA_FLAG_DEFER_WIDE, N.LA_FLAG_RAGGED):
            _same3(_call(ctx, w, flags, use_lag=False), exp, "hostile %s flags %d" % (regime, flags))


@pytest.mark.parametrize("p,c,lim", [(16, 16, 53), (256, 32, 49)])
def test_lag_bits_at_the_packing_limit_and_one_past(ctx, p, c, lim):
    """Packed records need lag bits <= min(63 - sh, 57 - log2(L * E)) (la_wave_tile_impl.h): 16 x 16 with ids below 16 -> 53,
    256 x 32 with ids below 256 -> 49.  Lags from tests/packing_cases.py ("brim": all within 4 096 of 2^bits - 1, "spread",
    "cliff") with exactly `lim` bits (packs) and lim + 1 (the wide form), next to a topic of small lags in the same batch."""
    rb, ib = PC.decision(p, c, PC.block_bins(c))
    for bits in (lim, lim + 1):
        for kind in ("brim", "spread", "cliff"):
            lag = PC.GENERATORS[kind](p, c, PC.block_bins(c), bits + rb + ib, 100 * bits + p)
            assert int(lag.max()) == (1 << bits) - 1 and int(lag.min()) >= 0
            shapes = [(p, c)] * (64 // max(c, 8) + 1)
            small = np.random.default_rng(bits).integers(0, 1000, p)
            w = _with_lags(shapes, [lag if i % 2 == 0 else small for i in range(len(shapes))], bits)
            key = "limit %dx%d %d bits %s" % (p, c, bits, kind)
            exp = _expect(key, w)
            for flags in (0, N.LA_FLAG_DEFER_WIDE):
                _same3(_call(ctx, w, flags), exp, key)
                _same3(_call(ctx, w, flags, ((1 << bits) - 1, p - 1)), exp, key + " bounded")
                if bits == lim:
                    assert ctx.last_launches() == 1, key
                    _same3(_call(ctx, w, flags, ((1 << bits) - 1, p - 1), wire=True), exp, key + " bounded, wire")


# ---- descriptor path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [8, 16, 32, 64])
def test_descriptors_around_one_wavefront_of_topics(ctx, L):
    """n_topics in {1, 64 / L - 1, 64 / L, 64 / L + 1} (and two wavefronts exactly) of one-record-per-lane topics: the full
    wavefronts take the scalar descriptor loads, the partly filled last one and every topic-list launch the indexed ones."""
    g = 64 // L
    for n in sorted({1, max(g - 1, 1), g, g + 1, 2 * g}):
        full = [(L, L)] * n                                             # every tile full: the FULL form, loads up to n_partitions exactly
        ragged = _alternate((L, L), [(max(L - 3, 1), max(L - 1, 1)), (1, 1)], n)
        ragged[-1] = (L, max(L // 2, 1))                                # the last topic ends exactly at n_partitions
        empty_end = ragged[:-1] + [(0, 2)] if n > 1 else ragged           # ... or has no partitions at all
        for tag, shapes in (("full", full), ("ragged", ragged), ("empty last", empty_end)):
            w = _batch_of(shapes, 7 * n + L, kinds=PACKING)
            assert int(w.part_off[-1]) == w.n_partitions
            _all_forms(ctx, "desc L=%d n=%d %s" % (L, n, tag), w, packs=True)


def test_descriptors_of_a_large_plain_batch_and_its_topic_list(ctx):
    """Many full wavefronts and a partly filled last one at L = 32 (two groups) and L = 8 (eight), plain and through a topic list."""
    for shape, n in (((256, 32), 2051), ((64, 8), 8197)):
        w = synth.make_uniform("desc", n, n, shape[0], shape[1], "zipf", offsets=False)
        exp = _expect("desc big %s" % (shape,), w)
        bounds = (int(w.lag.max()), int(w.partition_id.max()))
        _same3(_call(ctx, w, N.LA_FLAG_DEFER_WIDE), exp, "plain")
        _same3(_call(ctx, w, N.LA_FLAG_RAGGED), exp, "topic list")
        _same3(_call(ctx, w, 0, bounds), exp, "bounded")
        assert ctx.last_launches() == 1
        _same3(_call(ctx, w, 0, bounds, wire=True), exp, "bounded, wire out")


# ---- bounded form: bounds that do not hold ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wire", [False, True])
def test_bounds_too_small_for_one_tile_are_einval_and_touch_nothing_outside(ctx, wire):
    """One topic of the batch holds lags far beyond the caller's bound: its tile does not pack after all.  LA_EINVAL as before,
    nothing written outside the outputs (_call checks the guard bands when the call raises too), and the next call is fine."""
    rng = np.random.default_rng(3)
    for shapes, n in (([(16, 16)] * 9, 9), ([(256, 32)] * 2052, 2052)):
        p = shapes[0][0]
        lags = [rng.integers(0, 1000, p) for _ in range(n)]
        lags[n // 2] = rng.integers(1 << 61, 1 << 62, p)
        w = _with_lags(shapes, lags, 11)
        with pytest.raises(N.LagAssignError) as e:
            _call(ctx, w, N.LA_FLAG_DEFER_WIDE, (1000, p - 1), wire=wire)
        assert e.value.code == N.LA_EINVAL and "LA_FLAG_BOUNDS" in str(e.value)
        _same3(_call(ctx, w, N.LA_FLAG_DEFER_WIDE), _expect("bad bounds %d" % n, w), "after the error")
