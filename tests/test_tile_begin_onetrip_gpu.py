"""Stage 2 of the tile kernel, sparse form (csrc/la_wave_tile_impl.h, fetch_begin_sparse): a wavefront in which at most
LA_TILE_BEGIN_SPARSE_MAX elements lack a committed offset fetches exactly their `begin` words through scalar loads.  A pass serves
the lowest missing lane of each of the S = 8 register halves of a tile of 8 records per lane, all its loads back to back and one
wait, and puts each word into its lane; register halves with more than one missing lane take further passes.  "Missing" is
decided once, before the first word arrives: a word from `begin` is used as it is.  The cases here are those that any form which
serves several register halves and several lanes per pass must get right, and which the form of two halves per pass never told
apart: S - 1, S, S + 1, 2 S and 2 S + 1 missing, scattered; all of them in one lane (every register half at once); all of them
in one register half (as many passes); the two groups of one wavefront (each word from its own group's first element); patched
words that look like "missing" again (negative, INT64 min / max) in front of further passes; and the shifted last pair of a
ragged batch next to S others.

Every case is bit-exact (order, member, totals) against oracle.compute_lags + oracle.assign_flat three ways: with the hook at the
built switch K (and at 64), without the hook (the library's choice: a launch of a few wavefronts keeps the vector form) and with
the hook at 0 (always the vector form).  `begin`
is 1000000 + 7 i and all lags differ, so a word from a wrong index, or in a wrong lane or register, changes a total.  Device
buffers sit between guard bands, `begin` is a view that starts one element into its allocation, and every input must hold the
same bytes after the call.  LA_FLAG_DEFER_WIDE reaches the non-resident kernel, the only one the form is compiled in (tiles of
256 partitions and more, at most 8 records per lane: 32 x 8, 64 x 4, 64 x 8).  Positions are (wavefront, lane, pair register,
.x / .y) of the NARROW shape of each (partitions, consumers), which a handful of topics gets only under LA_NO_TILE_WIDEN=1 (read
once per process): test_narrow_shapes_in_a_fresh_process runs this file again under it, so that <32, 8> is the shape that runs."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import synth
from oracle import oracle
from gpu_helpers import ROOT, Guarded, _same3
import offset_cases as oc

pytestmark = pytest.mark.gpu

HOOK = "LA_TILE_BEGIN_SPARSE_MAX"
K = 32                                                      # kTileBeginSparseMax (la_kernels.h)
S = 8                                                       # kBeginSparseChunk (la_wave_tile_impl.h): register halves per pass
SHAPES = [(32, 8), (64, 4), (64, 8)]                        # (L lanes per topic, E records per lane): P = L * E, C = L
SHAPE_IDS = ["32x8", "64x4", "64x8"]
I64 = np.iinfo(np.int64)
DEFER = N.LA_FLAG_DEFER_WIDE


def _batch(L, E, sizes, seed=0):
    """Topics of `sizes` partitions (at most L * E), L consumers each; every partition has a committed offset."""
    sizes = np.asarray(sizes, np.int64)
    t = sizes.size
    part_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(part_off[-1])
    rng = np.random.default_rng(1000 * L + E + seed)
    pid = np.concatenate([rng.permutation(int(s)) for s in sizes]).astype(np.int32)
    i = np.arange(n, dtype=np.int64)
    begin = 1000000 + 7 * i
    end = begin + 1 + (i * 2654435761) % 100003             # lag of an element without a committed offset
    committed = end - (3 + (i * 40503) % 99991)             # ... and with one: both vary from element to element
    cons_off = (np.arange(t + 1) * L).astype(np.int64)
    cons_rank = np.concatenate([np.sort(rng.choice(3 * L + 5, L, replace=False)) for _ in range(t)]).astype(np.int32)
    assert (committed >= 0).all() and (begin > 0).all()
    return synth.Workload("one trip", t, part_off, pid, begin, end, committed, np.zeros(n, np.int64), cons_off, cons_rank, L * E, L)


def _full(L, E, waves, seed=0):
    return _batch(L, E, [L * E] * (waves * (64 // L)), seed)


def _el(w, L, E, topic, gl, k, c):
    """Element held by lane `gl` of `topic`'s group in the .x (c = 0) / .y (c = 1) of pair register k."""
    e = k * 2 * L + 2 * gl + c
    assert e < int(w.part_off[topic + 1] - w.part_off[topic]), (topic, gl, k, c)
    return int(w.part_off[topic]) + e


def _at(w, L, E, wave, lane, k, c):
    return _el(w, L, E, wave * (64 // L) + lane // L, lane % L, k, c)


def _slots(L, E):
    """Every (lane, k, c) of a wavefront, in a fixed scattered order."""
    np_ = E // 2
    order = np.random.default_rng(L * E + 1).permutation(64 * np_ * 2)
    return [(int(s) % 64, (int(s) // 64) % np_, int(s) // (64 * np_)) for s in order]


def _walk_order(slots):
    """Register half by register half, lowest lane first."""
    return sorted(slots, key=lambda s: (2 * s[1] + s[2], s[0]))


def _none(w, idx):
    idx = np.asarray(idx, np.int64)
    assert np.unique(idx).size == idx.size
    w.committed = w.committed.copy()
    w.committed[idx] = -1
    return w


def _expect(w, latest=False, begin="own"):
    lag = oracle.compute_lags(w.begin if isinstance(begin, str) else begin, w.end, w.committed, latest)
    return oracle.assign_flat(w.part_off, w.partition_id, lag, w.cons_off, w.cons_rank)


def _call(ctx, w, latest=False, begin="own", flags=0, hook=None):
    """la_assign_batch_device on guarded device buffers: `begin` is a view that starts one element into its allocation, every
    input sits between guard bands and must hold the same bytes after the call."""
    import torch
    names = ["part_off", "partition_id", "end", "committed", "cons_off", "cons_rank"] + (["begin"] if begin is not None else [])
    g = {k: Guarded("device", np.asarray(getattr(w, k)).size, np.asarray(getattr(w, k)).dtype, shift=1 if k == "begin" else 0,
                    values=getattr(w, k), name=k) for k in names}
    n, k = w.n_partitions, w.cons_rank.size
    out = {"pid": Guarded("device", n, np.int32, name="out_partition"), "rank": Guarded("device", n, np.int32, name="out_member_rank"),
           "total": Guarded("device", k, np.int64, name="out_total_lag")}
    b = N.DeviceBatch()
    b.n_topics, b.algo, b.flags = w.n_topics, N.LA_ALGO_AUTO, flags
    b.reset_mode = N.LA_RESET_LATEST if latest else N.LA_RESET_EARLIEST
    b.n_partitions, b.n_consumers = n, k
    b.max_partitions_per_topic, b.max_consumers_per_topic = w.max_partitions, w.max_consumers
    b.d_part_off, b.d_partition_id = g["part_off"].ptr, g["partition_id"].ptr
    b.d_begin_off = g["begin"].ptr if begin is not None else None
    b.d_end_off, b.d_committed_off = g["end"].ptr, g["committed"].ptr
    b.d_cons_off, b.d_cons_rank = g["cons_off"].ptr, g["cons_rank"].ptr
    b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = out["pid"].ptr, out["rank"].ptr, out["total"].ptr
    po, co = np.array(w.part_off), np.array(w.cons_off)
    b.h_part_off = po.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    b.h_cons_off = co.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    stream = torch.cuda.current_stream().cuda_stream
    old = os.environ.pop(HOOK, None)
    if hook is not None:
        os.environ[HOOK] = str(hook)                        # (read by the library at every call)
    try:
        ctx.assign_batch_device(b, stream)
        ctx.sync(stream)
    finally:
        os.environ.pop(HOOK, None)
        if old is not None:
            os.environ[HOOK] = old
    for x in g.values():
        x.check_unchanged("(hook %s)" % hook)
    for x in out.values():
        x.check_guards("(hook %s)" % hook)
    return out["pid"].values()[:n], out["rank"].values()[:n], out["total"].values()[:k]


def _check(ctx, w, what, hooks=(K,), exp=None, flagses=(DEFER,), **kw):
    """The sparse form at the given switch values, the library's own choice (no hook) and the always-vector form (hook 0):
    each against the oracle, hence all equal."""
    exp = _expect(w, kw.get("latest", False)) if exp is None else exp
    for flags in flagses:
        for hook in tuple(hooks) + (None, 0):
            _same3(_call(ctx, w, hook=hook, flags=flags, **kw), exp, "%s, flags %d, %s=%s" % (what, flags, HOOK, hook))


# ---- both sides of the pass boundary ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("count", [S - 1, S, S + 1, 2 * S, 2 * S + 1], ids=["S-1", "S", "S+1", "2S", "2S+1"])
def test_slot_counts(ctx, L, E, count):
    """`count` missing in the middle wavefront of three, scattered over lanes and registers: fewer than, as many as and more than
    a pass has loads, up to twice as many and one more."""
    w = _full(L, E, 3, seed=count)
    _none(w, [_at(w, L, E, 1, lane, k, c) for lane, k, c in _slots(L, E)[:count]])
    _check(ctx, w, "%d missing" % count, hooks=(K, 64), flagses=(DEFER, 0))


@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
def test_one_lane_many_registers(ctx, L, E):
    """S + 1 missing, every register half of whole lanes (as many as it takes to reach S) plus one element of another lane:
    every register's ballot has the same bits, and every load of a pass belongs to the same lane."""
    w = _full(L, E, 3)
    lanes = (37, 38, 36)[:-(-S // E)]
    idx = [_at(w, L, E, 1, lane, k, c) for lane in lanes for k in range(E // 2) for c in (0, 1)][:S]
    idx.append(_at(w, L, E, 1, 5, E // 2 - 1, 1))
    assert len(idx) == S + 1
    _none(w, idx)
    _check(ctx, w, "whole lanes %s and one more" % (lanes,))


@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("k_of,c", [("first", 0), ("last", 1)])
def test_one_register_half_many_lanes(ctx, L, E, k_of, c):
    """S + 1 missing in the same register half of different lanes: one ballot with S + 1 bits, served lowest lane first, each
    lane exactly once."""
    k = 0 if k_of == "first" else E // 2 - 1
    w = _full(L, E, 3)
    _none(w, [_at(w, L, E, 1, lane, k, c) for lane in (0, 1, 7, 8, 31, 32, 40, 62, 63)])
    _check(ctx, w, "nine lanes, register %d.%s" % (k, "xy"[c]))
    w = _full(L, E, 3)                                      # ... and 2 S + 1 of them
    _none(w, [_at(w, L, E, 1, lane, k, c) for lane in range(3, 3 + 3 * (2 * S + 1), 3)])
    _check(ctx, w, "seventeen lanes, register %d.%s" % (k, "xy"[c]), hooks=(K, 64))


@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
def test_group_boundaries(ctx, L, E, ragged):
    """Missing elements at the last lane of one topic's group and the first lane of the next (for 32 lanes per topic both in one
    wavefront), in several registers: each word must come from its own group's first element.  Ragged: the first of the two
    topics is five partitions short, so the second starts off every tile boundary (the general form, clamped indices)."""
    g = 64 // L
    cap = L * E
    sizes = [cap] * g + ([cap - 5] + [cap] * (2 * g - 1) if ragged else [cap] * (2 * g))
    w = _batch(L, E, sizes)
    a, b = g, g + 1                                         # two neighbouring topics: one wavefront when g == 2
    idx = [_el(w, L, E, a, L - 1, 0, 0), _el(w, L, E, a, L - 1, 0, 1), _el(w, L, E, a, L - (4 if ragged else 2), E // 2 - 1, 0),
           _el(w, L, E, b, 0, 0, 0), _el(w, L, E, b, 0, E // 2 - 1, 1), _el(w, L, E, b, 1, 0, 1)]
    if not ragged:
        idx.append(_el(w, L, E, a, L - 1, E // 2 - 1, 1))   # the topic's very last partition
    _none(w, idx)
    _check(ctx, w, "group boundary, %s" % ("ragged" if ragged else "full"), flagses=(DEFER, 0))
    for extra in range(2, 2 + S):                           # ... and with more than S in the two groups together, several per register half
        idx.append(_el(w, L, E, a if extra % 2 else b, 3 + extra, 0, extra % 2))
    _none(w, idx[-S:])
    _check(ctx, w, "group boundary, %s, more than S" % ("ragged" if ragged else "full"))


# ---- a patched word is never taken as missing again ------------------------------------------------------------------------------
@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("hostile", ["first pass", "all"])
def test_hostile_words_across_passes(ctx, L, E, hostile):
    """S + 4 missing; the words of the first S, register half by register half and lowest lane first (or in a scattered order, or
    of all), are negative, INT64 min or INT64 max.  They are used as they are (begin > end clamps the lag to 0, the subtract
    wraps like Java's), and the later passes must fetch exactly the others: a patched word that is tested for "missing" again
    would be fetched twice or displace another."""
    slots = _slots(L, E)[:S + 4]
    for order in (_walk_order(slots), slots):
        w = _full(L, E, 3)
        idx = [_at(w, L, E, 1, lane, k, c) for lane, k, c in order]
        _none(w, idx)
        w.begin = w.begin.copy()
        bad = idx if hostile == "all" else idx[:S]
        w.begin[bad] = [(-3, I64.min, I64.max, -1, I64.min + 1, I64.max - 1, -(1 << 40))[i % 7] for i in range(len(bad))]
        lag = oracle.compute_lags(w.begin, w.end, w.committed, False)
        np.testing.assert_array_equal(lag, oc.java_lags(w.begin, w.end, w.committed, False))
        _check(ctx, w, "hostile words (%s)" % hostile, flagses=(DEFER, 0))


# ---- the shifted last pair ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("others", [S - 1, S, S + 1])
def test_last_element_of_a_ragged_batch(ctx, L, E, others):
    """The last topic has an odd number of partitions, so the batch's very last element sits in the pair that is shifted back by
    one (its lane holds it in .y); it is missing together with `others` elements of the same wavefront."""
    g = 64 // L
    cap = L * E
    sizes = [cap] * (2 * g) + [cap] * (g - 1) + [cap - 1]
    w = _batch(L, E, sizes)
    n = w.n_partitions
    first = int(w.part_off[2 * g])                          # the last wavefront's first element
    pick = [first + int(x) for x in np.random.default_rng(others).permutation(n - 1 - first)[:others]]
    _none(w, [n - 1] + pick)
    _check(ctx, w, "last element and %d others" % others, flagses=(DEFER, 0))


# ---- the modes that never read `begin` ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
def test_latest_mode_and_no_begin_array_never_read_begin(ctx, L, E):
    """Latest mode with `begin` given (every word of it poison: a word that was read would change a total) and without a `begin`
    array (a null pointer), with S + 1 missing."""
    w = _full(L, E, 3)
    _none(w, [_at(w, L, E, 1, lane, k, c) for lane, k, c in _slots(L, E)[:S + 1]])
    exp = _expect(w, latest=True)
    _same3(exp, _expect(w, latest=True, begin=None), "the oracle without a begin array")
    w.begin = np.full_like(w.begin, I64.min + 12345)
    _same3(exp, _expect(w, latest=True), "the oracle, latest mode, poisoned begin")
    _check(ctx, w, "latest", exp=exp, latest=True)
    _check(ctx, w, "latest, no begin array", exp=exp, latest=True, begin=None)
    # (earliest mode without a `begin` array never reaches a kernel: the call refuses it)
    for hook in (K, None, 0):
        with pytest.raises(N.LagAssignError, match="begin_off is required"):
            _call(ctx, w, latest=False, begin=None, flags=DEFER, hook=hook)


# ---- the narrow shapes ------------------------------------------------------------------------------------------------------------
def test_narrow_shapes_in_a_fresh_process():
    """LA_NO_TILE_WIDEN=1 (read once per process) keeps the narrowest tile shape for a handful of topics, so that the positions
    above are the lanes and registers they name and <32, 8> is a shape that runs: every other test of this file once more."""
    if os.environ.get("LA_NO_TILE_WIDEN"):
        return                                              # (this IS that process)
    env = dict(os.environ, LA_NO_TILE_WIDEN="1")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-1000:])
