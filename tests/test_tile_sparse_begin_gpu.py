"""Stage 2 of the tile kernel (csrc/la_wave_tile_impl.h, issue_begin_loads): a wavefront in which only a few elements lack a
committed offset fetches exactly those `begin` words through scalar loads and puts each into its lane (fetch_begin_sparse); one
with none skips the stage; one with more than LA_TILE_BEGIN_SPARSE_MAX (16 in a launch that fills the chip, 0 -- never sparse --
in one of a few wavefronts like these, unless the hook says otherwise) runs the vector form.  The form exists for tiles of 256
partitions and more outside the resident single-launch kernel; every other instantiation runs the vector form whatever the hook.

Every case is bit-exact (order, member, totals) against oracle.compute_lags + oracle.assign_flat, with the hook at 16 (or the
values a case names), without it, and once more with
LA_TILE_BEGIN_SPARSE_MAX=0 (always the vector form), which must give the same arrays.  `begin` is 1000000 + 7 i and the lags
all differ, so a word taken from a wrong index, or put into a wrong lane or register, changes a total.  The missing elements are
placed by (wavefront, lane, pair register, .x / .y) of the NARROW tile shape of each (partitions, consumers): 8 lanes x 1
record, 16 x 4, 32 x 8, 64 x 16.  A process picks that shape for a handful of topics only with LA_NO_TILE_WIDEN=1, which the
library reads once: test_narrow_shapes_in_a_fresh_process runs this file again under it; in this process the same batches run
the widened shapes (64 lanes x 1 / 1 / 4 / 16 records).  Tiles of 16 records per lane keep the vector form at any count."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding, synth
from oracle import oracle
from gpu_helpers import ROOT, SENTINEL, Guarded, _same3
import offset_cases as oc

pytestmark = pytest.mark.gpu

HOOK = "LA_TILE_BEGIN_SPARSE_MAX"
K = 16                                                      # kTileBeginSparseMax (la_kernels.h)
SHAPES = [(8, 1), (16, 4), (32, 8), (64, 16)]               # (L lanes per topic, E records per lane): P = L * E, C = L
SHAPE_IDS = ["8x1", "16x4", "32x8", "64x16"]
I64 = np.iinfo(np.int64)


def _batch(L, E, sizes, seed=0):
    """Topics of `sizes` partitions (at most L * E), L consumers each; every partition has a committed offset."""
    sizes = np.asarray(sizes, np.int64)
    t = sizes.size
    part_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(part_off[-1])
    rng = np.random.default_rng(1000 * L + E + seed)
    pid = np.concatenate([rng.permutation(int(s)) for s in sizes]).astype(np.int32) if n else np.zeros(0, np.int32)
    i = np.arange(n, dtype=np.int64)
    begin = 1000000 + 7 * i
    end = begin + 1 + (i * 2654435761) % 100003             # lag of an element without a committed offset
    committed = end - (3 + (i * 40503) % 99991)             # ... and with one: both vary from element to element
    cons_off = (np.arange(t + 1) * L).astype(np.int64)
    cons_rank = np.concatenate([np.sort(rng.choice(3 * L + 5, L, replace=False)) for _ in range(t)]).astype(np.int32)
    assert (committed >= 0).all() and (begin > 0).all()
    return synth.Workload("sparse begin", t, part_off, pid, begin, end, committed, np.zeros(n, np.int64), cons_off, cons_rank, L * E, L)


def _full(L, E, waves, seed=0):
    return _batch(L, E, [L * E] * (waves * (64 // L)), seed)


def _at(w, L, E, wave, lane, k=0, c=0):
    """Element index held by `lane` of wavefront `wave` in the .x (c = 0) / .y (c = 1) of pair register k (full tiles before it)."""
    topic = wave * (64 // L) + lane // L
    gl = lane % L
    return int(w.part_off[topic]) + ((k * 2 * L + 2 * gl + c) if E >= 2 else gl)


def _slots(L, E):
    """Every (lane, k, c) of a wavefront, in a fixed scattered order."""
    np_, nc = (E + 1) // 2, (2 if E >= 2 else 1)
    order = np.random.default_rng(L * E).permutation(64 * np_ * nc)
    return [(int(s) % 64, (int(s) // 64) % np_, int(s) // (64 * np_)) for s in order]


def _none(w, idx):
    w.committed = w.committed.copy()
    w.committed[np.asarray(idx, np.int64)] = -1
    return w


def _expect(w, latest=False, begin="own"):
    lag = oracle.compute_lags(w.begin if isinstance(begin, str) else begin, w.end, w.committed, latest)
    return oracle.assign_flat(w.part_off, w.partition_id, lag, w.cons_off, w.cons_rank)


def _call(ctx, w, latest=False, begin="own", flags=0, algo=N.LA_ALGO_AUTO, bounds=None, hook=None, begin_shift=1):
    """la_assign_batch_device on guarded device buffers: `begin` is a view that starts `begin_shift` elements into its
    allocation, every input sits between guard bands and must hold the same bytes after the call."""
    import torch
    names = ["part_off", "partition_id", "end", "committed", "cons_off", "cons_rank"] + (["begin"] if begin is not None else [])
    g = {k: Guarded("device", np.asarray(getattr(w, k)).size, np.asarray(getattr(w, k)).dtype, shift=begin_shift if k == "begin" else 0,
                    values=getattr(w, k), name=k) for k in names}
    n, k = w.n_partitions, w.cons_rank.size
    out = {"pid": Guarded("device", max(n, 1), np.int32, name="out_partition"), "rank": Guarded("device", max(n, 1), np.int32, name="out_member_rank"),
           "total": Guarded("device", max(k, 1), np.int64, name="out_total_lag")}
    b = N.DeviceBatch()
    b.n_topics, b.algo, b.flags = w.n_topics, algo, flags
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
    if bounds is not None:
        b.flags |= N.LA_FLAG_BOUNDS
        b.max_lag_hint, b.max_partition_id_hint = bounds
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


def _check(ctx, w, what, hooks=(K,), exp=None, **kw):
    """The sparse form at the given switch values, the library's own choice (no hook: a launch of a few wavefronts keeps the
    vector form, the sparse one is for launches that fill the chip) and the always-vector form (hook 0), against the oracle."""
    exp = _expect(w, kw.get("latest", False)) if exp is None else exp
    for hook in tuple(hooks) + (None, 0):
        _same3(_call(ctx, w, hook=hook, **kw), exp, "%s, %s=%s" % (what, HOOK, hook))


# ---- one element missing in a wavefront -------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("flags", [0, N.LA_FLAG_DEFER_WIDE], ids=["resident", "full-tile form"])
def test_one_missing_element_at_every_corner(ctx, L, E, flags):
    """Lane 0 and lane 63, first and last pair register, .x and .y, the last lane of a group and the first of the next; the
    wavefronts before and after it have none missing (they skip the stage).  LA_FLAG_DEFER_WIDE: the packed kernel's full-tile
    form (without it a batch this small is the resident single-launch form, which runs the general one)."""
    last_k = (E + 1) // 2 - 1
    lanes = sorted({0, 63, L - 1, L % 64, 31, 32})
    for lane in lanes:
        for k in sorted({0, last_k}):
            for c in ((0, 1) if E >= 2 else (0,)):
                w = _full(L, E, 3)
                _none(w, [_at(w, L, E, 1, lane, k, c)])
                _check(ctx, w, "lane %d register %d.%s" % (lane, k, "xy"[c]), flags=flags)


@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
def test_last_element_of_the_batch(ctx, L, E):
    """The very last element missing: in a ragged last topic of odd size its pair is the one shifted back by one (its lane holds
    it in .y); in a full-tile batch it is lane 63's last .y.  Both also with the element before it missing."""
    for sizes in ([L * E] * (64 // L) + [L * E - 1], [L * E] * (64 // L) + [max(L * E - 3, 1)], [L * E] * (2 * (64 // L)), [1], [3]):
        for extra in ((), (2,)):
            w = _batch(L, E, sizes)
            n = w.n_partitions
            _none(w, [n - 1] + [n - e for e in extra if n >= e])
            for flags in (0, N.LA_FLAG_DEFER_WIDE):
                _check(ctx, w, "sizes %s, missing from the end %s, flags %d" % (sizes[-2:], (1,) + extra, flags), flags=flags)


# ---- both sides of the switch between the sparse and the vector form --------------------------------------------------------------
@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
def test_exactly_k_and_k_plus_one(ctx, L, E):
    """K and K + 1 missing in the middle wavefront of three, scattered over lanes and registers; with the hook at 1 and 2 the
    boundary is crossed with 1, 2 and 3 missing."""
    slots = _slots(L, E)
    for count, hooks in ((K - 1, (K,)), (K, (K,)), (K + 1, (K,)), (1, (1, 2)), (2, (1, 2)), (3, (1, 2))):
        w = _full(L, E, 3, seed=count)
        _none(w, [_at(w, L, E, 1, lane, k, c) for lane, k, c in slots[:count]])
        for flags in (0, N.LA_FLAG_DEFER_WIDE):
            _check(ctx, w, "%d missing, flags %d" % (count, flags), hooks=hooks, flags=flags)


@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
def test_several_in_one_register_and_one_lane(ctx, L, E):
    """Many lanes missing the SAME register half (one ballot with many bits: as many passes), and one lane missing all of its
    elements (every ballot with the same bit)."""
    np_ = (E + 1) // 2
    w = _full(L, E, 3)
    _none(w, [_at(w, L, E, 1, lane, np_ - 1, E >= 2) for lane in (0, 1, 7, 8, 31, 32, 62, 63)])
    _check(ctx, w, "eight lanes, one register half", flags=N.LA_FLAG_DEFER_WIDE)
    w = _full(L, E, 3)
    _none(w, [_at(w, L, E, 1, 37, k, c) for k in range(min(np_, 4)) for c in range(2 if E >= 2 else 1)])
    _check(ctx, w, "one lane, every register", flags=N.LA_FLAG_DEFER_WIDE)
    _check(ctx, w, "one lane, every register, resident form")


@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
def test_one_workgroup_with_none_sparse_and_dense_wavefronts(ctx, L, E):
    """Four wavefronts of one workgroup: none missing, three missing, every element missing, one missing."""
    slots = _slots(L, E)
    for flags in (0, N.LA_FLAG_DEFER_WIDE):
        w = _full(L, E, 4)
        idx = [_at(w, L, E, 1, lane, k, c) for lane, k, c in slots[:3]] + [_at(w, L, E, 3, *slots[5])]
        idx += list(range(_at(w, L, E, 2, 0), _at(w, L, E, 3, 0)))
        _none(w, idx)
        _check(ctx, w, "mixed workgroup, flags %d" % flags, flags=flags)


# ---- the other forms of the kernel ------------------------------------------------------------------------------------------------
def _ragged_sizes(L, E, topics=9):
    cap = L * E
    return [max(1, (cap * (3 + 5 * t) // 11) % (cap + 1)) if t % 3 else cap for t in range(topics)]


@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
def test_ragged_topics_topic_list_wide_and_index64(ctx, L, E):
    """Ragged topics (general form, clamped indices), LA_FLAG_RAGGED (a topic list per shape class), LA_ALGO_ROUNDS_WIDE (the
    wide-record kernel: vector form only), 64-bit indexing."""
    w = _batch(L, E, _ragged_sizes(L, E))
    n = w.n_partitions
    pick = np.unique((np.arange(1, 8) * 2654435761 % n).astype(np.int64))
    _none(w, np.concatenate([pick, [0, n - 1]]))
    exp = _expect(w)
    for flags, algo in ((0, N.LA_ALGO_AUTO), (N.LA_FLAG_DEFER_WIDE, N.LA_ALGO_AUTO), (N.LA_FLAG_RAGGED, N.LA_ALGO_AUTO),
                        (N.LA_FLAG_INDEX64 | N.LA_FLAG_DEFER_WIDE, N.LA_ALGO_AUTO), (0, N.LA_ALGO_ROUNDS_WIDE)):
        _check(ctx, w, "ragged, flags %d algo %d" % (flags, algo), hooks=(K, 2), exp=exp, flags=flags, algo=algo)


@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
def test_wire_out_form(ctx, L, E):
    from gpu_helpers import _wire_call
    slots = _slots(L, E)
    w = _full(L, E, 3)
    _none(w, [_at(w, L, E, 1, lane, k, c) for lane, k, c in slots[:4]] + [w.n_partitions - 1])
    exp = _expect(w)
    fmt = N.wire_format_for(int(w.partition_id.max()), int(w.cons_rank.max()) + 1)
    bounds = (int(w.end.max()), int(w.partition_id.max()))
    for hook in (K, None, 0):
        if hook is not None:
            os.environ[HOOK] = str(hook)
        try:
            wire, totals = _wire_call(ctx, w, fmt, bounds)
        finally:
            os.environ.pop(HOOK, None)
        np.testing.assert_array_equal(wire, sharding.pack_results_numpy(exp[0], exp[1], fmt.elem_bytes, fmt.id_bits), err_msg="hook %s" % hook)
        np.testing.assert_array_equal(totals, exp[2], err_msg="hook %s" % hook)


@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
def test_hostile_begin_at_a_missing_element(ctx, L, E):
    """begin > end (the lag clamps to 0), begin at INT64 min / max (the subtract wraps), begin negative: the word is used as it is."""
    slots = _slots(L, E)
    w = _full(L, E, 3)
    idx = [_at(w, L, E, 1, lane, k, c) for lane, k, c in slots[:5]]
    _none(w, idx)
    w.begin = w.begin.copy()
    w.begin[idx[:4]] = [w.end[idx[0]] + 5, I64.min, I64.max, -3]
    lag = oracle.compute_lags(w.begin, w.end, w.committed, False)
    np.testing.assert_array_equal(lag, oc.java_lags(w.begin, w.end, w.committed, False))
    assert lag[idx[0]] == 0
    for flags in (0, N.LA_FLAG_DEFER_WIDE):
        _check(ctx, w, "hostile begin, flags %d" % flags, flags=flags)


@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
def test_latest_mode_and_no_begin_array_never_read_begin(ctx, L, E):
    slots = _slots(L, E)
    w = _full(L, E, 3)
    _none(w, [_at(w, L, E, 1, lane, k, c) for lane, k, c in slots[:5]])
    exp = _expect(w, latest=True)
    _check(ctx, w, "latest", exp=exp, latest=True)
    _check(ctx, w, "latest, no begin array", exp=exp, latest=True, begin=None)
    _same3(exp, _expect(w, latest=True, begin=None), "the oracle without a begin array")


@pytest.mark.parametrize("L,E", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("shift", [0, 1, 3])
def test_begin_is_a_view_between_guard_bands(ctx, L, E, shift):
    """`begin` starts `shift` elements into a larger buffer whose guard bands would change any result (every _call checks that
    all inputs hold the same bytes afterwards); first and last element of the batch missing, so the words next to both bands are read."""
    w = _batch(L, E, _ragged_sizes(L, E, 5))
    _none(w, [0, 1, w.n_partitions - 1])
    _check(ctx, w, "shift %d" % shift, begin_shift=shift)
    _check(ctx, w, "shift %d, full-tile launch" % shift, begin_shift=shift, flags=N.LA_FLAG_DEFER_WIDE)


# ---- the narrow shapes ------------------------------------------------------------------------------------------------------------
def test_narrow_shapes_in_a_fresh_process():
    """LA_NO_TILE_WIDEN=1 (read once per process) keeps the narrowest tile shape for a handful of topics, so that the positions
    above are the lanes and registers they name: every other test of this file once more under it."""
    if os.environ.get("LA_NO_TILE_WIDEN"):
        return                                              # (this IS that process)
    env = dict(os.environ, LA_NO_TILE_WIDEN="1")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-1000:])
