"""Hostile offsets through every FUSED computePartitionLag (Main.java:376-404): the tile path's two-stage loads, the block path's
restatement, the large path's keys kernel, the sparse begin list of the host pipelines, and la_compute_lag itself.  The inputs
(tests/offset_cases.py) hold what the tame workloads never do: committed > end, begin > end, committed == 0, "none" as any negative
value, wrapping subtracts, and a poisoned `begin` wherever a partition has a committed offset.  Expected results are the literal
oracle on java_lags (plain numpy); every comparison is bit for bit on order, member and totals."""
import ctypes
import os

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding
from oracle import oracle
from gpu_helpers import SENTINEL, _pinned, _same3, _wire_call
import offset_cases as oc

pytestmark = pytest.mark.gpu

MODES = (False, True)                                                  # latest?
_expected = {}


def _expect(w, latest, begin="own"):
    """oracle.assign_flat on java_lags, once per (batch, mode); begin: the batch's own, or an array that replaces it."""
    own = isinstance(begin, str)
    key = (id(w), latest)
    if own and key in _expected:
        return _expected[key]
    lag = oc.java_lags(w.begin if own else begin, w.end, w.committed, latest)
    exp = oracle.assign_flat(w.part_off, w.partition_id, lag, w.cons_off, w.cons_rank)
    if own:
        _expected[key] = exp
    return exp


def _device_call(ctx, w, latest, begin="own", flags=0, algo=N.LA_ALGO_AUTO, bounds=None):
    """la_assign_batch_device, offsets form (no d_lag).  begin: "own", None (NULL; latest only) -> (order, member, totals)."""
    import torch
    dev = torch.device("cuda", 0)
    names = ["part_off", "partition_id", "end", "committed", "cons_off", "cons_rank"] + (["begin"] if begin is not None else [])
    d = {k: torch.from_numpy(np.array(getattr(w, k))).to(dev) for k in names}
    n, k = w.n_partitions, w.cons_rank.size
    out_pid = torch.full((max(n, 1),), SENTINEL, device=dev, dtype=torch.int32)
    out_rank = torch.full((max(n, 1),), SENTINEL, device=dev, dtype=torch.int32)
    out_total = torch.full((max(k, 1),), SENTINEL, device=dev, dtype=torch.int64)
    b = N.DeviceBatch()
    b.n_topics, b.algo, b.flags = w.n_topics, algo, flags
    b.reset_mode = N.LA_RESET_LATEST if latest else N.LA_RESET_EARLIEST
    b.n_partitions, b.n_consumers = n, k
    b.max_partitions_per_topic, b.max_consumers_per_topic = w.max_partitions, w.max_consumers
    b.d_part_off, b.d_partition_id = d["part_off"].data_ptr(), d["partition_id"].data_ptr()
    b.d_begin_off = d["begin"].data_ptr() if begin is not None else None
    b.d_end_off, b.d_committed_off = d["end"].data_ptr(), d["committed"].data_ptr()
    b.d_cons_off, b.d_cons_rank = d["cons_off"].data_ptr(), d["cons_rank"].data_ptr()
    b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = out_pid.data_ptr(), out_rank.data_ptr(), out_total.data_ptr()
    po, co = np.array(w.part_off), np.array(w.cons_off)
    b.h_part_off = po.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    b.h_cons_off = co.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    if bounds is not None:
        b.flags |= N.LA_FLAG_BOUNDS
        b.max_lag_hint, b.max_partition_id_hint = bounds
    stream = torch.cuda.current_stream().cuda_stream
    ctx.assign_batch_device(b, stream)
    ctx.sync(stream)
    return out_pid.cpu().numpy()[:n], out_rank.cpu().numpy()[:n], out_total.cpu().numpy()[:k]


def _sweep(ctx, shapes, regime, patterns, **kw):
    """Every pattern in both modes; in latest mode `begin` is NULL, and once per batch the poisoned array (it must be ignored)."""
    for i, pattern in enumerate(patterns):
        w = oc.make_case(shapes, regime, pattern)
        for latest in MODES:
            what = "(%s, %s, %s, %s)" % (regime, pattern, "latest" if latest else "earliest", kw)
            _same3(_device_call(ctx, w, latest, begin=None if latest else "own", **kw), _expect(w, latest), what)
        if i == 0:
            _same3(_device_call(ctx, w, True, **kw), _expect(w, True), "(%s, %s, latest with a begin array, %s)" % (regime, pattern, kw))


# ---- tile path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", oc.REGIMES)
@pytest.mark.parametrize("full", [True, False], ids=["full", "ragged"])
@pytest.mark.parametrize("p,c", oc.TILE_SHAPES)
def test_tile(ctx, p, c, full, regime):
    """Full tiles run with LA_FLAG_DEFER_WIDE (the packed kernel's FULL form; wide tiles go to the deferred-tile kernel), ragged
    batches -- last element alone in a clamped pair -- through the single-launch form."""
    patterns = oc.NONE_PATTERNS if (p, c) == oc.TILE_SWEEP else oc.REST_PATTERNS
    _sweep(ctx, oc.tile_batch(p, c, full), regime, patterns, flags=N.LA_FLAG_DEFER_WIDE if full else 0)


@pytest.mark.parametrize("regime", oc.REGIMES)
@pytest.mark.parametrize("algo,flags", [(N.LA_ALGO_ROUNDS_WIDE, 0), (N.LA_ALGO_AUTO, N.LA_FLAG_INDEX64), (N.LA_ALGO_AUTO, N.LA_FLAG_DEFER_WIDE),
                                        (N.LA_ALGO_AUTO, N.LA_FLAG_INDEX64 | N.LA_FLAG_DEFER_WIDE)])
def test_tile_algos_and_flags(ctx, algo, flags, regime):
    _sweep(ctx, oc.tile_batch(*oc.TILE_SWEEP, False), regime, oc.NONE_PATTERNS, algo=algo, flags=flags)


@pytest.mark.parametrize("full", [True, False], ids=["full", "ragged"])
def test_tile_bounded_is_one_launch(ctx, full):
    """Tame-range offsets: no lag exceeds the largest end offset, so the marshaller's bounds prove that every tile packs."""
    for pattern in oc.NONE_PATTERNS:
        w = oc.make_case(oc.tile_batch(*oc.TILE_SWEEP, full), "tame-range", pattern)
        bounds = (int(w.end.max()), int(w.partition_id.max()))
        for latest in MODES:
            for flags in (0, N.LA_FLAG_DEFER_WIDE):
                got = _device_call(ctx, w, latest, flags=flags, bounds=bounds)
                assert ctx.last_launches() == 1, (pattern, latest, flags, ctx.last_launches())
                _same3(got, _expect(w, latest), "(bounded, %s, latest %s, flags %d)" % (pattern, latest, flags))


@pytest.mark.parametrize("full", [True, False], ids=["full", "ragged"])
def test_tile_bounded_wire_out(ctx, full):
    for pattern in oc.NONE_PATTERNS:
        w = oc.make_case(oc.tile_batch(*oc.TILE_SWEEP, full), "tame-range", pattern)
        fmt = N.wire_format_for(int(w.partition_id.max()), int(w.cons_rank.max()) + 1)
        for latest in MODES:
            exp = _expect(w, latest)
            wire, totals = _wire_call(ctx, w, fmt, (int(w.end.max()), int(w.partition_id.max())), latest=latest)
            assert ctx.last_launches() == 1, ctx.last_launches()
            np.testing.assert_array_equal(wire, sharding.pack_results_numpy(exp[0], exp[1], fmt.elem_bytes, fmt.id_bits),
                                          err_msg="wire elements (%s, latest %s)" % (pattern, latest))
            np.testing.assert_array_equal(totals, exp[2], err_msg="totals (%s, latest %s)" % (pattern, latest))


# ---- block path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", oc.REGIMES)
@pytest.mark.parametrize("shapes", [(s,) for s in oc.BLOCK_SHAPES] + [oc.BLOCK_SHAPES], ids=lambda s: "x".join("%d_%d" % t for t in s))
def test_block(ctx, shapes, regime):
    """One topic per block class alone (its first word is the batch's: the dummy read of the `need` select) and the five side by
    side (every pattern; the topic patterns hit the middle one)."""
    _sweep(ctx, shapes, regime, oc.NONE_PATTERNS if len(shapes) > 1 else oc.BLOCK_ALONE_PATTERNS)


# ---- large path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", oc.REGIMES)
@pytest.mark.parametrize("shapes", [(s,) for s in oc.LARGE_SHAPES] + [oc.LARGE_MIXED], ids=lambda s: "x".join("%d_%d" % t for t in s))
def test_large(ctx, shapes, regime):
    _sweep(ctx, shapes, regime, oc.NONE_PATTERNS if len(shapes) > 1 else oc.REST_PATTERNS)


# ---- empty topics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", oc.REGIMES)
@pytest.mark.parametrize("path", list(oc.EMPTY_BATCHES))
def test_empty_topics(ctx, path, regime):
    _sweep(ctx, oc.EMPTY_BATCHES[path], regime, oc.REST_PATTERNS)


# ---- host entry points ---------------------------------------------------------------------------------------------------------
def _grouped_lists(w, exp, n_members):
    """What the grouped calls return, from the expected assignment (gpu_helpers._grouped_expect on given results)."""
    e_pid, e_rank, e_tot = exp
    order = np.argsort(e_rank, kind="stable")
    first = np.searchsorted(e_rank[order], np.arange(n_members + 1))
    topic = (np.searchsorted(w.part_off, order, side="right") - 1).astype(np.int32)
    return first.astype(np.int64), topic, e_pid[order], e_tot


KINDS = {"zero_copy": (0, False, N.LA_PIPELINE_ZERO_COPY), "one_copy": (0, False, N.LA_PIPELINE_ONE_COPY),
         "lanes": (N.LA_CREATE_SPLIT_ALWAYS | 3, False, N.LA_PIPELINE_LANES), "streams": (N.LA_CREATE_SPLIT_ALWAYS, True, N.LA_PIPELINE_STREAMS),
         "mapped": (N.LA_CREATE_SPLIT_ALWAYS, True, N.LA_PIPELINE_MAPPED), "shards": (N.LA_CREATE_SPLIT_ALWAYS, False, N.LA_PIPELINE_LANES)}


@pytest.mark.parametrize("regime", oc.REGIMES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_host_entry_points(kind, regime):
    """One mixed batch (tile, block and large topics, empty ones) through la_assign_batch and la_assign_batch_sparse in every host
    pipeline, each against the oracle and so against the other; the grouped forms where the call is staged or laned."""
    flags, pinned, pipeline = KINDS[kind]
    env = {"one_copy": {"LA_ZERO_COPY_BYTES": "0"}, "streams": {"LA_CHUNK_PARTITIONS": "20000", "LA_NO_MAPPED_PIPELINE": "1"}}.get(kind, {})
    os.environ.update(env)                                             # (the first two are read at la_create, the third at each call)
    try:
        with N.Context([0, 0, 0] if kind == "shards" else 0, flags=flags) as c:
            pin = (lambda a: _pinned(c, a)) if pinned else (lambda a: a)

            def outs(w):
                if not pinned:
                    return None
                return (c.host_alloc((w.n_partitions,), np.int32), c.host_alloc((w.n_partitions,), np.int32),
                        c.host_alloc((w.cons_rank.size,), np.int64))

            for pattern in oc.HOST_PATTERNS:
                w = oc.make_case(oc.HOST_BATCH, regime, pattern)
                idx, val = N.sparse_begin(w.begin, w.committed)
                assert idx.size == int((w.committed < 0).sum()) > 1
                lay = [pin(a) for a in (w.part_off, w.partition_id)]
                off = [pin(a) for a in (w.end, w.committed)]
                cons = [pin(a) for a in (w.cons_off, w.cons_rank)]
                n_members = int(w.cons_rank.max()) + 1
                for latest in MODES:
                    mode = N.LA_RESET_LATEST if latest else N.LA_RESET_EARLIEST
                    exp = _expect(w, latest)
                    what = "(%s, %s, %s, latest %s)" % (kind, regime, pattern, latest)
                    # dense; latest: without a begin array, and with the poisoned one
                    for begin in ((None, w.begin) if latest else (w.begin,)):
                        got = c.assign_batch(*lay, None if begin is None else pin(begin), *off, mode, *cons, out=outs(w))
                        assert c.last_pipeline() == pipeline, (what, c.last_pipeline())
                        _same3(got, exp, "dense " + what)
                    # sparse: the exact list
                    got = c.assign_batch_sparse(*lay, *off, mode, pin(idx), pin(val), *cons, out=outs(w))
                    assert c.last_pipeline() == pipeline, (what, c.last_pipeline())
                    _same3(got, exp, "sparse " + what)
                    # ... with an entry for every partition that HAS a committed offset too, carrying the poison
                    every = np.arange(w.n_partitions, dtype=np.int64)
                    _same3(c.assign_batch_sparse(*lay, *off, mode, pin(every), pin(w.begin), *cons, out=outs(w)), exp, "sparse + poison " + what)
                    # ... with half of its entries dropped: those partitions have begin 0
                    keep = np.arange(idx.size) % 2 == 0
                    begin0 = oc.poison(w.n_partitions)
                    begin0[idx] = 0
                    begin0[idx[keep]] = val[keep]
                    _same3(c.assign_batch_sparse(*lay, *off, mode, pin(idx[keep]), pin(val[keep]), *cons, out=outs(w)),
                           _expect(w, latest, begin0), "sparse, half dropped " + what)
                    if pinned:
                        continue
                    lists = _grouped_lists(w, exp, n_members)
                    g = c.assign_batch_grouped(w.part_off, w.partition_id, None if latest else w.begin, w.end, w.committed, mode,
                                               w.cons_off, w.cons_rank, n_members)
                    for x, y, name in zip(g, lists, ("member_off", "grouped_topic", "grouped_partition", "totals")):
                        np.testing.assert_array_equal(x, y, err_msg="grouped %s %s" % (name, what))
                    g = c.assign_batch_grouped_sparse(w.part_off, w.partition_id, w.end, w.committed, mode, idx, val, w.cons_off,
                                                      w.cons_rank, n_members)
                    for x, y, name in zip(g, lists, ("member_off", "grouped_topic", "grouped_partition", "totals")):
                        np.testing.assert_array_equal(x, y, err_msg="grouped sparse %s %s" % (name, what))
    finally:
        for k in env:
            os.environ.pop(k, None)


# ---- la_compute_lag -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("latest", MODES)
def test_compute_lag_on_every_corner_triple(ctx, latest):
    """All 14^3 triples, the grid cut to n - 1 (odd: the scalar kernel takes the last element) and to 1 (the scalar kernel alone);
    fresh arrays, and views one element into a larger buffer (element-aligned only; the call stages them into its own device
    buffers, so what the views add is the check that nothing outside [0, n) of the caller's output is written)."""
    b, e, c = (x.ravel() for x in np.meshgrid(oc.CORNERS, oc.CORNERS, oc.CORNERS, indexing="ij"))
    n = e.size
    assert n == 2744
    mode = N.LA_RESET_LATEST if latest else N.LA_RESET_EARLIEST
    for length in (n, n - 1, 1):
        for first in sorted({0, n - length}):                               # (the cut grids: from the front and from the back)
            s = slice(first, first + length)
            exp = oc.java_lags(b[s], e[s], c[s], latest)
            fresh = [np.array(x[s]) for x in (b, e, c)]
            np.testing.assert_array_equal(ctx.compute_lag(None if latest else fresh[0], fresh[1], fresh[2], mode), exp)
            views, out = [], np.full(length + 3, SENTINEL, np.int64)
            for x in (b, e, c):
                buf = np.full(length + 3, SENTINEL, np.int64)
                buf[1:1 + length] = x[s]
                views.append(buf[1:1 + length])
            assert all(v.ctypes.data % 8 == 0 for v in views)
            got = ctx.compute_lag(views[0], views[1], views[2], mode, out=out[1:1 + length])       # (latest: begin given, ignored)
            np.testing.assert_array_equal(got, exp)
            assert out[0] == SENTINEL and (out[1 + length:] == SENTINEL).all()
