"""Large path (csrc/la_large.hip: device radix sort + one-workgroup greedy rounds; the multi-pass form beyond 8 192 consumers) through the C ABI, bit-exact against the oracle."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding, synth
from oracle import oracle
from oracle.round_form import round_form
from gpu_helpers import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu


def test_large_topics_side_by_side_mixed_batch(ctx):
    """Large topics of every tile class and rounds class, with and without consumers, between tile- and block-sized topics and
    topics without partitions: the shared launches give what the serial form gives, which is what the oracle gives."""
    shapes = [(100, 5), (20000, 50), (0, 3), (70000, 300), (3000, 200), (18000, 3000), (17000, 0), (150000, 8192),
              (40000, 1), (0, 0), (16385, 64), (300000, 700), (20000, 2049), (64, 8), (3300000, 5)]
    w = _batch_of(shapes, 11)
    exp = round_form(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    got = _device_call(ctx, w)
    _same3(got, exp, "side by side")
    serial = _device_call(ctx, w, flags=N.LA_FLAG_SERIAL_LARGE)
    _same3(serial, exp, "serial hook")
    host = ctx.assign_batch_lags(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)       # the host entry, chunks and all
    _same3(host, exp, "host entry")
    # and twice in a row on the same context (the staging slots alternate; scratch is reused)
    _same3(_device_call(ctx, w), exp, "second call")
    # test hooks of the sort / the greedy still apply to every topic of the launch
    for fl in (N.LA_FLAG_NO_SAMPLE_SORT, N.LA_FLAG_SAMPLE_TIGHT, N.LA_FLAG_NO_RUN_MERGE, N.LA_FLAG_SORT_MULTIKERNEL):
        _same3(_device_call(ctx, w, flags=fl), exp, "flag %d" % fl)


def test_many_equal_large_topics_literal_oracle(ctx):
    """24 topics x 20 000 partitions x 2 100 consumers with wide, negative and tied lags, against the LITERAL oracle."""
    w = _batch_of([(20000, 2100)] * 24, 5, kinds=["full", "u40", "ties"], negative=True)
    exp = oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    _same3(_device_call(ctx, w), exp)


@pytest.mark.parametrize("p,c,kind", [
    (200000, 20000, "pareto"), (8193 * 3, 8193, "u40"), (5000, 9000, "u40"), (18000, 9000, "ties"), (30000, 10000, "zero"),
    (27000, 9000, "full"), (100000, 70000, "u20")])
def test_more_consumers_than_one_workgroup_holds(ctx, p, c, kind):
    """> 8 192 consumers: bins in HBM, a device sort per round.  P < C (one partial round), P = k * C exactly,
    ties, zero lags, negative lags with wrapping totals."""
    w = _batch_of([(p, c)], p + c, kinds=[kind], negative=True)
    exp = round_form(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    _same3(_device_call(ctx, w), exp, "%d x %d %s" % (p, c, kind))
    if p * c <= 200_000_000:                                             # the literal per-step min where it is affordable
        _same3(exp, oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank), "round form vs literal")
    got = _device_call(ctx, w, want_totals=False)
    np.testing.assert_array_equal(got[1], exp[1])


def test_huge_consumer_topic_inside_a_batch(ctx):
    w = _batch_of([(256, 32), (30000, 8300), (20000, 100), (0, 9000), (60000, 20000), (5000, 300)], 21)
    exp = round_form(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    _same3(_device_call(ctx, w), exp)
    _same3(ctx.assign_batch_lags(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank), exp, "host entry")


@pytest.mark.parametrize("n,kind,shuffled,dup,expect_first,expect_redo", [
    (70000, "wide", True, False, 1, 0), (200000, "runs", True, False, 1, 0), (150000, "run4096", True, False, 1, 0),
    (150000, "run9000", True, False, 1, 1), (300000, "run20000_top", True, False, 1, 1), (50000, "equal", True, False, 0, 0),
    (90000, "full", True, False, 1, 1), (120000, "runs", True, True, 1, 0), (80000, "runs", False, False, 0, 0),
    (20000, "runs", True, False, 1, 0), (16385, "wide", True, False, 1, 0), (40000, "pairs", True, False, 1, 0)])
def test_keys_first_sort_forced_on_small_topics(n, kind, shuffled, dup, expect_first, expect_redo):
    """LA_SORT_KEYS_FIRST=2 (test hook): every large-path sort with shuffled ids skips its id passes and repairs the runs of
    equal lags afterwards, whatever the sample says.  Same order as the comparator's (lag desc, id asc): no ties, thousands of
    short runs, a run that just fits a workgroup, runs that do not (the redo slots), negative lags, duplicate ids; ids already
    ascending and all-equal lags never go keys first."""
    os.environ["LA_SORT_KEYS_FIRST"] = "2"
    try:
        with N.Context(0) as c:
            w = _sort_topic(n, kind, n + len(kind), shuffled, dup)
            got = _device_call(c, w, flags=N.LA_FLAG_PROFILE)
            t = c.last_phase_times()
            assert (t.keys_first, t.redone) == (expect_first, expect_redo), (t.keys_first, t.redone)
            order = np.lexsort((w.partition_id, ~w.lag))
            np.testing.assert_array_equal(got[0], w.partition_id[order])
            assert (got[1] == -1).all()
            # with consumers: the greedy reads the repaired order
            w2 = _batch_of([(n, 37)], n, kinds=["ties"])
            _same3(_device_call(c, w2), round_form(w2.part_off, w2.partition_id, w2.lag, w2.cons_off, w2.cons_rank), "with consumers")
            # several topics side by side, each with its own decision
            w3 = _batch_of([(30000, 5), (50000, 0), (20000, 100), (65536, 3)], n + 1, kinds=["ties", "u40", "zero", "pareto"])
            _same3(_device_call(c, w3), round_form(w3.part_off, w3.partition_id, w3.lag, w3.cons_off, w3.cons_rank), "side by side")
    finally:
        os.environ.pop("LA_SORT_KEYS_FIRST", None)


@pytest.mark.parametrize("kind,expect_first", [("wide", 1), ("runs", 0), ("run20000_top", 0), ("equal", 0)])
def test_keys_first_sort_by_the_sample_at_five_million(ctx, kind, expect_first):
    """The default rule: from 4 M partitions on, with shuffled ids, keys first unless the sample of the lags shows a frequent one."""
    n = 5_000_000
    w = _sort_topic(n, kind, 77)
    got = _device_call(ctx, w, flags=N.LA_FLAG_PROFILE)
    t = ctx.last_phase_times()
    assert t.keys_first == expect_first and t.redone == 0, (t.keys_first, t.redone, t.id_passes, t.key_passes)
    order = np.lexsort((w.partition_id, ~w.lag))
    np.testing.assert_array_equal(got[0], w.partition_id[order])
    os.environ["LA_SORT_KEYS_FIRST"] = "0"                  # never: the round-3 order of passes, same answer
    try:
        got0 = _device_call(ctx, w, flags=N.LA_FLAG_PROFILE)
        assert ctx.last_phase_times().keys_first == 0
        np.testing.assert_array_equal(got0[0], got[0])
    finally:
        os.environ.pop("LA_SORT_KEYS_FIRST", None)





# ---- round 6: the caller's bounds rule radix passes out before they are launched ---------------------------------------------------
def _bounded_call(ctx, w, max_lag, max_id, flags=0):
    import ctypes
    import torch
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(getattr(w, k))).to(dev) for k in ("part_off", "partition_id", "lag", "cons_off", "cons_rank")}
    out_pid = torch.full((w.n_partitions,), -7, device=dev, dtype=torch.int32)
    out_rank = torch.full((w.n_partitions,), -7, device=dev, dtype=torch.int32)
    out_total = torch.full((max(w.cons_rank.size, 1),), -7, device=dev, dtype=torch.int64)
    b = N.DeviceBatch()
    b.n_topics, b.reset_mode, b.algo, b.flags = w.n_topics, N.LA_RESET_LATEST, N.LA_ALGO_AUTO, flags
    b.n_partitions, b.n_consumers = w.n_partitions, w.cons_rank.size
    b.max_partitions_per_topic, b.max_consumers_per_topic = w.max_partitions, w.max_consumers
    b.d_part_off, b.d_partition_id, b.d_lag = d["part_off"].data_ptr(), d["partition_id"].data_ptr(), d["lag"].data_ptr()
    b.d_cons_off, b.d_cons_rank = d["cons_off"].data_ptr(), d["cons_rank"].data_ptr()
    b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = out_pid.data_ptr(), out_rank.data_ptr(), out_total.data_ptr()
    po, co = np.ascontiguousarray(w.part_off, np.int64), np.ascontiguousarray(w.cons_off, np.int64)
    b.h_part_off = po.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    b.h_cons_off = co.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    if max_lag is not None:
        b.flags |= N.LA_FLAG_BOUNDS
        b.max_lag_hint, b.max_partition_id_hint = int(max_lag), int(max_id)
    stream = torch.cuda.current_stream().cuda_stream
    ctx.assign_batch_device(b, stream)
    ctx.sync(stream)
    return (out_pid.cpu().numpy(), out_rank.cpu().numpy(), out_total.cpu().numpy()[: w.cons_rank.size]), ctx.last_launches()


@pytest.mark.parametrize("p,c,lag_bits,dense", [(300_000, 3000, 24, True), (200_000, 0, 40, True), (150_000, 1500, 17, False),
                                                (5_000_000, 0, 33, True), (120_000, 8192, 8, True)])
def test_bounds_rule_radix_passes_out_and_a_broken_bound_is_an_error(ctx, p, c, lag_bits, dense):
    """LA_FLAG_BOUNDS on the large path (round 6): key digits above the largest lag's bits and id digits above the largest id's
    bits hold one value in every record -- the device-side plan skips such passes anyway, the host now does not even launch
    them (fewer launches, the same result: the oracle's); a partition outside the bounds is LA_EINVAL, never another order."""
    rng = np.random.default_rng(p + lag_bits)
    lag = rng.integers(0, 1 << lag_bits, p).astype(np.int64)
    ids = rng.permutation(p).astype(np.int32) if dense else (rng.permutation(p).astype(np.int64) * 5 + 3).astype(np.int32)
    w = synth.Workload("bounds", 1, np.array([0, p], np.int64), ids, np.zeros(p, np.int64), lag.copy(), np.zeros(p, np.int64), lag,
                       np.array([0, c], np.int64), np.arange(c, dtype=np.int32), p, c)
    exp = round_form(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    plain, n_plain = _bounded_call(ctx, w, None, None)
    _same3(plain, exp, "no bounds")
    tight, n_tight = _bounded_call(ctx, w, int(lag.max()), int(ids.max()))
    _same3(tight, exp, "tight bounds")
    loose, n_loose = _bounded_call(ctx, w, (1 << 62) - 1, (1 << 31) - 1)
    _same3(loose, exp, "bounds that rule nothing out")
    assert n_tight < n_plain and n_loose == n_plain, (n_tight, n_loose, n_plain)
    # a bound the data breaks: the largest lag (or id) minus one
    for ml, mi in ((int(lag.max()) - 1, int(ids.max())), (int(lag.max()), int(ids.max()) - 1)):
        with pytest.raises(N.LagAssignError) as e:
            _bounded_call(ctx, w, ml, mi)
        assert e.value.code == N.LA_EINVAL
    _same3(_bounded_call(ctx, w, int(lag.max()), int(ids.max()))[0], exp, "after the errors")


# ---- the narrow form of what the rounds kernel reads and writes (round 6: rounds_io, la_large.hip) ---------------------------------
# (_topic_with_lags: gpu_helpers.py)
@pytest.mark.parametrize("p,c,top", [
    (8192 * 5, 8192, (1 << 32) - 1),      # consumers fill every slot, full rounds only, the largest lag that still fits 32 bits
    (8192 * 5, 8192, 1 << 32),            # one bit more: the 64-bit form
    (8192 * 5 + 3, 8192, 10**6),          # a last round of three partitions
    (8192 * 5 - 1, 8192, 10**6),          # a last round one partition short
    (30001, 5001, 10**6),                 # an odd number of consumers: every round's stretch starts off a multiple of 8
    (4097 * 3, 4097, 10**6),              # the fewest consumers that take the form; P = 3 C
    (4096 * 6, 4096, 10**6),              # one consumer fewer: four bins per thread, the old form
    (100, 5000, 10**6),                   # one partial round, far fewer partitions than consumers
    (8, 8192, 10**6), (7, 8192, 10**6),   # the smallest topic that takes the form, and one that is too small for it
    (5003, 5000, 0),                      # equal lags: nothing ever moves
    (120000, 8000, 50),                   # heavy ties
])
def test_rounds_kernel_narrow_lags_and_results(ctx, p, c, top):
    """Topics of more than 4 096 consumers whose bins pack and whose lags fit 32 bits run their greedy rounds on 32-bit lags
    (left by emit_ids_kernel, every round's stretch on a multiple of 8 elements) and leave 16-bit consumer indices that
    map_ranks_kernel turns into member ranks; everything else keeps the 64-bit keys and 32-bit indices.  Both forms, their
    borders, partial rounds and consumer counts that are no multiple of anything, against the oracle -- alone and side by side
    with other large topics (the launches over items)."""
    rng = np.random.default_rng(p * 31 + c)
    lag = rng.integers(0, top + 1, p) if top else np.zeros(p, np.int64)
    if top:
        lag[rng.integers(0, p)] = top                                   # the largest lag is really there
    w = _topic_with_lags(lag, c, p + c)
    exp = round_form(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    if p * c <= 300_000_000:
        _same3(exp, oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank), "round form vs literal")
    _same3(_device_call(ctx, w), exp, "alone")
    got = _device_call(ctx, w, want_totals=False)
    np.testing.assert_array_equal(got[1], exp[1], err_msg="without totals")
    for fl in (N.LA_FLAG_NO_MOVED_SORT, N.LA_FLAG_SAMPLE_TIGHT, N.LA_FLAG_NO_SAMPLE_SORT):
        _same3(_device_call(ctx, w, flags=fl), exp, "flag %d" % fl)
    # side by side with topics of other classes: per-item buffers, one launch per kernel over all of them
    other = _batch_of([(20000, 3000), (p, c), (70000, 300), (9000, 8192), (50000, 6000)], p + 7, kinds=["u20", "u20", "u40", "u20", "ties"])
    lag2 = other.lag.copy()
    lag2[other.part_off[1]:other.part_off[2]] = lag
    w2 = synth.Workload("narrow batch", other.n_topics, other.part_off, other.partition_id, other.begin, lag2.copy(), other.committed, lag2,
                        other.cons_off, other.cons_rank, other.max_partitions, other.max_consumers)
    exp2 = round_form(w2.part_off, w2.partition_id, w2.lag, w2.cons_off, w2.cons_rank)
    _same3(_device_call(ctx, w2), exp2, "side by side")
    _same3(ctx.assign_batch_lags(w2.part_off, w2.partition_id, w2.lag, w2.cons_off, w2.cons_rank), exp2, "host entry")


@pytest.mark.parametrize("p,c,nonzero,top", [
    (100_000, 600, 0, 0),                 # every lag zero: the order of round 0 is final
    (100_000, 600, 1, 10**6),             # one partition with a lag
    (100_000, 600, 599, 10**6), (100_000, 600, 600, 10**6), (100_000, 600, 601, 10**6),   # the zeros begin around a round's border
    (100_000, 600, 31_337, 10**6),        # ... in the middle of round 52
    (100_000, 600, 99_999, 10**6),        # only the last partition has none
    (60_000, 3000, 7000, 50),             # four bins per thread, heavy ties before the zeros
    (200_000, 8192, 20_000, 10**6),       # the narrow form (32-bit lags in, 16-bit indices out)
    (200_000, 8192, 20_000, 1 << 40),     # 64-bit keys
    (200_000, 5000, 4999, 10**6),         # consumers that do not fill the slots; zeros from round 1 on
    (9000, 8192, 100, 10**6),             # two rounds, the second partial
])
def test_rounds_behind_the_last_lag_only_write_the_final_order_down(ctx, p, c, nonzero, top):
    """The lags descend: a greedy round whose first lag is zero hands out zeros only, and so does every round behind it -- the order
    the bins stand in is final, and those rounds skip their order check (found once per topic, before the rounds; greedy_rounds_packed).
    A consumer group that has caught up on most of a big topic's partitions.  Against the oracle, alone and inside an item launch."""
    rng = np.random.default_rng(p + 13 * c + nonzero)
    lag = np.zeros(p, np.int64)
    if nonzero:
        lag[:nonzero] = rng.integers(1, top + 1, nonzero)
        lag = rng.permutation(lag)
    w = _topic_with_lags(lag, c, p + c + nonzero)
    exp = round_form(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    if p * c <= 300_000_000:
        _same3(exp, oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank), "round form vs literal")
    _same3(_device_call(ctx, w), exp, "alone")
    for fl in (N.LA_FLAG_NO_MOVED_SORT, N.LA_FLAG_SAMPLE_TIGHT):
        _same3(_device_call(ctx, w, flags=fl), exp, "flag %d" % fl)
    other = _batch_of([(20000, 3000), (p, c), (70000, 300)], p + 7, kinds=["u20", "u20", "zero"])
    lag2 = other.lag.copy()
    lag2[other.part_off[1]:other.part_off[2]] = lag
    w2 = synth.Workload("zero tail batch", other.n_topics, other.part_off, other.partition_id, other.begin, lag2.copy(), other.committed, lag2,
                        other.cons_off, other.cons_rank, other.max_partitions, other.max_consumers)
    exp2 = round_form(w2.part_off, w2.partition_id, w2.lag, w2.cons_off, w2.cons_rank)
    _same3(_device_call(ctx, w2), exp2, "side by side")
