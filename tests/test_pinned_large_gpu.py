"""la_assign_pinned_device with LA_FLAG_PINNED_LARGE on the GPU: topics of more than 4096 partitions through the large form
(csrc/la_pinned_large.hip).  The expectation of every case is the dictionary model of pinned_cases.py with its limit lifted
(tests/test_pinned_large_cpu.py holds sharding.assign_pinned_numpy against it).  Every comparison is bit for bit on all five
outputs; outputs hold SENTINEL before a call, every array sits between guard bands, inputs must come back unchanged."""
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding
from oracle import oracle

import pinned_cases
import pinned_large_cases as PL
from gpu_helpers import SENTINEL, Guarded, _device_call, shifts_for
from pinned_cases import OUTPUTS, drawn

pytestmark = pytest.mark.gpu

INPUTS = ("part_off", "pid", "lag", "cons_off", "cons_rank", "owned_off", "owned_topic", "owned_pid")
OFFSET_INPUTS = ("begin", "end", "committed")
FLAG = N.LA_FLAG_PINNED_LARGE
MAX_LAUNCHES = N.PINNED_MAX_LAUNCHES + N.PINNED_LARGE_LAUNCHES
_i64p = ctypes.POINTER(ctypes.c_int64)


class Run:
    """One call: every array a Guarded device buffer (4 KiB guard bands, element shift per array).  h_po / h_co: the host's
    offsets (default: the case's; False: none); override: device arrays that differ from the case's."""

    def __init__(self, ctx, case, shifts=None, offsets=None, reset_mode=N.LA_RESET_LATEST, flags=FLAG, h_po=None, h_co=None,
                 override=None):
        import torch
        shifts, override = shifts or {}, override or {}
        self.case = case
        self.inputs = INPUTS + (OFFSET_INPUTS if offsets else ())
        self.g = {}
        for k in self.inputs:
            v = override[k] if k in override else offsets[k] if k in OFFSET_INPUTS else getattr(case, k)
            self.g[k] = Guarded("device", v.size, v.dtype, shifts.get(k, 0), v, name=k)
        sz = {"out_partition": case.n, "out_member_rank": case.n, "totals": case.k, "topic_free": case.t, "summary": 4}
        for k in OUTPUTS:
            self.g[k] = Guarded("device", sz[k], np.int32 if k in ("out_partition", "out_member_rank") else np.int64, shifts.get(k, 0), name=k)
        b = N.DeviceBatch()
        b.n_topics, b.reset_mode, b.flags = case.t, reset_mode, flags
        b.n_partitions, b.n_consumers = case.n, case.k
        b.d_part_off, b.d_partition_id = self.g["part_off"].ptr, self.g["pid"].ptr
        if offsets:
            b.d_begin_off, b.d_end_off, b.d_committed_off = self.g["begin"].ptr, self.g["end"].ptr, self.g["committed"].ptr
        else:
            b.d_lag = self.g["lag"].ptr
        b.d_cons_off, b.d_cons_rank = self.g["cons_off"].ptr, self.g["cons_rank"].ptr
        b.d_out_partition, b.d_out_member_rank = self.g["out_partition"].ptr, self.g["out_member_rank"].ptr
        b.d_out_total_lag = self.g["totals"].ptr
        self.h_po = None if h_po is False else np.ascontiguousarray(case.part_off if h_po is None else h_po, np.int64).copy()
        self.h_co = None if h_co is False else np.ascontiguousarray(case.cons_off if h_co is None else h_co, np.int64).copy()
        if self.h_po is not None:
            b.h_part_off = self.h_po.ctypes.data_as(_i64p)
        if self.h_co is not None:
            b.h_cons_off = self.h_co.ctypes.data_as(_i64p)
        a = N.PinnedArgs()
        a.n_members, a.n_owned = case.m, case.n_owned
        a.d_owned_member_off, a.d_owned_topic, a.d_owned_partition = self.g["owned_off"].ptr, self.g["owned_topic"].ptr, self.g["owned_pid"].ptr
        a.d_topic_free, a.d_summary = self.g["topic_free"].ptr, self.g["summary"].ptr
        self.batch, self.args = b, a
        self.stream = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()
        ctx.assign_pinned_device(b, a, self.stream)
        self.launches = ctx.last_launches()

    def outputs(self):
        return [self.g[k].values() for k in OUTPUTS]

    def check_contract(self, what=""):
        for k in self.inputs:
            self.g[k].check_unchanged(what)
        for k in OUTPUTS:
            self.g[k].check_guards(what)

    def check(self, exp, what=""):
        for k, g, e in zip(OUTPUTS, self.outputs(), exp):
            np.testing.assert_array_equal(g, e, err_msg="%s %s" % (k, what))
        self.check_contract(what)


def _expect_sync_error(ctx, stream, code):
    with pytest.raises(N.LagAssignError) as e:
        ctx.sync(stream)
    assert e.value.code == code, e.value
    ctx.sync(stream)                                                 # the status word is clean again


@pytest.mark.parametrize("name", list(PL.CASES))
def test_the_table_against_the_dictionary_model(ctx, name):
    c, exp = PL.case(name)
    pattern = ("aligned", "odd", "three", "mixed")[list(PL.CASES).index(name) % 4]
    r = Run(ctx, c, shifts_for(pattern, INPUTS + OUTPUTS))
    assert N.PINNED_MAX_LAUNCHES < r.launches <= MAX_LAUNCHES
    ctx.sync(r.stream)
    r.check(exp, name)


def test_nothing_owned_is_the_assign_call_on_each_of_its_routes(ctx):
    c, exp = PL.case("nothing owned")
    r = Run(ctx, c)
    ctx.sync(r.stream)
    r.check(exp, "nothing owned")
    got = r.outputs()
    for t in range(c.t):                                             # each topic alone: the block, wide-block and large routes
        p0, p1, c0, c1 = (int(x) for x in (c.part_off[t], c.part_off[t + 1], c.cons_off[t], c.cons_off[t + 1]))
        w = type("W", (), dict(part_off=np.array([0, p1 - p0], np.int64), partition_id=c.pid[p0:p1], lag=c.lag[p0:p1],
                               cons_off=np.array([0, c1 - c0], np.int64), cons_rank=c.cons_rank[c0:c1], n_topics=1,
                               n_partitions=p1 - p0, max_partitions=p1 - p0, max_consumers=c1 - c0))
        pid, rank, total = _device_call(ctx, w)
        np.testing.assert_array_equal(got[0][p0:p1], pid)
        np.testing.assert_array_equal(got[1][p0:p1], rank)
        np.testing.assert_array_equal(got[2][c0:c1], total)


@pytest.mark.parametrize("latest", [False, True])
def test_lags_from_offsets_are_the_assign_calls(ctx, latest):
    c = drawn(74, [(pinned_cases.MAX_P + 1, 3)], 4, owned=0.5, foreign=0.1, n_stale=2)
    rng = np.random.default_rng(74)
    committed = rng.integers(0, 1 << 20, c.n).astype(np.int64)
    committed[rng.random(c.n) < 0.3] = -1
    begin = rng.integers(0, 1 << 19, c.n).astype(np.int64)
    end = np.maximum(committed, begin) + rng.integers(0, 1 << 18, c.n)
    c.lag = oracle.compute_lags(begin, end, committed, latest)
    r = Run(ctx, c, offsets=dict(begin=begin, end=end, committed=committed),
            reset_mode=N.LA_RESET_LATEST if latest else N.LA_RESET_EARLIEST)
    ctx.sync(r.stream)
    r.check(PL.model(c), "latest=%s" % latest)


def test_the_flag_needs_both_host_arrays_and_checks_them(ctx):
    c, _ = PL.case("one past")
    for kw in (dict(h_po=False), dict(h_co=False), dict(h_po=np.array([5, 3], np.int64)), dict(h_po=np.array([0, c.n + 1], np.int64)),
               dict(h_co=np.array([0, c.k + 1], np.int64)), dict(h_co=np.array([-1, c.k], np.int64))):
        with pytest.raises(N.LagAssignError) as e:
            Run(ctx, c, **kw)
        assert e.value.code == N.LA_EINVAL, kw
        assert ctx.last_launches() == 0, kw
    ctx.sync(0)


def test_without_the_flag_the_topic_is_still_eshape(ctx):
    c, _ = PL.case("one past")
    r = Run(ctx, c, flags=0, h_po=False, h_co=False)
    assert r.launches <= N.PINNED_MAX_LAUNCHES
    _expect_sync_error(ctx, r.stream, N.LA_ESHAPE)
    got = r.outputs()
    assert (got[0] == SENTINEL).all() and (got[1] == SENTINEL).all() and (got[2] == SENTINEL).all()
    r.check_contract("unflagged")


def test_one_large_topic_takes_as_many_launches_as_three(ctx):
    runs = {}
    for name in ("one past", "two large", "three large"):
        c, exp = PL.case(name)
        runs[name] = Run(ctx, c)
        ctx.sync(runs[name].stream)
        runs[name].check(exp, name)
    assert runs["one past"].launches == runs["two large"].launches == runs["three large"].launches <= MAX_LAUNCHES


def test_a_flagged_call_without_a_large_topic_is_the_unflagged_call(ctx):
    c = pinned_cases.CASES["1024 and 1025 partitions"]()
    exp = c.expect()
    plain = Run(ctx, c, flags=0, h_po=False, h_co=False)
    ctx.sync(plain.stream)
    flagged = Run(ctx, c)
    ctx.sync(flagged.stream)
    plain.check(exp, "unflagged")
    flagged.check(exp, "flagged")
    assert flagged.launches == plain.launches <= N.PINNED_MAX_LAUNCHES


def test_a_topic_over_the_consumer_limit_is_eshape_and_its_large_neighbour_exact(ctx):
    c = PL.OVER_CONSUMERS()
    r = Run(ctx, c)
    _expect_sync_error(ctx, r.stream, N.LA_ESHAPE)
    exp = sharding.assign_pinned_numpy(*c.args(), strict=False, max_partitions=sharding.PINNED_ANY_SIZE)
    got = r.outputs()
    p1, c1 = int(c.part_off[1]), int(c.cons_off[1])
    for k, cut in (("out_partition", p1), ("out_member_rank", p1), ("totals", c1)):
        g, x = got[OUTPUTS.index(k)], exp[OUTPUTS.index(k)]
        np.testing.assert_array_equal(g[:cut], x[:cut], err_msg=k)
        assert (g[cut:] == SENTINEL).all(), "%s of the topic over the limit was written" % k
    np.testing.assert_array_equal(got[3], exp[3])
    np.testing.assert_array_equal(got[4][:3], exp[4][:3])
    r.check_contract("2049 consumers")


@pytest.mark.parametrize("what", ["boundary later", "boundary earlier", "large on the device only", "consumer boundary"])
def test_device_offsets_that_differ_from_the_hosts_are_a_shape_error(ctx, what):
    c, exp = PL.case("two large")
    po, h_po, co = c.part_off.copy(), c.part_off.copy(), c.cons_off.copy()
    if what == "boundary later":
        po[1] += 5                                                   # the first topic ends, the second starts, later on the device
    elif what == "boundary earlier":
        po[1] -= 3
    elif what == "consumer boundary":
        co[1] += 1
    else:
        h_po[1] = pinned_cases.MAX_P                                 # by the host's offsets topic 0 is within the limit
    r = Run(ctx, c, h_po=h_po, override={"part_off": po, "cons_off": co})
    _expect_sync_error(ctx, r.stream, N.LA_ESHAPE)
    r.check_contract(what)
    ok = Run(ctx, c)                                                 # the next call on the context is an ordinary one
    ctx.sync(ok.stream)
    ok.check(exp, "after the error")


@pytest.mark.parametrize("bad", ["unsorted ranks", "claimed twice"])
def test_errors_keep_their_codes_in_a_large_topic(ctx, bad):
    good, exp = PL.case("two large")
    c = PL.CASES["two large"]()
    if bad == "unsorted ranks":
        c0 = int(c.cons_off[1])
        c.cons_rank[c0 + 2], c.cons_rank[c0 + 3] = c.cons_rank[c0 + 3], c.cons_rank[c0 + 2]
    else:
        lo, hi = int(c.owned_off[0]), int(c.owned_off[-1])
        c.owned_topic[hi - 1], c.owned_pid[hi - 1] = c.owned_topic[lo], c.owned_pid[lo]
    r = Run(ctx, c)
    _expect_sync_error(ctx, r.stream, N.LA_EINVAL)
    r.check_contract(bad)
    if bad == "unsorted ranks":                                      # the other large topic is exact
        p1, c1 = int(c.part_off[1]), int(c.cons_off[1])
        got = r.outputs()
        np.testing.assert_array_equal(got[0][:p1], exp[0][:p1])
        np.testing.assert_array_equal(got[1][:p1], exp[1][:p1])
        np.testing.assert_array_equal(got[2][:c1], exp[2][:c1])
    ok = Run(ctx, good)
    ctx.sync(ok.stream)
    ok.check(exp, "after the error")


def test_the_result_feeds_the_round_and_the_member_loads_without_a_sync(ctx):
    c, exp = PL.case("foreign and stale")
    r = Run(ctx, c)
    outs = {k: Guarded("device", n, dt, name=k) for k, n, dt in (
        ("coop_rank", c.n, np.int32), ("withheld", c.t, np.int64), ("summary", 6, np.int64), ("member_off", c.m + 1, np.int64),
        ("grouped_topic", c.n, np.int32), ("grouped_partition", c.n, np.int32), ("member_partitions", c.m, np.int64),
        ("member_lag", c.m, np.int64), ("unassigned", 1, np.int64))}
    a = N.CoopRoundArgs()
    a.adjust.n_topics, a.adjust.n_partitions, a.adjust.n_members, a.adjust.n_owned = c.t, c.n, c.m, c.n_owned
    a.adjust.d_part_off, a.adjust.d_out_partition, a.adjust.d_out_member_rank = r.g["part_off"].ptr, r.g["out_partition"].ptr, r.g["out_member_rank"].ptr
    a.adjust.d_owned_member_off, a.adjust.d_owned_topic, a.adjust.d_owned_partition = r.g["owned_off"].ptr, r.g["owned_topic"].ptr, r.g["owned_pid"].ptr
    a.adjust.d_coop_member_rank, a.adjust.d_topic_withheld, a.adjust.d_summary = outs["coop_rank"].ptr, outs["withheld"].ptr, outs["summary"].ptr
    a.member_off, a.grouped_topic, a.grouped_partition = outs["member_off"].ptr, outs["grouped_topic"].ptr, outs["grouped_partition"].ptr
    ctx.cooperative_round_device(a, r.stream)
    ctx.member_loads_device(c.n, r.g["out_member_rank"].ptr, c.k, r.g["cons_rank"].ptr, r.g["totals"].ptr, c.m,
                            outs["member_partitions"].ptr, outs["member_lag"].ptr, outs["unassigned"].ptr, r.stream)
    ctx.sync(r.stream)
    r.check(exp, "before the round")
    e = sharding.cooperative_round_numpy(c.part_off, exp[0], exp[1], c.m, c.owned_off, c.owned_topic, c.owned_pid)
    np.testing.assert_array_equal(outs["coop_rank"].values(), e[1])
    np.testing.assert_array_equal(outs["withheld"].values(), e[6])
    np.testing.assert_array_equal(outs["summary"].values(), e[7])
    np.testing.assert_array_equal(outs["member_off"].values(), e[8])
    np.testing.assert_array_equal(outs["grouped_partition"].values(), e[10])
    assert exp[4][2] > 0 and e[7][2] == exp[4][2] and e[6].tolist() == [exp[4][2]]      # withheld: exactly the foreign partitions
    parts, lag, unassigned = sharding.member_loads_numpy(exp[1], c.cons_rank, exp[2], c.m)
    np.testing.assert_array_equal(outs["member_partitions"].values(), parts)
    np.testing.assert_array_equal(outs["member_lag"].values(), lag)
    assert int(outs["unassigned"].values()[0]) == unassigned == 0
    for g in outs.values():
        g.check_guards("chain")
