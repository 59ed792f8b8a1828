"""la_assign_pinned_device on the GPU: the pinned assignment of a batch against every member's owned list.  The yardstick is
sharding.assign_pinned_numpy (tests/test_pinned_cpu.py holds that restatement against a dictionary model and, with nothing
owned, against the reference oracle).  Every comparison is bit for bit on all five outputs; outputs hold SENTINEL before a call,
every array sits between guard bands, inputs must come back unchanged."""
import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from oracle import oracle

from gpu_helpers import SENTINEL, Guarded, _device_call, shifts_for
from pinned_cases import BROKEN, CASES, OUTPUTS, OVER, broken, drawn, same

pytestmark = pytest.mark.gpu

INPUTS = ("part_off", "pid", "lag", "cons_off", "cons_rank", "owned_off", "owned_topic", "owned_pid")
OFFSET_INPUTS = ("begin", "end", "committed")
CODE = {"LA_EINVAL": N.LA_EINVAL, "LA_ESHAPE": N.LA_ESHAPE}


class Run:
    """One call: every array a Guarded device buffer (4 KiB guard bands, element shift per array)."""

    def __init__(self, ctx, case, shifts=None, want=OUTPUTS, null_owned=False, offsets=None, reset_mode=N.LA_RESET_LATEST, flags=0):
        import torch
        shifts = shifts or {}
        self.case, self.want = case, want
        self.inputs = INPUTS + (OFFSET_INPUTS if offsets else ())
        self.g = {}
        for k in self.inputs:
            v = offsets[k] if k in OFFSET_INPUTS else getattr(case, k)
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
        if "totals" in want:
            b.d_out_total_lag = self.g["totals"].ptr
        a = N.PinnedArgs()
        a.n_members = case.m
        if not null_owned:
            a.n_owned = case.n_owned
            a.d_owned_member_off, a.d_owned_topic, a.d_owned_partition = self.g["owned_off"].ptr, self.g["owned_topic"].ptr, self.g["owned_pid"].ptr
        if "topic_free" in want:
            a.d_topic_free = self.g["topic_free"].ptr
        if "summary" in want:
            a.d_summary = self.g["summary"].ptr
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
            if k in self.want:
                np.testing.assert_array_equal(g, e, err_msg="%s %s" % (k, what))
            else:
                assert (np.asarray(g) == SENTINEL).all(), "%s was not asked for %s" % (k, what)
        self.check_contract(what)


@pytest.mark.parametrize("name", list(CASES))
def test_the_table_against_the_numpy_form(ctx, name):
    c = CASES[name]()
    pattern = ("aligned", "odd", "three", "mixed")[list(CASES).index(name) % 4]
    r = Run(ctx, c, shifts_for(pattern, INPUTS + OUTPUTS))
    assert r.launches <= N.PINNED_MAX_LAUNCHES
    ctx.sync(r.stream)
    r.check(c.expect(), name)


def test_nothing_owned_is_the_assign_call_bit_for_bit(ctx):
    c = drawn(40, [(300, 7), (0, 3), (1025, 65), (64, 64), (17, 0)], 70, lags="ties", owned=0.0)
    r = Run(ctx, c, null_owned=True)
    assert r.launches == 1                                           # no owned entries: no insert launch
    ctx.sync(r.stream)
    exp = c.expect()
    r.check(exp, "null owned lists")
    w = type("W", (), dict(part_off=c.part_off, partition_id=c.pid, lag=c.lag, cons_off=c.cons_off, cons_rank=c.cons_rank,
                           n_topics=c.t, n_partitions=c.n, max_partitions=1025, max_consumers=65))
    pid, rank, total = _device_call(ctx, w)
    np.testing.assert_array_equal(r.outputs()[0], pid)
    np.testing.assert_array_equal(r.outputs()[1], rank)
    np.testing.assert_array_equal(r.outputs()[2], total)


@pytest.mark.parametrize("latest", [False, True])
def test_lags_from_offsets_are_the_assign_calls(ctx, latest):
    c = drawn(41, [(90, 4), (33, 2), (200, 9)], 9, owned=0.6, foreign=0.2, n_stale=2)
    rng = np.random.default_rng(41)
    committed = rng.integers(0, 1 << 20, c.n).astype(np.int64)
    committed[rng.random(c.n) < 0.3] = -1
    begin = rng.integers(0, 1 << 19, c.n).astype(np.int64)
    end = np.maximum(committed, begin) + rng.integers(0, 1 << 18, c.n)
    c.lag = oracle.compute_lags(begin, end, committed, latest)
    r = Run(ctx, c, offsets=dict(begin=begin, end=end, committed=committed),
            reset_mode=N.LA_RESET_LATEST if latest else N.LA_RESET_EARLIEST)
    ctx.sync(r.stream)
    r.check(c.expect(), "latest=%s" % latest)


def test_optional_outputs_may_be_left_out(ctx):
    c = CASES["a foreign claimant"]()
    r = Run(ctx, c, want=("out_partition", "out_member_rank"))
    ctx.sync(r.stream)
    r.check(c.expect(), "results only")


@pytest.mark.parametrize("name", list(OVER))
def test_a_topic_over_a_limit_is_eshape_and_the_others_stay_exact(ctx, name):
    c = OVER[name]()
    r = Run(ctx, c)
    assert r.launches <= N.PINNED_MAX_LAUNCHES
    with pytest.raises(N.LagAssignError) as e:
        ctx.sync(r.stream)
    assert e.value.code == N.LA_ESHAPE
    exp = c.expect(strict=False)
    got = r.outputs()
    over = c.over_limit()
    part_over, cons_over = np.repeat(over, np.diff(c.part_off)), np.repeat(over, np.diff(c.cons_off))
    for k, on in (("out_partition", part_over), ("out_member_rank", part_over), ("totals", cons_over)):
        g, x = got[OUTPUTS.index(k)], exp[OUTPUTS.index(k)]
        np.testing.assert_array_equal(g[~on], x[~on], err_msg=k)
        assert (g[on] == SENTINEL).all(), "%s of the topic over the limit was written" % k
    np.testing.assert_array_equal(got[3], exp[3])
    np.testing.assert_array_equal(got[4][:3], exp[4][:3])
    r.check_contract(name)
    ctx.sync(r.stream)                                               # the status word is clean again


@pytest.mark.parametrize("bad", list(BROKEN))
def test_errors_return_their_codes(ctx, bad):
    c, exact = broken(bad)
    good = drawn(30, [(20, 3), (31, 4), (12, 2)], 6, owned=0.8, foreign=0.2)      # what broken() started from
    r = Run(ctx, c)
    with pytest.raises(N.LagAssignError) as e:
        ctx.sync(r.stream)
    assert e.value.code == CODE[BROKEN[bad]], bad
    r.check_contract(bad)
    exp, got = good.expect(), r.outputs()
    for t in exact:                                                  # the topics the error does not touch
        p0, p1, c0, c1 = (int(x) for x in (c.part_off[t], c.part_off[t + 1], c.cons_off[t], c.cons_off[t + 1]))
        np.testing.assert_array_equal(got[0][p0:p1], exp[0][p0:p1])
        np.testing.assert_array_equal(got[1][p0:p1], exp[1][p0:p1])
        np.testing.assert_array_equal(got[2][c0:c1], exp[2][c0:c1])
        assert got[3][t] == exp[3][t]


def test_offsets_that_leave_the_arrays_are_eshape_and_nothing_is_read_through_them(ctx):
    c = drawn(42, [(20, 3), (31, 4), (12, 2)], 6, owned=0.8)
    good = c.expect()
    c.part_off[2] = c.n + 1000                                       # topic 1 ends, and topic 2 begins, beyond the arrays
    r = Run(ctx, c)
    with pytest.raises(N.LagAssignError) as e:
        ctx.sync(r.stream)
    assert e.value.code == N.LA_ESHAPE
    r.check_contract("part offset beyond N")
    got = r.outputs()
    np.testing.assert_array_equal(got[0][:20], good[0][:20])         # topic 0 is exact, the two others were skipped
    np.testing.assert_array_equal(got[1][:20], good[1][:20])
    assert (got[0][20:] == SENTINEL).all() and (got[1][20:] == SENTINEL).all()
    c = drawn(42, [(20, 3), (31, 4), (12, 2)], 6, owned=0.8)
    c.cons_off[1] = -5
    r = Run(ctx, c)
    with pytest.raises(N.LagAssignError) as e:
        ctx.sync(r.stream)
    assert e.value.code == N.LA_ESHAPE
    r.check_contract("negative consumer offset")


def test_bad_arguments_are_refused_at_the_call(ctx):
    c = CASES["the worked case"]()
    with pytest.raises(N.LagAssignError) as e:
        Run(ctx, c, flags=N.LA_FLAG_WIRE_OUT)
    assert e.value.code == N.LA_EINVAL
    a = N.PinnedArgs()
    a.struct_size = 8
    with pytest.raises(N.LagAssignError) as e:
        ctx.assign_pinned_device(N.DeviceBatch(), a, 0)
    assert e.value.code == N.LA_EINVAL
    a = N.PinnedArgs()
    a.reserved2 = 1
    with pytest.raises(N.LagAssignError) as e:
        ctx.assign_pinned_device(N.DeviceBatch(), a, 0)
    assert e.value.code == N.LA_EINVAL
    ctx.assign_pinned_device(N.DeviceBatch(), N.PinnedArgs(), 0)     # T == 0, N == 0, nothing owned: valid, nothing launched
    assert ctx.last_launches() == 0
    ctx.sync(0)


def test_the_result_feeds_the_cooperative_call_as_it_lies(ctx):
    from kafka_lag_based_assignor_amd import sharding
    c = CASES["64 and 65 consumers"]()
    r = Run(ctx, c)
    ctx.sync(r.stream)
    exp = c.expect()
    r.check(exp, "before the round")
    # the three results as they lie are the target of the cooperative round
    outs = {k: Guarded("device", n, dt, name=k) for k, n, dt in (("coop_rank", c.n, np.int32), ("withheld", c.t, np.int64), ("summary", 6, np.int64))}
    a = N.CoopArgs()
    a.n_topics, a.n_partitions, a.n_members, a.n_owned = c.t, c.n, c.m, c.n_owned
    a.d_part_off, a.d_out_partition, a.d_out_member_rank = r.g["part_off"].ptr, r.g["out_partition"].ptr, r.g["out_member_rank"].ptr
    a.d_owned_member_off, a.d_owned_topic, a.d_owned_partition = r.g["owned_off"].ptr, r.g["owned_topic"].ptr, r.g["owned_pid"].ptr
    a.d_coop_member_rank, a.d_topic_withheld, a.d_summary = outs["coop_rank"].ptr, outs["withheld"].ptr, outs["summary"].ptr
    ctx.cooperative_adjust_device(a, r.stream)
    ctx.sync(r.stream)
    e = sharding.cooperative_adjust_numpy(c.part_off, exp[0], exp[1], c.m, c.owned_off, c.owned_topic, c.owned_pid)
    np.testing.assert_array_equal(outs["coop_rank"].values(), e[1])
    np.testing.assert_array_equal(outs["withheld"].values(), e[6])
    np.testing.assert_array_equal(outs["summary"].values(), e[7])
    assert (np.diff(c.cons_off) > 0).all() and e[7][2] == exp[4][2]      # every topic has consumers: withheld == foreign
