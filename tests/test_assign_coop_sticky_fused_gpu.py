"""la_assign_batch_cooperative_sticky on the GPU: the FUSED zero-copy form (the sticky round's workgroup as the last launch of a
staged call) beside the GENERAL one.  The yardstick is sharding.assign_cooperative_sticky_numpy over the reference oracle's
assign_flat, on all eighteen outputs -- never the library.  Every case runs three times on the same inputs: as it comes (fused
where the call allows it), with LA_NO_FUSED_STICKY=1 in the environment (the general form as it was before there was a fused
one) and with LA_COOP_FORCE_TABLE; all three must equal the yardstick bit for bit.  Cases come from coop_sticky_cases.HostCase
(a group that has caught up: long runs of lag 0) or are built here from explicit arrays."""
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding
from oracle import oracle

import coop_cases as C
import coop_sticky_cases as K
import sticky_cases as S
from gpu_helpers import SENTINEL, Guarded

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
FORMS = ("fused", "general", "forced")
# the eighteen outputs in the order of the yardstick, under the names of the caller's buffers
EXP = ("out_partition", "out_member_rank", "totals", "sticky_partition", "topic_kept", "topic_saved", "sticky_summary", "prev_owner",
       "coop_member_rank", "kept", "fresh", "pending", "release", "topic_withheld", "summary", "member_off", "grouped_topic",
       "grouped_partition")
STICKY = EXP[3:7]
REQUIRED = ("member_off", "grouped_partition")
INPUT_KEYS = ("lag", "begin", "end", "committed", "none_index", "none_begin")


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
class Host(K.HostCase):
    """A HostCase from explicit arrays.  `lag` is what the reference computes in the mode the case is run in; `offsets` =
    (begin, end, committed) for the offset modes; `sparse` = (none_index, none_begin) where the list is not simply every
    partition without a committed offset; owned = (owned_off, owned_topic, owned_partition), default: nobody owns anything."""

    def __init__(self, part_off, pid, lag, cons_off, cons_rank, m, owned=None, offsets=None, sparse=None):
        self.part_off, self.pid = np.ascontiguousarray(part_off, np.int64), np.ascontiguousarray(pid, np.int32)
        self.lag = np.ascontiguousarray(lag, np.int64)
        self.cons_off, self.cons_rank = np.ascontiguousarray(cons_off, np.int64), np.ascontiguousarray(cons_rank, np.int32)
        self.m, self.t, self.n, self.k = int(m), self.part_off.size - 1, int(self.pid.size), int(self.cons_rank.size)
        if owned is None:
            owned = (np.zeros(self.m + 1, np.int64), np.empty(0, np.int32), np.empty(0, np.int32))
        self.owned = (np.ascontiguousarray(owned[0], np.int64), np.ascontiguousarray(owned[1], np.int32), np.ascontiguousarray(owned[2], np.int32))
        if offsets is None:                                         # committed everywhere: end - committed is the lag (where it is >= 0)
            offsets = (np.zeros(self.n, np.int64), self.lag.copy(), np.zeros(self.n, np.int64))
        self.begin, self.end, self.committed = (np.ascontiguousarray(x, np.int64) for x in offsets)
        self.sparse = sparse

    def inputs(self, mode):
        kw = super().inputs(mode)
        if mode == "sparse" and self.sparse is not None:
            kw["none_index"], kw["none_begin"] = (np.ascontiguousarray(x, np.int64) for x in self.sparse)
        return kw

    def with_owned(self, owned, lag=None):
        h = Host(self.part_off, self.pid, self.lag if lag is None else lag, self.cons_off, self.cons_rank, self.m, owned,
                 None if lag is not None else (self.begin, self.end, self.committed), self.sparse)
        return h


def caught_up(seed, sizes, m, rate=0.05):
    """coop_sticky_cases.HostCase with the share of lagging partitions as a parameter: what every member owns is the oracle's
    assignment of the same group one rebalance earlier, when other partitions lagged."""
    rng = np.random.default_rng(seed)
    part_off, pid = C.layout(seed, sizes)
    n = int(pid.size)
    segs = [np.sort(rng.choice(m, int(rng.integers(1, m + 1)), replace=False)) for _ in sizes]
    cons_off = np.concatenate([[0], np.cumsum([x.size for x in segs])]).astype(np.int64)
    cons_rank = np.concatenate(segs + [np.empty(0, np.int64)]).astype(np.int32)
    before, lag = S.caught_up_lags(n, rate, rng), S.caught_up_lags(n, rate, rng)
    was = oracle.assign_flat(part_off, pid, before, cons_off, cons_rank)
    owned = sharding.group_by_member_numpy(part_off, was[0], was[1], m)
    committed = rng.integers(0, 1 << 20, n).astype(np.int64)
    committed[rng.random(n) < 0.3] = -1
    begin = rng.integers(0, 1 << 19, n).astype(np.int64)
    end = np.where(committed >= 0, committed, begin) + lag
    return Host(part_off, pid, lag, cons_off, cons_rank, m, owned, (begin, end, committed))


def small_case():
    """Three topics whose lags and ids pack under the bounds hint: one tile launch."""
    h = K.HostCase(53, [40, 9, 25], 4)
    return Host(h.part_off, h.pid, h.lag % 1000, h.cons_off, h.cons_rank, h.m, h.owned,
                (h.begin, np.where(h.committed >= 0, h.committed, h.begin) + h.lag % 1000, h.committed))


def bounds_of(h):
    """(largest lag, largest id): what holds for the lags of every mode (LATEST only zeroes some)."""
    assert int(h.lag.min()) >= 0 and int(h.pid.min()) >= 0
    return int(h.lag.max()), int(h.pid.max())


LE, LO, LM, LT = K.LE, K.LO, K.LM, K.LT


def limit_case(which, over):
    """Every limit of the one-workgroup form reached at once, `which` one above it when `over`: one partition per topic, the last
    topic holds the surplus (two with N + 1, none with T + 1) and its lags are drawn from {0, 1}; one subscriber per topic."""
    n = LE + (over if which == "N" else 0)
    t = LT + (over if which == "T" else 0)
    m = LM + (over if which == "M" else 0)
    rng = np.random.default_rng(40)
    sizes = np.ones(t, np.int64)
    sizes[-1] += n - t
    part_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pid = rng.integers(-5, 5, n).astype(np.int32)
    pid[-2:] = [7, 8]                                                    # (distinct where a topic has two)
    lag = rng.integers(0, 1 << 30, n)
    a = int(part_off[-2])
    lag[a:] = rng.integers(0, 2, n - a)                                  # (the only topic that can hold a run)
    sub = rng.integers(0, m, t)
    sub[0] = m - 1
    cons_off, cons_rank = np.arange(t + 1, dtype=np.int64), sub.astype(np.int32)
    n_owned = LO + (over if which == "n_owned" else 0)
    owners = np.where(rng.random(n) < 0.7, rng.integers(0, m, n), -1)
    claims = C.claims_from(41, part_off, pid, m, owners=owners)[:n_owned]
    owned = C.owned_arrays(m, claims, 0, n_owned - len(claims), 42)
    assert owned[1].size == n_owned
    return Host(part_off, pid, lag, cons_off, cons_rank, m, owned)


def full_range_lags():
    """Lags over all of int64, negatives included, every extreme twice and side by side with its neighbour."""
    h = caught_up(60, [33, 16, 50], 5)
    rng = np.random.default_rng(61)
    lag = rng.integers(I64.min, I64.max, h.n, endpoint=True)
    vals = [I64.max, I64.max, I64.max - 1, I64.max - 1, 1, 1, 0, 0, -1, -1, -7, -7, I64.min + 1, I64.min + 1, I64.min, I64.min]
    lag[:16], lag[33:49] = vals, vals
    lag[60:90] = rng.integers(-2, 2, 30)
    return h.with_owned(h.owned, lag=lag)


def wrapping_offsets():
    """A dense case whose end - committed and end - begin leave int64: Java's subtraction wraps, then max(., 0)."""
    h = caught_up(62, [40, 7, 30], 4)
    rng = np.random.default_rng(63)
    n = h.n
    pick = lambda: rng.choice(np.array([I64.min, I64.min + 1, -3, 0, 5, I64.max - 1, I64.max], np.int64), n)
    begin, end, committed = pick(), pick(), pick()
    committed[rng.random(n) < 0.4] = -1
    committed[::7] = rng.integers(0, 1 << 20, committed[::7].size)       # some ordinary partitions with ties among them
    end[::7] = committed[::7] + rng.integers(0, 3, committed[::7].size)
    lag = oracle.compute_lags(begin, end, committed, False)
    assert (lag > 0).any() and ((end < 0) & (committed > 0)).any()
    return Host(h.part_off, h.pid, lag, h.cons_off, h.cons_rank, h.m, h.owned, (begin, end, committed))


def sparse_with_unlisted():
    """A sparse case that lists only every other partition without a committed offset: the unlisted ones have begin 0."""
    h = caught_up(64, [50, 21, 30], 4)
    none = np.flatnonzero(h.committed < 0)
    listed = none[::2]
    assert listed.size and listed.size < none.size
    begin = np.zeros(h.n, np.int64)
    begin[listed] = h.begin[listed]
    lag = oracle.compute_lags(begin, h.end, h.committed, False)
    assert not np.array_equal(lag, h.lag)
    return Host(h.part_off, h.pid, lag, h.cons_off, h.cons_rank, h.m, h.owned, (begin, h.end, h.committed), (listed, h.begin[listed]))


def without_consumers():
    """Three topics, the middle one without a subscriber; nearly everything is owned by somebody."""
    part_off, pid = C.layout(65, [20, 15, 30])
    rng = np.random.default_rng(65)
    lag = S.caught_up_lags(65, 0.1, rng)
    claims = C.claims_from(66, part_off, pid, 3, owned_frac=0.9)
    return Host(part_off, pid, lag, [0, 3, 3, 5], [0, 1, 2, 0, 2], 3, C.owned_arrays(3, claims, 1, 1, 67))


# ---- calls --------------------------------------------------------------------------------------------------------------------------------
def host_call(ctx, h, mode, force=False, out=None):
    off, topic, pid = h.owned
    return ctx.assign_batch_cooperative_sticky(h.part_off, h.pid, h.cons_off, h.cons_rank, h.m, off, topic, pid, force_table=force,
                                               out=out, **h.inputs(mode))


def assign_call(ctx, h, mode):
    """The plain assign call on the same inputs: assign_batch_lags / assign_batch / assign_batch_sparse."""
    kw = h.inputs(mode)
    if mode == "lag":
        return ctx.assign_batch_lags(h.part_off, h.pid, kw["lag"], h.cons_off, h.cons_rank)
    if mode == "sparse":
        return ctx.assign_batch_sparse(h.part_off, h.pid, kw["end"], kw["committed"], kw["reset_mode"], kw["none_index"], kw["none_begin"],
                                       h.cons_off, h.cons_rank)
    return ctx.assign_batch(h.part_off, h.pid, kw.get("begin"), kw["end"], kw["committed"], kw["reset_mode"], h.cons_off, h.cons_rank)


def flat(got):
    """An AssignSticky -> its arrays by the names of EXP."""
    d = dict(zip(N.AssignCoop._fields, got.coop))
    d.update(zip(STICKY, got[1:]))
    return d


def same(got, exp, what="", names=EXP):
    for name, e in zip(EXP, exp):
        if name in names:
            np.testing.assert_array_equal(got[name], e, err_msg="%s %s" % (name, what))


def three_ways(ctx, monkeypatch, h, mode, exp=None, what=""):
    """The call as it comes, under LA_NO_FUSED_STICKY and with LA_COOP_FORCE_TABLE, each against the yardstick ->
    {form: (outputs by name, launches, pipeline)}."""
    exp = h.expect(mode) if exp is None else exp
    res = {}
    for form in FORMS:
        with monkeypatch.context() as mp:
            if form == "general":
                mp.setenv("LA_NO_FUSED_STICKY", "1")
            got = flat(host_call(ctx, h, mode, force=form == "forced"))
        res[form] = (got, ctx.last_launches(), ctx.last_pipeline())
        same(got, exp, "%s, %s, %s" % (what, mode, form))
    return res


def buffers(h, null=(), make=None):
    """Caller-owned outputs holding SENTINEL, by name; those in `null` are None ("target": the pair)."""
    make = make or (lambda name, size, dtype: np.full(size, SENTINEL, dtype))
    n, m, t, k = h.n, h.m, h.t, h.k
    sizes = dict(out_partition=n, out_member_rank=n, totals=k, sticky_partition=n, topic_kept=t, topic_saved=t, sticky_summary=4,
                 prev_owner=n, coop_member_rank=n, kept=m, fresh=m, pending=m, release=m, topic_withheld=t, summary=6, member_off=m + 1,
                 grouped_topic=n, grouped_partition=n)
    i32 = ("out_partition", "out_member_rank", "sticky_partition", "prev_owner", "coop_member_rank", "grouped_topic", "grouped_partition")
    gone = set(null) | ({"out_partition", "out_member_rank"} if "target" in null else set())
    return {name: None if name in gone else make(name, sizes[name], np.int32 if name in i32 else np.int64) for name in EXP}


def raw_call(ctx, h, mode, bufs, force=False, inputs=None, owned=None, arrays=None):
    """la_assign_batch_cooperative_sticky through ctypes, so that EVERY output can be NULL -> the return code.  `arrays`: the
    caller's input arrays by name where they are not h's own (guarded views)."""
    a = arrays or {}
    kw = dict(h.inputs(mode) if inputs is None else inputs)
    kw.update({k: a[k] for k in INPUT_KEYS if k in a})
    off, topic, pid = owned if owned is not None else tuple(a.get(k, x) for k, x in zip(("owned_off", "owned_topic", "owned_partition"), h.owned))
    args = N.AssignStickyArgs()
    args.struct_size = ctypes.sizeof(N.AssignStickyArgs)
    coop = N.AssignCoop(**{k: bufs[k] for k in N.AssignCoop._fields})
    ctx._fill_assign_coop(args.coop, a.get("part_off", h.part_off), a.get("pid", h.pid), a.get("cons_off", h.cons_off),
                          a.get("cons_rank", h.cons_rank), h.m, off, topic, pid, kw.get("lag"), kw.get("begin"), kw.get("end"),
                          kw.get("committed"), kw.get("reset_mode", 0), kw.get("none_index"), kw.get("none_begin"), force, coop)
    for name in STICKY:
        setattr(args, name, bufs[name].ctypes.data if bufs[name] is not None and bufs[name].size else None)
    return N.load().la_assign_batch_cooperative_sticky(ctx._h, ctypes.byref(args))


def raw_three_ways(ctx, monkeypatch, h, mode, exp, null=(), what="", **kw):
    """raw_call in the three forms with fresh buffers each time; every buffer that is there must equal the yardstick."""
    for form in FORMS:
        bufs = buffers(h, null)
        with monkeypatch.context() as mp:
            if form == "general":
                mp.setenv("LA_NO_FUSED_STICKY", "1")
            rc = raw_call(ctx, h, mode, bufs, force=form == "forced", **kw)
        assert rc == N.LA_OK, "%s, %s: %d" % (what, form, rc)
        same(bufs, exp, "%s, %s" % (what, form), names=[k for k in EXP if bufs[k] is not None])


# ---- 1: the form is taken ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", K.HOST_MODES)
def test_the_fused_form_is_taken(ctx, torch_dev, monkeypatch, mode):
    h = small_case()
    exp = h.expect(mode)
    res = three_ways(ctx, monkeypatch, h, mode, exp)
    same(flat(host_call(ctx, h, mode)), exp, "unhinted")
    unhinted, pipeline = ctx.last_launches(), ctx.last_pipeline()
    assign_call(ctx, h, mode)
    assert unhinted == ctx.last_launches(), "the sticky round takes the place of the assign call's finishing launch"
    assert pipeline == N.LA_PIPELINE_ZERO_COPY
    assert res["fused"][1] == unhinted
    assert res["general"][1] > unhinted, "LA_NO_FUSED_STICKY: the launches of the assign call and of the round"
    ctx.hint_next_call(bounds_of(h))
    same(flat(host_call(ctx, h, mode)), exp, "hinted")
    assert ctx.last_launches() == 2, "one tile launch, then the sticky round"
    assert ctx.last_pipeline() == N.LA_PIPELINE_ZERO_COPY


# ---- 2: register and LDS edges of the lag delivery ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["lag", "sparse"])
@pytest.mark.parametrize("sizes", [[1], [1023], [1024], [1025], [1024, 1024], [2047, 1]], ids=lambda s: "x".join(map(str, s)))
def test_a_caught_up_group_at_the_edges_of_the_lag_delivery(ctx, torch_dev, monkeypatch, sizes, mode):
    h = caught_up(21, sizes, 1 if sizes == [1] else 8, rate=0.01)
    res = three_ways(ctx, monkeypatch, h, mode, what=str(sizes))
    assert res["fused"][2] == N.LA_PIPELINE_ZERO_COPY and res["fused"][1] < res["general"][1]
    if h.n >= 1023:
        assert res["fused"][0]["sticky_summary"][2] > 0, "some topic's order changed: the runs of lag 0 were re-matched"


# ---- 3: each limit and one above it -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [0, 1], ids=["at the limit", "one above"])
@pytest.mark.parametrize("which", ["N", "n_owned", "M", "T"])
def test_each_limit_and_one_above_it(ctx, torch_dev, monkeypatch, which, over):
    h = limit_case(which, over)
    res = three_ways(ctx, monkeypatch, h, "lag", what="%s + %d" % (which, over))
    same(flat(host_call(ctx, h, "lag")), h.expect("lag"))
    launches, pipeline = ctx.last_launches(), ctx.last_pipeline()
    assign_call(ctx, h, "lag")
    if not over:
        assert launches == ctx.last_launches(), "the round takes the place of the finishing launch"
        assert pipeline == N.LA_PIPELINE_ZERO_COPY
    else:
        assert launches > ctx.last_launches(), "the general form: the launches of both calls"
    assert res["fused"][1] == launches


# ---- 4: lags ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["full int64 range", "wrapping offsets", "sparse with unlisted partitions"])
def test_lags(ctx, torch_dev, monkeypatch, name):
    h, mode = {"full int64 range": (full_range_lags, "lag"), "wrapping offsets": (wrapping_offsets, "dense"),
               "sparse with unlisted partitions": (sparse_with_unlisted, "sparse")}[name]
    h = h()
    res = three_ways(ctx, monkeypatch, h, mode, what=name)
    assert res["fused"][2] == N.LA_PIPELINE_ZERO_COPY and res["fused"][1] < res["general"][1]


# ---- 5: optional outputs ------------------------------------------------------------------------------------------------------------------
def test_every_optional_output_is_null_in_turn_and_all_at_once(ctx, torch_dev, monkeypatch):
    h = caught_up(30, [12, 0, 33, 5], 4)
    exp = h.expect("dense")
    optional = tuple(k for k in EXP if k not in REQUIRED + ("out_partition", "out_member_rank")) + ("target",)
    assert len(optional) == 15
    for drop in optional:
        raw_three_ways(ctx, monkeypatch, h, "dense", exp, null=(drop,), what="without %s" % drop)
    raw_three_ways(ctx, monkeypatch, h, "dense", exp, null=optional, what="only the required outputs")
    raw_three_ways(ctx, monkeypatch, h, "dense", exp, what="every output")


# ---- 6: degenerate shapes -------------------------------------------------------------------------------------------------------------------
def test_nothing_owned_and_a_topic_without_consumers(ctx, torch_dev, monkeypatch):
    c = caught_up(31, [40, 9, 25], 4)
    h = c.with_owned(None)
    res = three_ways(ctx, monkeypatch, h, "sparse", what="n_owned == 0")
    got = res["fused"][0]
    np.testing.assert_array_equal(got["sticky_partition"], got["out_partition"], err_msg="nothing owned: nothing to keep")
    assert res["fused"][2] == N.LA_PIPELINE_ZERO_COPY and res["fused"][1] < res["general"][1]
    h = without_consumers()
    res = three_ways(ctx, monkeypatch, h, "lag", what="a topic without consumers")
    got = res["fused"][0]
    assert (got["out_member_rank"][20:35] == -1).all() and got["summary"][3] > 0       # owned by somebody, assigned to nobody: dropped
    assert got["member_off"][0] >= 15


def test_no_topics_no_entries_no_members(ctx, torch_dev, monkeypatch):
    three_ways(ctx, monkeypatch, Host([0], [], [], [0], [], 3), "lag", what="T == 0")
    three_ways(ctx, monkeypatch, Host([0, 0, 0], [], [], [0, 1, 3], [0, 0, 1], 2, ([0, 1, 2], [0, 1], [5, 6])), "lag", what="N == 0")
    res = three_ways(ctx, monkeypatch, Host([0, 2, 5], [1, 0, 2, 0, 1], [3, 4, 5, 6, 7], [0, 0, 0], [], 0), "lag", what="M == 0")
    assert (res["fused"][0]["out_member_rank"] == -1).all() and res["fused"][0]["member_off"].tolist() == [5]


# ---- 7: errors ------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched_and_nothing_behind(ctx, torch_dev, monkeypatch):
    h = small_case()
    exp = h.expect("lag")
    same(flat(host_call(ctx, h, "lag")), exp, "before the errors")
    unhinted = ctx.last_launches()
    dup = Host(h.part_off, h.pid.copy(), h.lag, h.cons_off, h.cons_rank, h.m, h.owned, (h.begin, h.end, h.committed))
    dup.pid[1] = dup.pid[0]
    none_index, none_begin = N.sparse_begin(h.begin, h.committed)
    assert none_index.size >= 2
    descending = dict(h.inputs("sparse"), none_index=none_index[::-1].copy(), none_begin=none_begin)
    twice = ([0, 1, 2, 2, 2], [0, 0], [h.pid[0], h.pid[0]])
    cases = {"a partition owned twice": (h, "lag", dict(owned=twice)), "a duplicate input id": (dup, "lag", {}),
             "none_index descends": (h, "sparse", dict(inputs=descending))}
    for what, (k, mode, kw) in cases.items():
        for form in FORMS:
            bufs = buffers(k)
            with monkeypatch.context() as mp:
                if form == "general":
                    mp.setenv("LA_NO_FUSED_STICKY", "1")
                rc = raw_call(ctx, k, mode, bufs, force=form == "forced", **kw)
            assert rc == N.LA_EINVAL, "%s, %s: %d" % (what, form, rc)
            for name, b in bufs.items():
                assert (b == SENTINEL).all(), "%s was written by a call that failed (%s, %s)" % (name, what, form)
        # the next fused call on the same context: exact, and nothing of the failed one is left in the status word
        same(flat(host_call(ctx, h, "lag")), exp, "after %s" % what)
        assert ctx.last_launches() == unhinted and ctx.last_pipeline() == N.LA_PIPELINE_ZERO_COPY
    # a hint taken by a failed fused call is gone
    ctx.hint_next_call(bounds_of(h))
    assert raw_call(ctx, h, "lag", buffers(h), owned=twice) == N.LA_EINVAL
    same(flat(host_call(ctx, h, "lag")), exp, "after a failed hinted call")
    assert ctx.last_launches() == unhinted


@pytest.mark.parametrize("form", ["as it comes", "LA_NO_FUSED_STICKY"])
def test_entry_refuses_bad_arguments(ctx, torch_dev, monkeypatch, form):
    """The table of la_assign_batch_cooperative's test of this name (test_assign_coop_gpu.py), on a struct that is valid but for
    the one field: two topics of 5 and 6 partitions, 2 members, lags mode."""
    if form == "LA_NO_FUSED_STICKY":
        monkeypatch.setenv("LA_NO_FUSED_STICKY", "1")
    lib = N.load()
    h = caught_up(38, [5, 6], 2)
    bufs = buffers(h)

    def args():
        a = N.AssignStickyArgs()
        a.struct_size = ctypes.sizeof(N.AssignStickyArgs)
        ctx._fill_assign_coop(a.coop, h.part_off, h.pid, h.cons_off, h.cons_rank, h.m, *h.owned, h.lag, None, None, None, 0, None, None,
                              False, N.AssignCoop(**{k: bufs[k] for k in N.AssignCoop._fields}))
        for name in STICKY:
            setattr(a, name, bufs[name].ctypes.data)
        return a

    def no_owned_arrays(a):
        a.coop.n_owned, a.coop.owned_member_off, a.coop.owned_topic, a.coop.owned_partition = 3, None, None, None

    for name, change in (("struct_size", lambda a: setattr(a, "struct_size", a.struct_size - 8)),
                         ("an unknown flag bit", lambda a: setattr(a.coop, "flags", 4)),
                         ("reserved", lambda a: setattr(a, "reserved", 1)), ("coop.reserved", lambda a: setattr(a.coop, "reserved", 1)),
                         ("n_members", lambda a: setattr(a.coop, "n_members", -1)), ("n_owned without owned arrays", no_owned_arrays),
                         ("member_off", lambda a: setattr(a.coop, "member_off", None)),
                         ("grouped_partition", lambda a: setattr(a.coop, "grouped_partition", None)),
                         ("out_partition without out_member_rank", lambda a: setattr(a.coop, "out_member_rank", None))):
        a = args()
        change(a)
        assert lib.la_assign_batch_cooperative_sticky(ctx._h, ctypes.byref(a)) == N.LA_EINVAL, name
        for out, b in bufs.items():
            assert (b == SENTINEL).all(), "%s was written by a call that was refused (%s)" % (out, name)
    assert lib.la_assign_batch_cooperative_sticky(ctx._h, None) == N.LA_EINVAL
    assert lib.la_assign_batch_cooperative_sticky(None, ctypes.byref(args())) == N.LA_EINVAL
    a = args()
    assert lib.la_assign_batch_cooperative_sticky(ctx._h, ctypes.byref(a)) == N.LA_OK
    same(bufs, h.expect("lag"), form)


# ---- 8: buffer contract ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["lag", "dense", "sparse"])
def test_guarded_views_at_shift_one(ctx, torch_dev, monkeypatch, mode):
    h = caught_up(32, [70, 1, 130, 0, 56], 5)
    exp = h.expect(mode)
    named = dict(part_off=h.part_off, pid=h.pid, cons_off=h.cons_off, cons_rank=h.cons_rank, owned_off=h.owned[0], owned_topic=h.owned[1],
                 owned_partition=h.owned[2])
    named.update({k: v for k, v in h.inputs(mode).items() if k in INPUT_KEYS})
    for form in FORMS:
        ins = {k: Guarded("numpy", v.size, v.dtype, 1, v, name=k) for k, v in named.items()}
        outs = {}

        def make(name, size, dtype):
            outs[name] = Guarded("numpy", size, dtype, 1, name=name)
            return outs[name].array

        bufs = buffers(h, make=make)
        with monkeypatch.context() as mp:
            if form == "general":
                mp.setenv("LA_NO_FUSED_STICKY", "1")
            rc = raw_call(ctx, h, mode, bufs, force=form == "forced", arrays={k: g.array for k, g in ins.items()})
        assert rc == N.LA_OK, (form, rc)
        same(bufs, exp, "%s, %s" % (mode, form))
        for g in ins.values():
            g.check_unchanged("%s, %s" % (mode, form))
        for g in outs.values():
            g.check_guards("%s, %s" % (mode, form))


# ---- 9: one context, many layouts -----------------------------------------------------------------------------------------------------------
def test_fifty_alternating_calls_on_one_context(ctx, torch_dev, monkeypatch):
    cases = [caught_up(33, [3, 0, 2], 2), caught_up(34, [40, 9, 25], 4), caught_up(35, [300, 150, 57], 6)]
    sticky_exp = [h.expect("lag") for h in cases]
    coop_exp = [sharding.assign_cooperative_numpy(h.part_off, h.pid, h.lag, h.cons_off, h.cons_rank, h.m, *h.owned, assign=oracle.assign_flat)
                for h in cases]
    grouped_exp = []
    for h in cases:
        t = oracle.assign_flat(h.part_off, h.pid, h.lag, h.cons_off, h.cons_rank)
        grouped_exp.append(tuple(sharding.group_by_member_numpy(h.part_off, t[0], t[1], h.m)) + (t[2],))
    for h, e in zip(cases, sticky_exp):
        three_ways(ctx, monkeypatch, h, "lag", e)
    for i in range(50):
        kind, s = i % 3, (i + i // 3) % 3
        h, what = cases[s], "call %d, size %d" % (i, s)
        if kind == 0:
            same(flat(host_call(ctx, h, "lag")), sticky_exp[s], what)
            assert ctx.last_pipeline() == N.LA_PIPELINE_ZERO_COPY
        elif kind == 1:
            got = ctx.assign_batch_cooperative(h.part_off, h.pid, h.cons_off, h.cons_rank, h.m, *h.owned, lag=h.lag)
            for name, g, e in zip(N.AssignCoop._fields, got, coop_exp[s]):
                np.testing.assert_array_equal(g, e, err_msg="%s %s" % (name, what))
        else:
            got = ctx.assign_batch_grouped(h.part_off, h.pid, None, h.lag, np.zeros(h.n, np.int64), N.LA_RESET_LATEST, h.cons_off, h.cons_rank,
                                           h.m)
            for name, g, e in zip(("member_off", "grouped_topic", "grouped_partition", "totals"), got, grouped_exp[s]):
                np.testing.assert_array_equal(g, e, err_msg="%s %s" % (name, what))


# ---- 10: three chained rebalances -----------------------------------------------------------------------------------------------------------
def chained(rounds=3):
    """The inputs of `rounds` rebalances of one caught-up group: new lags every time; the owned arrays of the first."""
    h = caught_up(36, [300, 200, 100], 6)
    rng = np.random.default_rng(37)
    return h, [S.caught_up_lags(h.n, 0.05, rng) for _ in range(rounds)]


def test_three_chained_rebalances(ctx, torch_dev, monkeypatch):
    h, lags = chained()
    owned = h.owned
    for r, lag in enumerate(lags):
        k = h.with_owned(owned, lag=lag)
        res = three_ways(ctx, monkeypatch, k, "lag", what="rebalance %d" % r)
        got = res["fused"][0]
        assert res["fused"][2] == N.LA_PIPELINE_ZERO_COPY and res["fused"][1] < res["general"][1]
        plain = ctx.assign_batch_cooperative(k.part_off, k.pid, k.cons_off, k.cons_rank, k.m, *owned, lag=lag)
        sticky_withheld, plain_withheld = int(got["summary"][2]), int(plain.summary[2])
        assert sticky_withheld < plain_withheld, "rebalance %d: the sticky round withholds %d partitions, la_assign_batch_cooperative %d" % (
            r, sticky_withheld, plain_withheld)
        owned = (got["member_off"], got["grouped_topic"], got["grouped_partition"])       # the lists are the next owned arrays


# ---- 11: two shards ---------------------------------------------------------------------------------------------------------------------------
def test_a_two_shard_context_takes_the_general_form(torch_dev, monkeypatch):
    c2 = N.Context([0, 0], flags=N.LA_CREATE_SPLIT_ALWAYS)
    try:
        h = caught_up(38, [90, 0, 300, 45, 7], 6)
        res = three_ways(c2, monkeypatch, h, "sparse", what="two shards")
        assert res["fused"][2] != N.LA_PIPELINE_ZERO_COPY and res["fused"][1] == res["general"][1]
    finally:
        c2.close()
