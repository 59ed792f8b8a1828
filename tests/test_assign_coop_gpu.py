"""la_assign_batch_cooperative on the GPU: a cooperative rebalance -- the assign call and the round on its result -- in one host
call.  Everything goes through ctypes on the C ABI.  The yardstick is sharding.assign_cooperative_numpy over the reference
oracle's assign_flat (tests/test_assign_coop_cpu.py holds it against a dictionary model).  Every comparison is bit for bit;
outputs hold SENTINEL before a call, every array is a view between guard bands at an element shift of its own, inputs must come
back unchanged."""
import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding
from oracle import oracle

from coop_cases import claims_from, layout, owned_arrays
from gpu_helpers import SENTINEL, Guarded, shifts_for

pytestmark = pytest.mark.gpu

LE, LO, LM, LT = N.COOP_SMALL_ENTRIES, N.COOP_SMALL_OWNED, N.COOP_SMALL_MEMBERS, N.COOP_SMALL_TOPICS
FIELDS = N.AssignCoop._fields
REQUIRED = ("member_off", "grouped_partition")
OPTIONAL = tuple(k for k in FIELDS if k not in REQUIRED)
ADJUST = FIELDS[3:11]
I64 = np.iinfo(np.int64)


class Rebalance:
    """The inputs of one cooperative rebalance on the host: the layout, the lags (and offsets that give them), who subscribes to
    what, who owns what."""

    def __init__(self, part_off, pid, lag, cons_off, cons_rank, m, owned=None):
        self.part_off, self.pid = np.ascontiguousarray(part_off, np.int64), np.ascontiguousarray(pid, np.int32)
        self.lag = np.ascontiguousarray(lag, np.int64)
        self.cons_off, self.cons_rank = np.ascontiguousarray(cons_off, np.int64), np.ascontiguousarray(cons_rank, np.int32)
        self.m = int(m)
        self.t, self.n, self.k = self.part_off.size - 1, self.pid.size, self.cons_rank.size
        self.set_owned(*(owned if owned is not None else (np.zeros(self.m + 1, np.int64), [], [])))

    def set_owned(self, off, topic, pid):
        self.owned_off = np.ascontiguousarray(off, np.int64)
        self.owned_topic, self.owned_pid = np.ascontiguousarray(topic, np.int32), np.ascontiguousarray(pid, np.int32)
        return self

    def sizes(self):
        n, m = self.n, self.m
        return dict(out_partition=n, out_member_rank=n, totals=self.k, prev_owner=n, coop_member_rank=n, kept=m, fresh=m, pending=m,
                    release=m, topic_withheld=self.t, summary=6, member_off=m + 1, grouped_topic=n, grouped_partition=n)

    def expect(self, lag=None):
        return sharding.assign_cooperative_numpy(self.part_off, self.pid, self.lag if lag is None else lag, self.cons_off,
                                                 self.cons_rank, self.m, self.owned_off, self.owned_topic, self.owned_pid,
                                                 assign=oracle.assign_flat)


def subscriptions(rng, t, m, none=()):
    """Every topic's subscribers: a random non-empty subset of the members, ascending; nobody for the topics in `none`."""
    segs = [np.empty(0, np.int64) if (i in none or m == 0) else np.sort(rng.choice(m, int(rng.integers(1, m + 1)), replace=False))
            for i in range(t)]
    off = np.concatenate([[0], np.cumsum([s.size for s in segs])]).astype(np.int64)
    return off, np.concatenate(segs + [np.empty(0, np.int64)]).astype(np.int32)


def rebalance(seed, sizes, m, ids="shuffled", none=(), lag_bits=40, **owned):
    rng = np.random.default_rng(seed)
    part_off, pid = layout(seed, sizes, ids)
    lag = rng.integers(0, 1 << lag_bits, pid.size)
    cons_off, cons_rank = subscriptions(rng, len(sizes), m, none)
    r = Rebalance(part_off, pid, lag, cons_off, cons_rank, m)
    head, tail = owned.pop("head", 0), owned.pop("tail", 0)
    if owned or head or tail:
        r.set_owned(*owned_arrays(m, claims_from(seed + 1, part_off, pid, m, **owned), head, tail, seed + 2))
    return r


def offsets_for(r, seed, frac_none=0.3):
    """begin / end / committed whose EARLIEST lags are r.lag where there is a committed offset."""
    rng = np.random.default_rng(seed)
    com = rng.integers(0, 1 << 20, r.n).astype(np.int64)
    com[rng.random(r.n) < frac_none] = -1
    begin = rng.integers(0, 1 << 19, r.n).astype(np.int64)
    end = np.maximum(com, begin) + r.lag
    return begin, end, com


INPUTS = ("part_off", "pid", "cons_off", "cons_rank", "owned_off", "owned_topic", "owned_pid")


def call(ctx, r, mode="lags", want=FIELDS, force=False, pattern="mixed", offsets=None, raw=False):
    """One call on guarded views.  Returns ({name: array}, guarded inputs, guarded outputs) after checking the guard bands, that
    the inputs are unchanged and that what was not wanted still holds SENTINEL; with raw=True the exception is the caller's."""
    data = {k: getattr(r, k) for k in INPUTS}
    if mode == "lags":
        data["lag"] = r.lag
    else:
        data["begin"], data["end"], data["committed"] = offsets
        if mode == "sparse":
            data["none_index"], data["none_begin"] = N.sparse_begin(data.pop("begin"), data["committed"])
        elif mode == "latest":
            data.pop("begin")
    shifts = shifts_for(pattern, tuple(data) + FIELDS)
    gi = {k: Guarded("numpy", v.size, v.dtype, shifts[k], v, name=k) for k, v in data.items()}
    sizes = r.sizes()
    go = {k: Guarded("numpy", sizes[k], np.int32 if k in ("out_partition", "out_member_rank", "prev_owner", "coop_member_rank",
                                                          "grouped_topic", "grouped_partition") else np.int64, shifts[k], name=k)
          for k in FIELDS}
    out = N.AssignCoop(*[go[k].array if k in want or k in REQUIRED else None for k in FIELDS])
    a = {k: g.array for k, g in gi.items()}
    kw = dict(lag=a.get("lag"), begin=a.get("begin"), end=a.get("end"), committed=a.get("committed"),
              none_index=a.get("none_index"), none_begin=a.get("none_begin"),
              reset_mode=N.LA_RESET_LATEST if mode == "latest" else N.LA_RESET_EARLIEST, force_table=force, out=out)

    def check(what):
        for k in FIELDS:
            go[k].check_guards(what)
        for g in gi.values():
            g.check_unchanged(what)

    try:
        ctx.assign_batch_cooperative(a["part_off"], a["pid"], a["cons_off"], a["cons_rank"], r.m, a["owned_off"] if r.owned_topic.size else None,
                                     a["owned_topic"], a["owned_pid"], **kw)
    except N.LagAssignError:
        check("after an error")
        for k in FIELDS:
            assert (go[k].array == SENTINEL).all(), "%s was written by a call that failed" % k
        raise
    check("")
    for k in FIELDS:
        if not (k in want or k in REQUIRED):
            assert (go[k].array == SENTINEL).all(), "%s was not asked for" % k
    return {k: go[k].array for k in FIELDS}, gi, go


def same(got, exp, want=FIELDS, what=""):
    for k, e in zip(FIELDS, exp):
        if k in want or k in REQUIRED:
            np.testing.assert_array_equal(got[k], e, err_msg="%s %s" % (k, what))


def exact(ctx, r, what="", fused=True, **kw):
    """The call as it comes and with LA_COOP_FORCE_TABLE: both exact; the first one fused where it should be."""
    exp = r.expect(kw.pop("lag", None))
    for force in (False, True):
        got, _, _ = call(ctx, r, force=force, **kw)
        same(got, exp, kw.get("want", FIELDS), "%s force=%s" % (what, force))
        if not force and fused is not None:
            assert (ctx.last_pipeline() == N.LA_PIPELINE_ZERO_COPY) or not fused, what
    return exp


# ---- the fused form, smallest shapes that can go wrong -------------------------------------------------------------------------------
def test_first_rebalance_with_a_lag_tie_equals_the_grouped_call(ctx, torch_dev):
    r = Rebalance([0, 3], [2, 0, 1], [5, 5, 1], [0, 2], [0, 1], 2)
    exp = exact(ctx, r)
    off, g_t, g_p, tot = ctx.assign_batch_grouped(r.part_off, r.pid, None, r.lag, np.zeros(3, np.int64), N.LA_RESET_LATEST, r.cons_off,
                                                  r.cons_rank, 2)
    got, _, _ = call(ctx, r)
    for k, e in (("member_off", off), ("grouped_topic", g_t), ("grouped_partition", g_p), ("totals", tot)):
        np.testing.assert_array_equal(got[k], e, err_msg=k)
    np.testing.assert_array_equal(got["summary"], [0, 3, 0, 0, 0, 0])
    assert exp[11][0] == 0


@pytest.mark.parametrize("ids", ["shuffled", "negative"])
def test_five_ragged_topics_with_padded_stale_and_unmapped_owned_entries(ctx, torch_dev, ids):
    r = rebalance(5, [0, 40, 7, 1, 23], 5, ids=ids, n_stale=9, n_unmapped=4, head=3, tail=2)
    assert r.owned_off[0] == 3 and r.owned_topic.size > r.owned_off[-1] and (r.owned_topic == -1).any()
    exp = exact(ctx, r, ids)
    assert exp[10][2] > 0 and exp[10][4] > 0                           # something withheld, something stale


def test_every_optional_output_is_null_in_turn_and_all_at_once(ctx, torch_dev):
    r = rebalance(6, [12, 0, 33, 5], 4, n_stale=3, n_unmapped=2, head=1, tail=1)
    exp = r.expect()
    for force in (False, True):
        for drop in OPTIONAL:
            if drop in ("out_partition", "out_member_rank"):
                continue
            want = tuple(k for k in FIELDS if k != drop)
            got, _, _ = call(ctx, r, want=want, force=force)
            same(got, exp, want, "without %s" % drop)
        for want in (tuple(k for k in FIELDS if k not in ("out_partition", "out_member_rank")), REQUIRED, REQUIRED + ("totals",),
                     REQUIRED + ("out_partition", "out_member_rank")):
            got, _, _ = call(ctx, r, want=want, force=force)
            same(got, exp, want, "only %s" % (want,))


@pytest.mark.parametrize("mode", ["dense", "sparse", "latest"])
def test_offsets_mode(ctx, torch_dev, mode):
    r = rebalance(7, [30, 3, 0, 19], 4, lag_bits=30, n_stale=2, head=1)
    begin, end, com = offsets_for(r, 8)
    lag = oracle.compute_lags(begin, end, com, mode == "latest")
    exp = exact(ctx, r, mode, mode=mode, offsets=(begin, end, com), lag=lag)
    if mode != "latest":
        assert (com < 0).any() and not np.array_equal(lag, r.lag)
    assert exp[2].size == r.k


def test_lags_over_the_full_int64_range(ctx, torch_dev):
    r = rebalance(9, [25, 4, 11], 3, n_stale=1, tail=2)
    rng = np.random.default_rng(9)
    r.lag = rng.integers(I64.min, I64.max, r.n, endpoint=True)
    r.lag[:4] = [I64.min, I64.max, -1, 0]
    exact(ctx, r)


def test_a_topic_with_no_consumer(ctx, torch_dev):
    r = rebalance(10, [6, 9, 4], 3, none=(1,), owned_frac=1.0)
    exp = exact(ctx, r)
    assert (exp[1][6:15] == -1).all() and exp[10][3] == 9             # owned by somebody, assigned to nobody: dropped
    assert exp[11][0] >= 9


def test_no_entries_no_topics_no_members(ctx, torch_dev):
    # N == 0 with topics (owned entries all stale)
    r = Rebalance([0, 0, 0], [], [], [0, 1, 3], [0, 0, 1], 2, owned=([0, 1, 2], [0, 1], [5, 6]))
    exp = exact(ctx, r, "N == 0", fused=None)
    np.testing.assert_array_equal(exp[10], [0, 0, 0, 0, 2, 0])
    # T == 0
    r = Rebalance([0], [], [], [0], [], 3)
    exp = exact(ctx, r, "T == 0", fused=None)
    np.testing.assert_array_equal(exp[11], [0, 0, 0, 0])
    # M == 0: nobody subscribes, nobody owns
    r = Rebalance([0, 2, 5], [1, 0, 2, 0, 1], [3, 4, 5, 6, 7], [0, 0, 0], [], 0)
    exp = exact(ctx, r, "M == 0")
    assert (exp[1] == -1).all() and exp[11].tolist() == [5]


# ---- the limits -----------------------------------------------------------------------------------------------------------------------
def limit_case(which, over):
    """Every limit reached at once; `which` one above it when `over`."""
    n = LE + (over if which == "N" else 0)
    t = LT + (over if which == "T" else 0)
    m = LM + (over if which == "M" else 0)
    rng = np.random.default_rng(40)
    sizes = np.ones(t, np.int64)                                         # one partition each ...
    sizes[-1] += n - t                                                   # ... but the last topic: two (N + 1) or none (T + 1)
    part_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pid = rng.integers(-5, 5, n).astype(np.int32)
    pid[-2:] = [7, 8]                                                    # (distinct where a topic has two)
    lag = rng.integers(0, 1 << 30, n)
    sub = rng.integers(0, m, t)                                          # one subscriber per topic; the last member among them
    sub[0] = m - 1
    cons_off, cons_rank = np.arange(t + 1, dtype=np.int64), sub.astype(np.int32)
    n_owned = LO + (over if which == "n_owned" else 0)
    owners = np.where(rng.random(n) < 0.7, rng.integers(0, m, n), -1)
    claims = claims_from(41, part_off, pid, m, owners=owners)
    claims = claims[:n_owned]
    pad = n_owned - len(claims)
    r = Rebalance(part_off, pid, lag, cons_off, cons_rank, m, owned=owned_arrays(m, claims, 0, pad, 42))
    assert r.owned_topic.size == n_owned
    return r


@pytest.mark.parametrize("over", [0, 1], ids=["at the limit", "one above"])
@pytest.mark.parametrize("which", ["N", "n_owned", "M", "T"])
def test_each_limit_and_one_above_it(ctx, torch_dev, which, over):
    r = limit_case(which, over)
    exp = r.expect()
    got, _, _ = call(ctx, r, pattern="aligned")
    same(got, exp, what="%s + %d" % (which, over))
    launches = ctx.last_launches()
    plain = ctx.assign_batch_lags(r.part_off, r.pid, r.lag, r.cons_off, r.cons_rank)
    if not over:
        assert ctx.last_launches() == launches, "the round takes the place of the finishing launch"
        assert ctx.last_pipeline() == N.LA_PIPELINE_ZERO_COPY
    else:
        assert launches > ctx.last_launches(), "the general form: the launches of both calls"
    np.testing.assert_array_equal(plain[0], exp[0])
    forced, _, _ = call(ctx, r, force=True, pattern="aligned")
    same(forced, exp, what="%s + %d, forced" % (which, over))


def test_a_block_path_topic_beside_small_ones(ctx, torch_dev):
    r = rebalance(43, [1500, 17, 0, 300, 64], 9, n_stale=20, n_unmapped=5, head=2, tail=2)
    assert r.n <= LE
    exact(ctx, r)


# ---- what the form promises -----------------------------------------------------------------------------------------------------------
def test_pipeline_launches_the_one_shot_hint_and_the_kept_target(ctx, torch_dev):
    r = rebalance(44, [40, 9, 25], 4, lag_bits=20, n_stale=2)
    exp = r.expect()
    bounds = N.offset_bounds(None, None, None, r.pid, lag=r.lag)
    assert bounds is not None
    ctx.hint_next_call(bounds)
    got, _, _ = call(ctx, r)
    same(got, exp, what="hinted")
    assert ctx.last_pipeline() == N.LA_PIPELINE_ZERO_COPY
    assert ctx.last_launches() == 2, "one tile launch, then the round"
    # the target stays on the device: its EAGER lists
    eager = ctx.group_last_by_member(r.n, r.m)
    for g, e in zip(eager, sharding.group_by_member_numpy(r.part_off, exp[0], exp[1], r.m)):
        np.testing.assert_array_equal(g, e)
    # the hint was spent: the same call again is an unhinted one, as la_assign_batch_lags counts it
    got, _, _ = call(ctx, r)
    same(got, exp, what="unhinted")
    unhinted = ctx.last_launches()
    ctx.assign_batch_lags(r.part_off, r.pid, r.lag, r.cons_off, r.cons_rank)
    assert ctx.last_launches() == unhinted
    ctx.hint_next_call(bounds)
    ctx.assign_batch_lags(r.part_off, r.pid, r.lag, r.cons_off, r.cons_rank)
    assert ctx.last_launches() == 2
    # a hint that an earlier, failing cooperative call took does not come back either
    ctx.hint_next_call(bounds)
    bad = Rebalance(r.part_off, r.pid, r.lag, r.cons_off, r.cons_rank, r.m, owned=([0, 1, 2, 2, 2], [0, 0], [r.pid[0], r.pid[0]]))
    with pytest.raises(N.LagAssignError):
        call(ctx, bad)
    got, _, _ = call(ctx, r)
    assert ctx.last_launches() == unhinted
    same(got, exp, what="after a failed hinted call")


# ---- errors, each followed by correct calls on the same context -------------------------------------------------------------------------
def broken(bad):
    r = rebalance(50, [20, 30, 20], 5, lag_bits=20, owned_frac=1.0, n_unmapped=2, head=2, tail=2)
    lo, hi = int(r.owned_off[0]), int(r.owned_off[-1])
    live = np.flatnonzero(r.owned_topic[lo:hi] >= 0) + lo
    kw, hint, code = {}, None, N.LA_EINVAL
    if bad == "duplicate claim":
        r.owned_topic[live[-1]], r.owned_pid[live[-1]] = r.owned_topic[live[0]], r.owned_pid[live[0]]
    elif bad == "owned topic T":
        r.owned_topic[live[1]] = r.t
    elif bad == "owned topic -2":
        r.owned_topic[live[1]] = -2
    elif bad == "owned offsets descend":
        r.owned_off[1], r.owned_off[2] = r.owned_off[2] + 1, r.owned_off[1]
        code = N.LA_ESHAPE
    elif bad == "unsorted cons_rank":
        seg = slice(int(r.cons_off[1]), int(r.cons_off[2]))
        if r.cons_rank[seg].size < 2:
            r.cons_off[2:] += 1
            r.cons_rank = np.concatenate([r.cons_rank[:seg.stop], [0], r.cons_rank[seg.stop:]]).astype(np.int32)
            r.k += 1
            seg = slice(seg.start, seg.stop + 1)
        r.cons_rank[seg] = r.cons_rank[seg][::-1]
    elif bad == "sparse list out of order":
        begin, end, com = offsets_for(r, 51, 0.5)
        kw = dict(mode="sparse", offsets=(begin, end, com))
    else:
        raise ValueError(bad)
    return r, kw, hint, code


@pytest.mark.parametrize("force", [False, True], ids=["fused", "general"])
@pytest.mark.parametrize("bad", ["duplicate claim", "owned topic T", "owned topic -2", "owned offsets descend", "unsorted cons_rank",
                                 "sparse list out of order"])
def test_an_error_leaves_the_outputs_alone_and_nothing_behind(ctx, torch_dev, bad, force, monkeypatch):
    good = rebalance(52, [20, 30, 20], 5, lag_bits=20, n_stale=3, head=1)
    exp = good.expect()
    r, kw, hint, code = broken(bad)
    if bad == "sparse list out of order":
        real = N.sparse_begin
        monkeypatch.setattr(N, "sparse_begin", lambda b, c: tuple(x[::-1].copy() for x in real(b, c)))
    if hint:
        ctx.hint_next_call(hint)
    with pytest.raises(N.LagAssignError) as ei:
        call(ctx, r, force=force, **kw)                                  # (checks every output for its sentinel)
    assert ei.value.code == code, ei.value
    monkeypatch.undo()
    # the leftover-status and leftover-counter hazard: the next calls on this context are exact
    got, _, _ = call(ctx, good, force=force)
    same(got, exp, what="after %s" % bad)
    off, g_t, g_p, tot = ctx.assign_batch_grouped(good.part_off, good.pid, None, good.lag, np.zeros(good.n, np.int64), N.LA_RESET_LATEST,
                                                  good.cons_off, good.cons_rank, good.m)
    for g, e in zip((off, g_t, g_p), sharding.group_by_member_numpy(good.part_off, exp[0], exp[1], good.m)):
        np.testing.assert_array_equal(g, e, err_msg="grouped after %s" % bad)
    np.testing.assert_array_equal(tot, exp[2])


def test_a_violated_bounds_hint(ctx, torch_dev):
    """The assign kernels report a broken promise only where a tile that does not pack has no wide-record code beside it: a batch
    beyond one round of resident workgroups (tests/test_host_calls_gpu.py, test_violated_hint_is_einval_never_a_different_result).
    A batch within the fused form's limits always runs the single launch with the wide code inline, where a wrong bound is
    harmless -- for la_assign_batch_lags and for this call alike.  So the error is met in the general form, on a batch of the
    size that test uses; the small batch shows the composition: the same result with and without the wrong hint."""
    from kafka_lag_based_assignor_amd import synth
    good = rebalance(52, [20, 30, 20], 5, lag_bits=20, n_stale=3, head=1)
    good.lag[7] = 1 << 62
    exp = good.expect()
    for wrong in ((1 << 31, 255), None):
        ctx.hint_next_call(wrong)
        plain = ctx.assign_batch_lags(good.part_off, good.pid, good.lag, good.cons_off, good.cons_rank)
        np.testing.assert_array_equal(plain[1], exp[1])
        ctx.hint_next_call(wrong)
        got, _, _ = call(ctx, good)
        same(got, exp, what="small batch, hint %s" % (wrong,))
        assert ctx.last_pipeline() == N.LA_PIPELINE_ZERO_COPY
    z = synth.make_uniform("wake", 52, 3000, 256, 32, "zipf")
    big = z.end.copy()
    big[1234] = 1 << 56                                              # its tile needs wide records: breaks a bound of 2^31
    m = int(z.cons_rank.max()) + 1
    sizes = dict(out_partition=z.n_partitions, out_member_rank=z.n_partitions, totals=z.cons_rank.size, prev_owner=z.n_partitions,
                 coop_member_rank=z.n_partitions, kept=m, fresh=m, pending=m, release=m, topic_withheld=z.n_topics, summary=6,
                 member_off=m + 1, grouped_topic=z.n_partitions, grouped_partition=z.n_partitions)
    out = N.AssignCoop(*[np.full(sizes[k], SENTINEL, np.int32 if k in ("out_partition", "out_member_rank", "prev_owner", "coop_member_rank",
                                                                      "grouped_topic", "grouped_partition") else np.int64) for k in FIELDS])
    ctx.hint_next_call((1 << 31, 255))
    with pytest.raises(N.LagAssignError) as ei:
        ctx.assign_batch_cooperative(z.part_off, z.partition_id, z.cons_off, z.cons_rank, m, None, None, None, begin=z.begin, end=big,
                                     committed=z.committed, reset_mode=N.LA_RESET_EARLIEST, out=out)
    assert ei.value.code == N.LA_EINVAL and "bounds" in str(ei.value)
    for k, a in zip(FIELDS, out):
        assert (a == SENTINEL).all(), "%s was written by a call that failed" % k
    good.lag[7] = 5
    exp = good.expect()
    got, _, _ = call(ctx, good)                                      # the hint went with the failing call; nothing else stayed behind
    same(got, exp, what="after the violated hint")
    off, g_t, g_p, tot = ctx.assign_batch_grouped(good.part_off, good.pid, None, good.lag, np.zeros(good.n, np.int64), N.LA_RESET_LATEST,
                                                  good.cons_off, good.cons_rank, good.m)
    for g, e in zip((off, g_t, g_p), sharding.group_by_member_numpy(good.part_off, exp[0], exp[1], good.m)):
        np.testing.assert_array_equal(g, e)


def test_fifty_alternating_calls_on_one_context(ctx, torch_dev):
    cases = [rebalance(60 + i, [int(x) for x in np.random.default_rng(60 + i).integers(0, 30, 1 + i % 5)], 1 + i % 6,
                       lag_bits=20, n_stale=i % 3, head=i % 2) for i in range(6)]
    exps = [c.expect() for c in cases]
    for i in range(50):
        r, exp = cases[i % 6], exps[i % 6]
        kind = i % 3
        if kind == 0:
            got = ctx.assign_batch_cooperative(r.part_off, r.pid, r.cons_off, r.cons_rank, r.m, r.owned_off, r.owned_topic, r.owned_pid,
                                               lag=r.lag)
            for k, g, e in zip(FIELDS, got, exp):
                np.testing.assert_array_equal(g, e, err_msg="%s, call %d" % (k, i))
        elif kind == 1:
            got = ctx.assign_batch_grouped(r.part_off, r.pid, None, r.lag, np.zeros(r.n, np.int64), N.LA_RESET_LATEST, r.cons_off,
                                           r.cons_rank, r.m)
            for g, e in zip(got[:3], sharding.group_by_member_numpy(r.part_off, exp[0], exp[1], r.m)):
                np.testing.assert_array_equal(g, e, err_msg="grouped, call %d" % i)
        else:
            got = ctx.assign_batch_lags(r.part_off, r.pid, r.lag, r.cons_off, r.cons_rank)
            for g, e in zip(got, exp[:3]):
                np.testing.assert_array_equal(g, e, err_msg="plain, call %d" % i)


# ---- buffer contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", [False, True], ids=["fused", "general"])
@pytest.mark.parametrize("pattern", ["aligned", "odd", "three"])
def test_buffer_contract_at_every_element_shift(ctx, torch_dev, pattern, force):
    r = rebalance(70, [33, 1, 0, 65, 14], 6, ids="negative", n_stale=5, n_unmapped=3, head=3, tail=3)
    got, gi, go = call(ctx, r, pattern=pattern, force=force)         # (guards and inputs are checked inside)
    same(got, r.expect(), what=pattern)
    assert all(g.shift == {"aligned": 0, "odd": 1, "three": 3}[pattern] for g in list(gi.values()) + list(go.values()))


# ---- a chain on the device path ---------------------------------------------------------------------------------------------------------
def test_three_rebalances_chained_the_lists_of_one_are_the_owned_arrays_of_the_next(ctx, torch_dev):
    rng = np.random.default_rng(80)
    sizes, m = [30, 0, 12, 55, 7], 5
    part_off, pid = layout(80, sizes)
    topic = np.repeat(np.arange(len(sizes)), sizes)
    # rebalance 0 (eager): what everybody owns to begin with
    r0 = rebalance(80, sizes, m, lag_bits=20)
    e0 = r0.expect()
    owned = (e0[11], e0[12], e0[13])
    assert e0[10][5] == 0
    # rebalance 1: other lags, other subscriptions -- rounds until no follow-up is asked for, two at the most
    lag = rng.integers(0, 1 << 20, pid.size)
    cons_off, cons_rank = subscriptions(rng, len(sizes), m)
    eager = sharding.group_by_member_numpy(part_off, *oracle.assign_flat(part_off, pid, lag, cons_off, cons_rank)[:2], m)
    rounds = 0
    for rounds in range(1, 4):
        r = Rebalance(part_off, pid, lag, cons_off, cons_rank, m, owned=owned)
        exp = r.expect()
        got, _, _ = call(ctx, r)
        same(got, exp, what="round %d" % rounds)
        assert ctx.last_pipeline() == N.LA_PIPELINE_ZERO_COPY
        # safety: nobody is handed what another member still owns
        lo = int(owned[0][0])
        owner = {(int(t), int(i)): int(np.searchsorted(owned[0], j, side="right") - 1)
                 for j, (t, i) in enumerate(zip(owned[1][lo:], owned[2][lo:]), lo)}
        off = got["member_off"]
        for j in range(int(off[0]), r.n):
            who = int(np.searchsorted(off, j, side="right") - 1)
            assert owner.get((int(got["grouped_topic"][j]), int(got["grouped_partition"][j])), who) == who
        owned = (got["member_off"].copy(), got["grouped_topic"].copy(), got["grouped_partition"].copy())   # as they lie, head included
        if got["summary"][5] == 0:
            break
    assert rounds <= 2 and got["summary"][5] == 0
    lo = int(owned[0][0])
    np.testing.assert_array_equal(owned[0], eager[0])
    np.testing.assert_array_equal(owned[1][lo:], eager[1][lo:])
    np.testing.assert_array_equal(owned[2][lo:], eager[2][lo:])
    assert topic.size == pid.size


# ---- the general form beyond one staging buffer / one shard ----------------------------------------------------------------------------
def test_a_two_shard_context_takes_the_general_form(torch_dev):
    c2 = N.Context([0, 0], flags=N.LA_CREATE_SPLIT_ALWAYS)
    try:
        r = rebalance(90, [90, 0, 300, 45, 7], 6, n_stale=10, n_unmapped=4, head=2, tail=2)
        got, _, _ = call(c2, r)
        same(got, r.expect())
    finally:
        c2.close()


# ---- plugin level -------------------------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments(ctx, torch_dev):
    import ctypes
    lib = N.load()
    r = rebalance(91, [5, 6], 2)
    keep = dict(part_off=r.part_off, pid=r.pid, lag=r.lag, cons_off=r.cons_off, cons_rank=r.cons_rank,
                off=np.full(3, SENTINEL, np.int64), gp=np.full(r.n, SENTINEL, np.int32))

    def args():
        g = N.AssignCoopArgs()
        g.struct_size, g.n_topics, g.n_members = ctypes.sizeof(N.AssignCoopArgs), r.t, r.m
        g.part_off, g.partition_id, g.lag = keep["part_off"].ctypes.data, keep["pid"].ctypes.data, keep["lag"].ctypes.data
        g.cons_off, g.cons_rank = keep["cons_off"].ctypes.data, keep["cons_rank"].ctypes.data
        g.member_off, g.grouped_partition = keep["off"].ctypes.data, keep["gp"].ctypes.data
        return g

    for name, change in (("struct_size", lambda g: setattr(g, "struct_size", g.struct_size - 8)), ("flags", lambda g: setattr(g, "flags", 2)),
                         ("reserved", lambda g: setattr(g, "reserved", 1)), ("n_members", lambda g: setattr(g, "n_members", -1)),
                         ("n_owned", lambda g: setattr(g, "n_owned", 3)), ("member_off", lambda g: setattr(g, "member_off", None)),
                         ("grouped_partition", lambda g: setattr(g, "grouped_partition", None)),
                         ("out_partition alone", lambda g: setattr(g, "out_partition", keep["gp"].ctypes.data))):
        g = args()
        change(g)
        assert lib.la_assign_batch_cooperative(ctx._h, ctypes.byref(g)) == N.LA_EINVAL, name
        assert (keep["off"] == SENTINEL).all() and (keep["gp"] == SENTINEL).all(), name
    assert lib.la_assign_batch_cooperative(ctx._h, None) == N.LA_EINVAL
    assert lib.la_assign_batch_cooperative(None, ctypes.byref(args())) == N.LA_EINVAL
    g = args()
    assert lib.la_assign_batch_cooperative(ctx._h, ctypes.byref(g)) == N.LA_OK
    exp = r.expect()
    np.testing.assert_array_equal(keep["off"], exp[11])
    np.testing.assert_array_equal(keep["gp"], exp[13])
    with pytest.raises(ValueError):
        ctx.assign_batch_cooperative(r.part_off, r.pid, r.cons_off, r.cons_rank, r.m, None, None, None, lag=r.lag,
                                     out=N.AssignCoop(*([None] * 11), np.zeros(r.m + 1, np.int64), None, np.zeros(2 * r.n, np.int32)[::2]))


# ---- plugin level: the host that speaks cooperative -------------------------------------------------------------------------------------------
class FakeOffsets:
    """Plays the side KafkaConsumer: one call per kind for ALL partitions."""

    def __init__(self, begin, end, committed):
        self.begin, self.end, self.com = begin, end, committed

    def beginning_offsets(self, tps):
        return {tp: self.begin[tp] for tp in tps if tp in self.begin}

    def end_offsets(self, tps):
        return {tp: self.end[tp] for tp in tps if tp in self.end}

    def committed(self, tps):
        return {tp: self.com.get(tp) for tp in tps}


def offsets_fixture():
    """The metadata and offsets of test_plugin_level_assign_with_offsets (tests/test_reference_suite_gpu.py)."""
    import random
    rng = random.Random(5)
    metadata = {"orders": list(range(12)), "payments": list(range(5)), "empty": []}
    begin, end, com = {}, {}, {}
    for t, ps in metadata.items():
        for p in ps:
            b = rng.randint(0, 100)
            e = b + rng.randint(0, 10000)
            begin[(t, p)], end[(t, p)] = b, e
            if rng.random() < 0.7:
                com[(t, p)] = rng.randint(b, e)
    del end[("orders", 3)]
    return metadata, FakeOffsets(begin, end, com)


def round_numbers(metadata, subs, target, owned):
    """kept / fresh / pending / release per member, withheld per topic and the summary through sharding.cooperative_round_numpy."""
    from kafka_lag_based_assignor_amd.assignor import _host
    h = _host()
    members = list(subs)
    rank = dict(zip(members, h.rank_members(members)))
    topics = [t for t, ps in metadata.items() if ps]
    entries = {t: [] for t in topics}
    for m, tps in target.items():
        for t, p in tps:
            entries[t].append((p, rank[m]))
    held = {tp for tps in target.values() for tp in tps}
    for t in topics:                                                   # partitions of topics nobody consumes
        entries[t] += [(p, -1) for p in metadata[t] if (t, p) not in held]
    part_off = np.concatenate([[0], np.cumsum([len(entries[t]) for t in topics])])
    flat = [e for t in topics for e in entries[t]]
    off, o_topic, o_pid = h.cooperative_owned_arrays(members, topics, [list(owned.get(m, ())) for m in members])
    out = sharding.cooperative_round_numpy(part_off, [e[0] for e in flat], [e[1] for e in flat], len(members), off, o_topic, o_pid)
    per = {m: tuple(int(out[2 + w][rank[m]]) for w in range(4)) for m in members}
    return per, dict(zip(topics, out[6].tolist())), out[7].tolist()


def test_plugin_level_cooperative_assign():
    from kafka_lag_based_assignor_amd.assignor import LagBasedPartitionAssignor
    assert LagBasedPartitionAssignor.supported_protocols() == ["COOPERATIVE", "EAGER"]
    metadata, src = offsets_fixture()
    subs = {"app-2": ["orders", "payments", "nometa"], "app-10": ["orders"], "app-1": ["payments", "empty"]}
    a = LagBasedPartitionAssignor()
    a.configure({"group.id": "g", "auto.offset.reset": "earliest"})
    eager = a.assign(metadata, subs, src)
    totals, loads = a.last_topic_totals(), a.last_member_loads()
    # nothing owned: assign(), list for list, and the same description of the target
    first = a.assign_cooperative(metadata, subs, {}, src)
    assert first == eager
    assert a.last_native_call()["launches"] == 2 and a.last_native_call()["hinted"]
    assert a.last_topic_totals() == totals and a.last_member_loads() == loads
    c = a.last_cooperative_round()
    assert (c["kept"], c["fresh"], c["withheld"], c["dropped"], c["stale"], c["followup"]) == (0, 17, 0, 0, 0, False)
    # a member leaves, a member joins: rounds until no follow-up is asked for
    subs2 = {"app-2": ["orders", "payments", "nometa"], "app-10": ["orders"], "app-3": ["payments", "orders"]}
    target = a.assign(metadata, subs2, src)
    target_loads = a.last_member_loads()
    owned = {m: list(tps) for m, tps in eager.items() if m in subs2}
    owned["app-2"] = owned["app-2"] + [("deleted", 4)]                  # a stale claim
    for rounds in (1, 2):
        got = a.assign_cooperative(metadata, subs2, owned, src)
        c = a.last_cooperative_round()
        per, withheld, summary = round_numbers(metadata, subs2, target, owned)
        assert c["per_member"] == per, rounds
        assert {t: n for t, n in c["topic_withheld"].items() if n} == {t: n for t, n in withheld.items() if n}
        assert [c["kept"], c["fresh"], c["withheld"], c["dropped"], c["stale"], int(c["followup"])] == summary, rounds
        assert a.last_member_loads() == target_loads                   # counts of the TARGET, not of the adjusted lists
        was = {tp: m for m, tps in owned.items() for tp in tps}
        assert all(was.get(tuple(tp), m) == m for m, tps in got.items() for tp in tps), "handed out while still owned"
        owned = {m: list(tps) for m, tps in got.items()}
        if not c["followup"]:
            break
    assert rounds == 2 and not c["followup"]
    assert got == target
    # the debug hook describes the target
    said, said_eager = [], []
    a.set_debug(said.append)
    a.assign_cooperative(metadata, subs2, {m: list(tps) for m, tps in eager.items() if m in subs2}, src)
    a.set_debug(said_eager.append)
    a.assign(metadata, subs2, src)
    assert said == said_eager and len(said) > 0
    # a partition claimed twice
    with pytest.raises(ValueError):
        a.assign_cooperative(metadata, subs2, {"app-2": [("orders", 1)], "app-10": [("orders", 1)]}, src)
    assert a.assign_cooperative(metadata, subs2, owned, src) == target
