"""LA_COOP_PINNED on the GPU: la_assign_batch_cooperative whose target is the pinned assignment, and the host mirror's
lag.assignor.cooperative.followup.  The yardstick is sharding.assign_pinned_numpy followed by sharding.cooperative_round_numpy
(tests/test_pinned_cpu.py holds the former against a dictionary model).  Every comparison is bit for bit; outputs hold SENTINEL
before a call, every array is a view between guard bands, inputs must come back unchanged."""
import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding
from oracle import oracle

from gpu_helpers import SENTINEL, Guarded, shifts_for
from pinned_cases import CASES, OVER, Scenario, drawn

pytestmark = pytest.mark.gpu

FIELDS = N.AssignCoop._fields
INT32 = ("out_partition", "out_member_rank", "prev_owner", "coop_member_rank", "grouped_topic", "grouped_partition")
INPUTS = ("part_off", "pid", "cons_off", "cons_rank", "owned_off", "owned_topic", "owned_pid")
HOST_CASES = ("the worked case", "a foreign claimant", "topic -1 and entries outside the offsets", "C = 0 with claims", "P = 0",
              "one consumer at 0, the others at 40", "negative lags, totals that wrap", "1024 and 1025 partitions")


def expect(c, pinned=True):
    """The call restated: the pinned target (or the oracle's), then the round on it."""
    assign = (lambda *a: c.expect()[:3]) if pinned else oracle.assign_flat
    return sharding.assign_cooperative_numpy(*c.args(), assign=assign)


def call(ctx, c, mode="lags", offsets=None, pinned=True, pattern="mixed", force=False):
    """One call on guarded views -> {name: array}; after an error the outputs must still hold SENTINEL."""
    data = {k: getattr(c, k) for k in INPUTS}
    if mode == "lags":
        data["lag"] = c.lag
    else:
        data["begin"], data["end"], data["committed"] = offsets
        if mode == "sparse":
            data["none_index"], data["none_begin"] = N.sparse_begin(data.pop("begin"), data["committed"])
        elif mode == "latest":
            data.pop("begin")
    shifts = shifts_for(pattern, tuple(data) + FIELDS)
    gi = {k: Guarded("numpy", v.size, v.dtype, shifts[k], v, name=k) for k, v in data.items()}
    sizes = dict(out_partition=c.n, out_member_rank=c.n, totals=c.k, prev_owner=c.n, coop_member_rank=c.n, kept=c.m, fresh=c.m,
                 pending=c.m, release=c.m, topic_withheld=c.t, summary=6, member_off=c.m + 1, grouped_topic=c.n, grouped_partition=c.n)
    go = {k: Guarded("numpy", sizes[k], np.int32 if k in INT32 else np.int64, shifts[k], name=k) for k in FIELDS}
    a = {k: g.array for k, g in gi.items()}

    def check(what):
        for g in go.values():
            g.check_guards(what)
        for g in gi.values():
            g.check_unchanged(what)

    try:
        ctx.assign_batch_cooperative(a["part_off"], a["pid"], a["cons_off"], a["cons_rank"], c.m, a["owned_off"], a["owned_topic"],
                                     a["owned_pid"], lag=a.get("lag"), begin=a.get("begin"), end=a.get("end"),
                                     committed=a.get("committed"), none_index=a.get("none_index"), none_begin=a.get("none_begin"),
                                     reset_mode=N.LA_RESET_LATEST if mode == "latest" else N.LA_RESET_EARLIEST, force_table=force,
                                     out=N.AssignCoop(*[go[k].array for k in FIELDS]), pinned=pinned)
    except N.LagAssignError:
        check("after an error")
        for k in FIELDS:
            assert (go[k].array == SENTINEL).all(), "%s was written by a call that failed" % k
        raise
    check("")
    return {k: go[k].array for k in FIELDS}


def same(got, exp, what=""):
    for k, e in zip(FIELDS, exp):
        np.testing.assert_array_equal(got[k], e, err_msg="%s %s" % (k, what))


@pytest.mark.parametrize("name", HOST_CASES)
def test_the_flag_from_lags_equals_pinned_numpy_then_the_round(ctx, name):
    c = CASES[name]()
    same(call(ctx, c, pattern=("aligned", "mixed")[HOST_CASES.index(name) % 2]), expect(c), name)


@pytest.mark.parametrize("mode", ["dense", "sparse", "latest"])
@pytest.mark.parametrize("force", [False, True])
def test_the_flag_from_offsets(ctx, mode, force):
    c = drawn(50, [(70, 4), (0, 2), (300, 9), (25, 0)], 9, owned=0.6, foreign=0.2, n_stale=3, n_unmapped=2, head=1, tail=2)
    rng = np.random.default_rng(50)
    committed = rng.integers(0, 1 << 20, c.n).astype(np.int64)
    committed[rng.random(c.n) < 0.3] = -1
    begin = rng.integers(1, 1 << 19, c.n).astype(np.int64)            # non-zero: a dropped sparse entry would show
    end = np.maximum(committed, begin) + rng.integers(0, 1 << 18, c.n)
    c.lag = oracle.compute_lags(begin, end, committed, mode == "latest")
    same(call(ctx, c, mode, (begin, end, committed), force=force), expect(c), "%s force=%s" % (mode, force))


def test_without_the_flag_nothing_differs(ctx):
    c = drawn(51, [(70, 4), (0, 2), (300, 9), (25, 0)], 9, owned=0.6, foreign=0.2, n_stale=3)
    same(call(ctx, c, pinned=False), expect(c, pinned=False), "flag off")
    got = call(ctx, c)
    same(got, expect(c), "flag on")
    assert not np.array_equal(got["out_member_rank"], expect(c, pinned=False)[1])      # (the two targets do differ here)


def test_empty_calls(ctx):
    for shapes, m in (([], 0), ([], 3), ([(0, 0)], 2), ([(0, 2), (0, 0)], 2)):
        c = drawn(52, shapes, m)
        same(call(ctx, c), expect(c), str(shapes))


@pytest.mark.parametrize("name", list(OVER))
def test_a_topic_over_the_limits_is_eshape_at_the_call_with_nothing_enqueued(ctx, name):
    c = OVER[name]()
    with pytest.raises(N.LagAssignError) as e:
        call(ctx, c)
    assert e.value.code == N.LA_ESHAPE
    assert ctx.last_launches() == 0
    same(call(ctx, c, pinned=False), expect(c, pinned=False), "the full form takes it")


def test_every_other_entry_refuses_the_bit(ctx):
    r = N.CoopRoundArgs()
    r.flags = N.LA_COOP_PINNED
    with pytest.raises(N.LagAssignError) as e:
        ctx.cooperative_round_device(r, 0)
    assert e.value.code == N.LA_EINVAL
    s = N.CoopStickyArgs()
    s.flags = N.LA_COOP_PINNED
    with pytest.raises(N.LagAssignError) as e:
        ctx.cooperative_round_sticky_device(N.DeviceBatch(), s, 0)
    assert e.value.code == N.LA_EINVAL
    import ctypes
    a = N.AssignStickyArgs()
    a.struct_size = ctypes.sizeof(N.AssignStickyArgs)
    a.coop.flags = N.LA_COOP_PINNED
    assert N.load().la_assign_batch_cooperative_sticky(ctx._h, ctypes.byref(a)) == N.LA_EINVAL


# ---- the host mirror: lag.assignor.cooperative.followup ---------------------------------------------------------------------------
class Offsets:
    """end - committed = the lag; everything committed."""

    def __init__(self, lag_of):
        self.lag_of = lag_of

    def beginning_offsets(self, tps):
        return {tp: 0 for tp in tps}

    def end_offsets(self, tps):
        return {tp: 1000 + self.lag_of[tp] for tp in tps}

    def committed(self, tps):
        return {tp: 1000 for tp in tps}


def mirror_rounds(conf, followups=2):
    """The settling scenario through the host mirror: a settled group of 4 x 64 x 8, one rebalance, then follow-ups ->
    last_cooperative_round() of each call after the settling one, and whether a list ever lost what its member owned."""
    from kafka_lag_based_assignor_amd.assignor import LagBasedPartitionAssignor
    s = Scenario(7, 4, 64, 8)
    topics = ["topic-%d" % t for t in range(s.t)]
    members = ["m%d" % r for r in range(s.m)]
    metadata = {t: list(range(s.p)) for t in topics}
    subs = {m: list(topics) for m in members}
    a = LagBasedPartitionAssignor()
    a.configure(dict({"group.id": "g", "auto.offset.reset": "earliest"}, **conf))
    lags = lambda: {(t, p): int(s.lag[i * s.p + p]) for i, t in enumerate(topics) for p in range(s.p)}
    owned = a.assign_cooperative(metadata, subs, {}, Offsets(lags()))
    assert not a.last_cooperative_round()["followup"]
    rounds, moved = [], 0
    for _ in range(1 + followups):
        s.grow()
        got = a.assign_cooperative(metadata, subs, owned, Offsets(lags()))
        c = a.last_cooperative_round()
        was = {tuple(tp): m for m, tps in owned.items() for tp in tps}
        moved += sum(1 for m, tps in got.items() for tp in tps if was.get(tuple(tp), m) != m)
        if c["pinned"]:                                              # a pinned follow-up takes nothing away
            assert all(set(map(tuple, owned[m])) <= set(map(tuple, got[m])) for m in members)
        rounds.append(c)
        owned = got
    return a, rounds, moved


def test_the_mirror_with_pinned_followups_settles_in_one():
    a, rounds, moved = mirror_rounds({"lag.assignor.cooperative.followup": "pinned"})
    assert a.cooperative_followup() == "pinned" and moved == 0
    first, second, third = rounds
    assert not first["pinned"] and first["withheld"] > 0 and first["followup"]
    assert second["pinned"] and (second["withheld"], second["dropped"], second["followup"]) == (0, 0, False)
    assert second["pinned_free"] == first["withheld"] and second["pinned_foreign"] == 0
    assert second["kept"] + second["fresh"] == 4 * 64 and second["fresh"] == first["withheld"]
    assert not third["pinned"]                                       # the group had settled: the next rebalance is a full one


def test_the_mirror_with_the_default_behaves_as_before():
    from kafka_lag_based_assignor_amd.assignor import LagBasedPartitionAssignor
    a, rounds, moved = mirror_rounds({})
    b, rounds_full, _ = mirror_rounds({"lag.assignor.cooperative.followup": "full"})
    assert a.cooperative_followup() == "full" and b.cooperative_followup() == "full" and moved == 0
    assert rounds == rounds_full
    assert all(not c["pinned"] and c["pinned_free"] == 0 and c["pinned_foreign"] == 0 for c in rounds)
    assert all(c["withheld"] > 0 and c["followup"] for c in rounds)  # the full form never settles here
    with pytest.raises(ValueError):
        LagBasedPartitionAssignor().configure({"group.id": "g", "lag.assignor.cooperative.followup": "sticky"})


def test_the_mirror_falls_back_when_the_group_changed():
    from kafka_lag_based_assignor_amd.assignor import LagBasedPartitionAssignor
    s = Scenario(8, 2, 32, 4)
    topics, members = ["a", "b"], ["m0", "m1", "m2", "m3"]
    metadata = {t: list(range(s.p)) for t in topics}
    lags = lambda: {(t, p): int(s.lag[i * s.p + p]) for i, t in enumerate(topics) for p in range(s.p)}
    a = LagBasedPartitionAssignor()
    a.configure({"group.id": "g", "auto.offset.reset": "earliest", "lag.assignor.cooperative.followup": "pinned"})
    subs = {m: list(topics) for m in members}
    owned = a.assign_cooperative(metadata, subs, {}, Offsets(lags()))
    s.grow()
    owned = a.assign_cooperative(metadata, subs, owned, Offsets(lags()))
    assert a.last_cooperative_round()["followup"]
    s.grow()
    fewer = {m: list(topics) for m in members[:3]}                   # a member left in between: not the follow-up of that round
    got = a.assign_cooperative(metadata, fewer, {m: owned[m] for m in fewer}, Offsets(lags()))
    assert not a.last_cooperative_round()["pinned"]
    if a.last_cooperative_round()["followup"]:
        s.grow()
        a.assign_cooperative(metadata, fewer, got, Offsets(lags()))
        assert a.last_cooperative_round()["pinned"] and not a.last_cooperative_round()["followup"]
