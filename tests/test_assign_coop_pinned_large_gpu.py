"""LA_COOP_PINNED | LA_COOP_PINNED_LARGE on the GPU: la_assign_batch_cooperative whose target is the pinned assignment of topics
of any size, and the host mirror's lag.assignor.cooperative.followup.large.  The yardstick is the dictionary model of
pinned_cases.py with its limit lifted followed by sharding.cooperative_round_numpy.  Every comparison is bit for bit; outputs
hold SENTINEL before a call, every array is a view between guard bands, inputs must come back unchanged."""
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding

import pinned_large_cases as PL
from gpu_helpers import SENTINEL, Guarded, shifts_for
from pinned_cases import Scenario
from test_assign_coop_pinned_gpu import Offsets

pytestmark = pytest.mark.gpu

FIELDS = N.AssignCoop._fields
INT32 = ("out_partition", "out_member_rank", "prev_owner", "coop_member_rank", "grouped_topic", "grouped_partition")
INPUTS = ("part_off", "pid", "cons_off", "cons_rank", "owned_off", "owned_topic", "owned_pid", "lag")


def call(ctx, c, pinned=True, pinned_large=True, pattern="mixed"):
    """One call from lags on guarded views -> {name: array}; after an error the outputs must still hold SENTINEL."""
    data = {k: getattr(c, k) for k in INPUTS}
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
                                     a["owned_pid"], lag=a["lag"], out=N.AssignCoop(*[go[k].array for k in FIELDS]),
                                     pinned=pinned, pinned_large=pinned_large)
    except N.LagAssignError:
        check("after an error")
        for k in FIELDS:
            assert (go[k].array == SENTINEL).all(), "%s was written by a call that failed" % k
        raise
    check("")
    return {k: go[k].array for k in FIELDS}


@pytest.mark.parametrize("name", ["neighbours", "foreign and stale"])
def test_both_flags_equal_the_lifted_pinned_target_then_the_round(ctx, name):
    c, target = PL.case(name)
    exp = sharding.assign_cooperative_numpy(*c.args(), assign=lambda *a: target[:3])
    got = call(ctx, c)
    for k, e in zip(FIELDS, exp):
        np.testing.assert_array_equal(got[k], e, err_msg="%s %s" % (k, name))


def test_without_the_large_bit_the_call_is_eshape_and_writes_nothing(ctx):
    c, _ = PL.case("neighbours")
    with pytest.raises(N.LagAssignError) as e:
        call(ctx, c, pinned_large=False)
    assert e.value.code == N.LA_ESHAPE
    assert ctx.last_launches() == 0


def test_over_the_consumer_limit_both_flags_are_eshape_at_the_call(ctx):
    c = PL.OVER_CONSUMERS()
    with pytest.raises(N.LagAssignError) as e:
        call(ctx, c)
    assert e.value.code == N.LA_ESHAPE
    assert ctx.last_launches() == 0


def test_the_large_bit_alone_and_on_other_entries_is_einval(ctx):
    c, _ = PL.case("one past")
    with pytest.raises(N.LagAssignError) as e:
        call(ctx, c, pinned=False)
    assert e.value.code == N.LA_EINVAL
    r = N.CoopRoundArgs()
    r.flags = N.LA_COOP_PINNED_LARGE
    with pytest.raises(N.LagAssignError) as e:
        ctx.cooperative_round_device(r, 0)
    assert e.value.code == N.LA_EINVAL
    s = N.CoopStickyArgs()
    s.flags = N.LA_COOP_PINNED_LARGE
    with pytest.raises(N.LagAssignError) as e:
        ctx.cooperative_round_sticky_device(N.DeviceBatch(), s, 0)
    assert e.value.code == N.LA_EINVAL
    a = N.AssignStickyArgs()
    a.struct_size = ctypes.sizeof(N.AssignStickyArgs)
    a.coop.flags = N.LA_COOP_PINNED | N.LA_COOP_PINNED_LARGE
    assert N.load().la_assign_batch_cooperative_sticky(ctx._h, ctypes.byref(a)) == N.LA_EINVAL


# ---- the host mirror: lag.assignor.cooperative.followup.large ---------------------------------------------------------------------
def mirror_rounds(conf):
    """Scenario(7, 1, 4097, 3) through the host mirror: a settled group, one rebalance, one follow-up -> last_cooperative_round()
    of the two calls after the settling one."""
    from kafka_lag_based_assignor_amd.assignor import LagBasedPartitionAssignor
    s = Scenario(7, 1, 4097, 3)
    members = ["m%d" % r for r in range(s.m)]
    metadata = {"topic-0": list(range(s.p))}
    subs = {m: ["topic-0"] for m in members}
    a = LagBasedPartitionAssignor()
    a.configure(dict({"group.id": "g", "auto.offset.reset": "earliest"}, **conf))
    lags = lambda: {("topic-0", p): int(s.lag[p]) for p in range(s.p)}
    owned = a.assign_cooperative(metadata, subs, {}, Offsets(lags()))
    assert not a.last_cooperative_round()["followup"]
    rounds = []
    for _ in range(2):
        s.grow()
        got = a.assign_cooperative(metadata, subs, owned, Offsets(lags()))
        c = a.last_cooperative_round()
        if c["pinned"]:                                              # a pinned follow-up takes nothing away
            assert all(set(map(tuple, owned[m])) <= set(map(tuple, got[m])) for m in members)
        rounds.append(c)
        owned = got
    return rounds


def test_the_mirror_with_both_keys_settles_a_topic_of_4097_partitions():
    first, second = mirror_rounds({"lag.assignor.cooperative.followup": "pinned", "lag.assignor.cooperative.followup.large": "true"})
    assert not first["pinned"] and first["withheld"] > 0 and first["followup"]
    assert second["pinned"] and (second["withheld"], second["dropped"], second["followup"]) == (0, 0, False)
    assert second["pinned_free"] == first["withheld"] and second["pinned_foreign"] == 0


def test_the_mirror_with_followup_pinned_alone_falls_back_to_the_full_form():
    first, second = mirror_rounds({"lag.assignor.cooperative.followup": "pinned"})
    assert not first["pinned"] and not second["pinned"]
    assert second["withheld"] > 0 and second["followup"]
