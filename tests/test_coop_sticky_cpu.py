"""sharding.cooperative_round_sticky_numpy -- the yardstick tests/test_coop_sticky_gpu.py holds la_cooperative_round_sticky_device
to -- against the dictionary model of coop_sticky_cases.py at the cases the GPU tests run; that the case table reaches every edge
it names; the consequences the header states; the struct, the limits and the symbol against the header and the C compiler.
No GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding

import coop_cases as C
import coop_sticky_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
@pytest.mark.parametrize("name", K.NAMES)
def test_the_yardstick_is_the_dictionary_model(name):
    k = K.case(name)
    K.same(k.expect(), K.dict_model(k), name)


def test_the_composition_is_the_three_functions_and_nothing_else():
    k = K.case("mixed lags")
    c = k.coop
    prev = sharding.cooperative_adjust_numpy(c.part_off, c.pid, c.rank, c.m, c.owned_off, c.owned_topic, c.owned_pid)[0]
    sticky = sharding.sticky_ties_numpy(c.part_off, k.partition_id, k.lag, c.pid, c.rank, prev, max_partitions=k.cap, strict=False)
    third = sharding.cooperative_round_numpy(c.part_off, sticky[0], c.rank, c.m, c.owned_off, c.owned_topic, c.owned_pid)
    K.same(k.expect(), sticky + third, "by hand")
    assert (sticky[0] != c.pid).any() and sticky[3][1] > sticky[3][0]


def topic_ranges(k):
    po = k.coop.part_off
    return [(int(po[t]), int(po[t + 1])) for t in range(k.coop.t)]


def lag_at_positions(k):
    out = np.zeros(k.coop.n, np.int64)
    for a, z in topic_ranges(k):
        by_id = dict(zip(k.partition_id[a:z].tolist(), k.lag[a:z].tolist()))
        out[a:z] = [by_id[int(i)] for i in k.coop.pid[a:z]]
    return out


# ---- the table reaches every edge it names -------------------------------------------------------------------------------------------
def test_the_empty_cases_are_empty():
    assert K.case("no topics").coop.t == 0 and K.case("no topics").coop.n == 0
    k = K.case("no entries")
    assert k.coop.t > 0 and k.coop.n == 0 and k.coop.n_owned > 0
    k = K.case("nothing owned")
    assert k.coop.n_owned == 0 and k.coop.n > 0
    np.testing.assert_array_equal(k.expect()[0], k.coop.pid)         # sticky equals the target
    k = K.case("one partition")
    assert k.coop.t == 1 and k.coop.n == 1


def test_adjacent_topics_of_equal_lag_break_the_run_at_the_boundary():
    k = K.case("adjacent topics, all lags 0")
    exp = k.expect()
    lag = lag_at_positions(k)
    assert (lag == 0).all() and k.coop.t == 2
    a = int(k.coop.part_off[1])
    assert k.coop.rank[a - 1] != k.coop.rank[a]                      # different owners either side of the boundary
    assert exp[0].tolist() == [12, 13, 10, 11, 14, 15, 14, 15, 12, 13, 10, 11]
    for lo, hi in topic_ranges(k):
        assert sorted(exp[0][lo:hi].tolist()) == sorted(k.coop.pid[lo:hi].tolist())      # nothing crossed over
        assert (exp[0][lo:hi] != k.coop.pid[lo:hi]).any()                                # and each topic was re-matched
    assert exp[3].tolist() == [0, 8, 2, 0] and exp[4 + 7][2] == 4 and k.plain_round()[7][2] == 12
    # one run over both topics would hand member 0's surplus of topic 0 to its places in topic 1: the ids are the same on purpose
    assert set(k.coop.pid[:a].tolist()) == set(k.coop.pid[a:].tolist())


def test_the_equal_lag_carries_across_topics_of_63_64_and_65():
    k = K.case("equal lag across topics of 63, 64, 65")
    assert np.diff(k.coop.part_off).tolist() == [63, 64, 65] and np.unique(lag_at_positions(k)).size == 1
    exp = k.expect()
    for lo, hi in topic_ranges(k):
        assert sorted(exp[0][lo:hi].tolist()) == sorted(k.coop.pid[lo:hi].tolist())
    assert exp[3][2] >= 2, "topics were re-matched"


def test_a_run_starts_at_a_topics_last_position():
    k = K.case("run starts at a topic's last position")
    lag = lag_at_positions(k)
    a = int(k.coop.part_off[1])
    assert lag[a - 1] != lag[a - 2] and lag[a - 1] == lag[a]         # a run of one that ends with its topic, the value goes on
    exp = k.expect()
    assert exp[0][a - 1] == k.coop.pid[a - 1] and (exp[0][a:] != k.coop.pid[a:]).any()


def test_a_topic_without_consumers_lies_between_two_with():
    k = K.case("topic without consumers between two")
    (a0, z0), (a1, z1), (a2, z2) = topic_ranges(k)
    assert (k.coop.rank[a1:z1] == -1).all() and (k.coop.rank[a0:z0] >= 0).all() and (k.coop.rank[a2:z2] >= 0).all()
    exp = k.expect()
    np.testing.assert_array_equal(exp[0][a1:z1], k.coop.pid[a1:z1])  # nobody to match: the order stays
    assert exp[1][1] == 0 and exp[4 + 7][3] > 0                      # and what was owned there is dropped


def test_a_previous_owner_that_owns_nothing_in_the_run_matches_nobody():
    k = K.case("previous owner owns nothing in the run")
    exp = k.expect()
    prev_target = C.dict_model(k.coop)[0]
    assert (prev_target[:6] == 2).sum() == 2 and not (k.coop.rank[:6] == 2).any()
    assert (exp[4][:6] == 2).sum() == 2                              # they travel inside the run, still owned by member 2 before
    assert exp[3].tolist()[:2] == [0, 3], "the three partitions whose owner has a place in the run are kept"


def test_stale_unmapped_head_and_tail_claims_are_there():
    c = K.case("stale, unmapped, head and tail claims").coop
    assert c.owned_off[0] == 2 and c.n_owned - c.owned_off[-1] == 2
    assert (c.owned_topic[c.owned_off[0]:c.owned_off[-1]] == -1).sum() == 3
    assert K.case("stale, unmapped, head and tail claims").expect()[4 + 7][4] >= 13


def test_the_lags_are_negative_and_extreme_and_the_offsets_have_no_committed():
    k = K.case("negative and extreme lags")
    assert {K.I64.min, K.I64.min + 1, K.I64.max, K.I64.max - 1, -1} <= set(k.lag.tolist())
    assert k.expect()[3][1] > k.expect()[3][0]
    for name, latest in (("offsets, latest", True), ("offsets, earliest", False)):
        k = K.case(name)
        begin, end, committed = k.offsets
        assert (committed < 0).any() and k.latest == latest
        from oracle import oracle
        np.testing.assert_array_equal(oracle.compute_lags(begin, end, committed, latest), k.lag)
        assert np.unique(k.lag).size < 8


@pytest.mark.parametrize("which", K.LIMITS)
def test_the_limit_cases_sit_at_and_one_over_each_limit_alone(which):
    at, over = K.case("at the limit of " + which).coop, K.case("one over the limit of " + which).coop
    size = lambda c: {"N": c.n, "n_owned": c.n_owned, "M": c.m, "T": c.t}
    limit = {"N": K.LE, "n_owned": K.LO, "M": K.LM, "T": K.LT}
    assert size(at)[which] == limit[which] and size(over)[which] == limit[which] + 1
    assert K.case("at the limit of " + which).small and not K.case("one over the limit of " + which).small
    for other in K.LIMITS:
        if other != which:
            assert size(over)[other] <= limit[other], other


def test_the_large_topic_and_the_topic_over_the_hint():
    k = K.case("topic of 4097")
    assert np.diff(k.coop.part_off).max() == K.TOPIC_LIMIT + 1 and not k.small and k.cap == K.TOPIC_LIMIT
    exp = k.expect()
    a, z = topic_ranges(k)[1]
    np.testing.assert_array_equal(exp[0][a:z], k.coop.pid[a:z])
    assert exp[3][3] == 1
    k = K.case("topic over the hint")
    assert k.small and k.cap == 64 and (np.diff(k.coop.part_off) > 64).sum() == 1
    assert k.expect()[3][3] == 1 and k.expect()[3][2] == 2


def test_the_ids_are_shuffled_descending_and_hostile():
    c = K.case("ids descending").coop
    assert all((np.diff(c.pid[a:z]) < 0).all() for a, z in topic_ranges(K.case("ids descending")))
    assert {K.I32.min, K.I32.max, -1, 0} <= set(K.case("ids hostile").coop.pid[:12].tolist())
    c = K.case("ids shuffled").coop
    assert not all((np.diff(c.pid[a:z]) > 0).all() for a, z in topic_ranges(K.case("ids shuffled")) if z - a > 2)


# ---- consequences ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.CLEAN)
def test_sticky_withholds_no_more_than_the_plain_round_and_keeps_no_less(name):
    k = K.case(name)
    exp, plain = k.expect(), k.plain_round()
    assert exp[4 + 7][2] <= plain[7][2], "withheld"
    assert exp[3][1] >= exp[3][0] and (exp[2] >= 0).all()
    assert exp[4 + 7][0] == exp[3][1], "kept of the round on the sticky order is kept after"
    assert plain[7][0] == exp[3][0], "kept of the round on the target is kept before"


@pytest.mark.parametrize("name", ("mixed lags", "stale, unmapped, head and tail claims", "ids hostile", "adjacent topics, all lags 0"))
def test_the_lists_fed_back_with_the_same_lags_withhold_nothing(name):
    k = K.case(name)
    c = k.coop
    first = k.expect()
    member_off, topic, pid = first[-3:]
    # members that obeyed round n and were then handed what was withheld or fresh: round n + 1 from the TARGET's owners
    settled = sharding.group_by_member_numpy(c.part_off, first[0], c.rank, c.m)
    again = sharding.cooperative_round_sticky_numpy(c.part_off, k.partition_id, k.lag, c.pid, c.rank, c.m, *settled, max_partitions=k.cap)
    assert again[4 + 7][2] == 0 and again[4 + 7][5] == 0, "nothing withheld, no follow-up"
    # and the lists of round n as they lie are valid owned arrays of round n + 1: nothing they hold is withheld again
    nxt = sharding.cooperative_round_sticky_numpy(c.part_off, k.partition_id, k.lag, c.pid, c.rank, c.m, member_off, topic, pid,
                                                  max_partitions=k.cap)
    assert nxt[4 + 7][2] == 0 and nxt[4 + 7][5] == 0


# ---- header, binding, library ---------------------------------------------------------------------------------------------------------
def test_coop_sticky_args_struct_is_the_c_compilers():
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    fields = [name for name, _ in N.CoopStickyArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lagassign.h"\nint main(void){printf("%zu", sizeof(la_coop_sticky_args));' + \
          "".join('printf(" %%zu", offsetof(la_coop_sticky_args, %s));' % f for f in fields) + \
          'printf(" %d %d %d %d", LA_COOP_STICKY_ENTRIES, LA_COOP_STICKY_OWNED, LA_COOP_STICKY_MEMBERS, LA_COOP_STICKY_TOPICS);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [ctypes.sizeof(N.CoopStickyArgs)] + [getattr(N.CoopStickyArgs, f).offset for f in fields] + \
        [N.COOP_STICKY_ENTRIES, N.COOP_STICKY_OWNED, N.COOP_STICKY_MEMBERS, N.COOP_STICKY_TOPICS]
    assert N.CoopStickyArgs.round.size == ctypes.sizeof(N.CoopRoundArgs)


def test_assign_sticky_args_struct_is_the_c_compilers():
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    fields = [name for name, _ in N.AssignStickyArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lagassign.h"\nint main(void){printf("%zu", sizeof(la_assign_sticky_args));' + \
          "".join('printf(" %%zu", offsetof(la_assign_sticky_args, %s));' % f for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [ctypes.sizeof(N.AssignStickyArgs)] + [getattr(N.AssignStickyArgs, f).offset for f in fields]
    assert N.AssignStickyArgs.coop.size == ctypes.sizeof(N.AssignCoopArgs)


def test_the_host_restatement_is_the_assign_restatement_and_the_sticky_round():
    h = K.host_case("tiny")
    from oracle import oracle
    for mode in K.HOST_MODES:
        exp = h.expect(mode)
        target = oracle.assign_flat(h.part_off, h.pid, h.lag_of(mode), h.cons_off, h.cons_rank)
        for a, b in zip(exp[:3], target):
            np.testing.assert_array_equal(a, b)
        rest = sharding.cooperative_round_sticky_numpy(h.part_off, h.pid, h.lag_of(mode), target[0], target[1], h.m, *h.owned)
        K.same(exp[3:], rest, mode)
    big = K.host_case("at the limit")
    assert big.n == K.LE and K.host_case("one over the limit").n == K.LE + 1 and (big.committed < 0).any()
    exp = big.expect("lag")
    plain = sharding.cooperative_round_numpy(big.part_off, exp[0], exp[1], big.m, *big.owned)
    assert exp[3 + 4 + 7][2] < plain[7][2], "the caught-up group withholds less with sticky ties"


def test_the_host_mirrors_config_key_parses_and_defaults_to_off():
    from kafka_lag_based_assignor_amd.assignor import LagBasedPartitionAssignor
    a = LagBasedPartitionAssignor()
    assert a.sticky_ties() is False
    a.configure({"group.id": "g"})
    assert a.sticky_ties() is False
    for value, on in (("true", True), ("TRUE", True), (True, True), ("false", False), ("yes", False), ("", False)):
        a.configure({"group.id": "g", "lag.assignor.sticky.ties": value})
        assert a.sticky_ties() is on, value
    a.configure({"group.id": "g"})
    assert a.sticky_ties() is False, "a key that is gone is off again"
    c = LagBasedPartitionAssignor.last_cooperative_round()
    assert {"sticky_kept_before", "sticky_kept_after", "sticky_topics_passed_through"} <= set(c)
    src = open(os.path.join(ROOT, "kafka_lag_based_assignor_amd", "csrc", "host", "lag_based_partition_assignor.cpp")).read()
    assert "lag.assignor.sticky.ties" in src and "la_assign_batch_cooperative_sticky" in src


def test_the_four_limits_are_those_of_the_source_and_within_what_the_issue_allows():
    csrc = os.path.join(ROOT, "kafka_lag_based_assignor_amd", "csrc")
    coop, group = open(os.path.join(csrc, "la_coop.h")).read(), open(os.path.join(csrc, "la_group_small.h")).read()
    consts = {"kTailGroupM": int(re.search(r"constexpr int kTailGroupM = (\d+);", group).group(1))}

    def limit(name):
        m = re.search(r"constexpr int %s = ([^;]+);" % name, coop)
        assert m, name
        consts[name] = int(eval(m.group(1), {"__builtins__": {}}, consts))
        return consts[name]

    for small in ("kCoopSmallEntries", "kCoopSmallOwned", "kCoopSmallMembers", "kCoopSmallTopics"):
        limit(small)
    assert limit("kCoopStickyEntries") == N.COOP_STICKY_ENTRIES >= 1024
    assert limit("kCoopStickyOwned") == N.COOP_STICKY_OWNED >= 1024
    assert limit("kCoopStickyMembers") == N.COOP_STICKY_MEMBERS >= 1022
    assert limit("kCoopStickyTopics") == N.COOP_STICKY_TOPICS


def test_the_symbol_is_declared_bound_and_exported():
    from kafka_lag_based_assignor_amd import build
    header = open(os.path.join(ROOT, "include", "lagassign.h")).read()
    lib = N.load()                                                   # loads without a GPU
    name = "la_cooperative_round_sticky_device"
    assert re.search(r"\bint %s\(" % name, header) and name in N.EXPORTED_SYMBOLS and hasattr(lib, name)
    host = "la_assign_batch_cooperative_sticky"
    assert re.search(r"\bint %s\(" % host, header) and host in N.EXPORTED_SYMBOLS and hasattr(lib, host)
    assert getattr(lib, host).argtypes[1] == ctypes.POINTER(N.AssignStickyArgs)
    assert callable(N.Context.assign_batch_cooperative_sticky) and callable(sharding.assign_cooperative_sticky_numpy)
    assert getattr(lib, name).argtypes[1:3] == [ctypes.POINTER(N.DeviceBatch), ctypes.POINTER(N.CoopStickyArgs)]
    assert "#define LA_VERSION 500" in header and lib.la_version() == 500, "added without an ABI bump"
    assert callable(N.Context.cooperative_round_sticky_device) and "la_coop_sticky_small.hip" in build.SOURCES
