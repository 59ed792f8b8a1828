"""Sticky ties for topics of any size, on the host: the yardstick of tests/test_sticky_large_gpu.py --
sharding.sticky_ties_numpy without a limit -- against the independent model of sticky_cases at every case of
sticky_large_cases.py, that the case table reaches the edges it names, and the new names of the ABI."""
import os
import re

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import build, sharding

import sticky_cases as S
import sticky_large_cases as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", SL.NAMES)
def test_the_yardstick_without_a_limit_is_the_model(name):
    w, res = SL.case(name)
    kinds = SL.KINDS if name.startswith("shape") else ("mixed", "skewed") if name == "straddle" else ("mixed",)
    for kind in kinds:
        prev = SL.prev_of(name, kind)
        sticky, kept, saved, summary = SL.expected(name, kind)
        m_sticky, m_before, m_after = S.model(w, res, prev)
        np.testing.assert_array_equal(sticky, m_sticky, err_msg="%s, %s" % (name, kind))
        np.testing.assert_array_equal(kept, m_after)
        np.testing.assert_array_equal(saved, m_after - m_before)
        assert list(summary) == [m_before.sum(), m_after.sum(), sum((sticky[w.part_off[t]:w.part_off[t + 1]] !=
                                 res[0][w.part_off[t]:w.part_off[t + 1]]).any() for t in range(w.n_topics)), 0]
        np.testing.assert_array_equal(kept, S.min_sum(w, res, prev))


def test_the_default_limit_passes_the_large_topics_through():
    w, res = SL.case("mixed batch")
    prev = SL.prev_of("mixed batch")
    limited, free = S.expect(w, res, prev), SL.expected("mixed batch")
    big = SL.big_topics(w)
    assert big == [0, 4, 6] and limited[3][3] == len(big) and free[3][3] == 0
    for t in range(w.n_topics):
        a, z = int(w.part_off[t]), int(w.part_off[t + 1])
        if t in big:
            np.testing.assert_array_equal(limited[0][a:z], res[0][a:z])
            assert limited[2][t] == 0
        else:
            np.testing.assert_array_equal(limited[0][a:z], free[0][a:z])
            assert (limited[1][t], limited[2][t]) == (free[1][t], free[2][t])
    assert free[2][0] > 0 and free[2][4] > 0 and free[2][6] == 0      # (a topic without consumers keeps nothing)
    assert int(w.part_off[4] - w.part_off[3]) == SL.LIMIT


def test_the_cases_reach_the_edges_they_name():
    w, res = SL.case("straddle")
    runs = SL.groups_of(w, res, SL.prev_of("straddle", "skewed"))
    for edge in SL.EDGES:
        across = [r for r in runs if r[0] < edge < r[1]]
        assert len(across) == 1, "a run across position %d of the concatenated list" % edge
        groups = across[0][2]
        assert any(s and s[0] < edge <= s[-1] for s, _ in groups.values()), "a member's places on both sides of %d" % edge
        assert any(wl and wl[0] < edge <= wl[-1] for _, wl in groups.values())
    more_s = sum(1 for _, _, g in runs for s, wl in g.values() if len(s) > len(wl) > 0)
    more_w = sum(1 for _, _, g in runs for s, wl in g.values() if len(wl) > len(s) > 0)
    assert more_s > 0 and more_w > 0
    left_over = [sum(len(s) - min(len(s), len(wl)) for s, wl in g.values()) for _, _, g in runs]
    assert sum(1 for n in left_over if n >= 2) > 1, "leftovers in more than one run"
    # two neighbouring topics, all lag 0: one run each, not one over both
    w, res = SL.case("neighbours")
    runs = SL.groups_of(w, res, SL.prev_of("neighbours"))
    assert [(a, z) for a, z, _ in runs] == [(0, SL.LIMIT + 1), (SL.LIMIT + 1, 2 * SL.LIMIT + 3)]
    assert (S.lag_at_positions(w, res) == 0).all()
    # the shapes: one topic each, over the limit by one element of a 4 096 / 8 192 / 16 384 tile
    for p in SL.SHAPE_P:
        w, _ = SL.case("shape %d" % p)
        assert (w.n_topics, w.n_partitions) == (1, p) and p > SL.LIMIT
    w, res = SL.case("one run")
    assert len(SL.groups_of(w, res, SL.prev_of("one run"))) == 1 and w.n_partitions == 3 * SL.LIMIT + 1
    w, res = SL.case("no ties")
    assert len(SL.groups_of(w, res, SL.prev_of("no ties"))) == w.n_partitions
    np.testing.assert_array_equal(SL.expected("no ties")[0], res[0])
    assert SL.expected("no ties")[3][2] == 0
    w, res = SL.case("extremes")
    assert {SL.I64.min, SL.I64.max, -5} <= set(w.lag.tolist())
    assert SL.case("one large")[0].n_partitions == SL.case("three large")[0].n_partitions
    assert len(SL.big_topics(SL.case("three large")[0])) == 3 and SL.big_topics(SL.case("small only")[0]) == []
    prev = SL.prev_of("shape %d" % SL.SHAPE_P[0])
    assert {-1, -2, S.I32_MAX} <= set(prev.tolist())


def test_any_size_reaches_the_composed_yardsticks():
    import coop_sticky_cases as K
    k = K.drawn(61, [SL.LIMIT + 1, 40], 5, K.caught_up)
    c = k.coop
    args = (c.part_off, k.partition_id, k.lag, c.pid, c.rank, c.m, c.owned_off, c.owned_topic, c.owned_pid)
    limited = sharding.cooperative_round_sticky_numpy(*args)
    free = sharding.cooperative_round_sticky_numpy(*args, max_partitions=sharding.STICKY_ANY_SIZE)
    assert limited[3][3] == 1 and free[3][3] == 0 and free[3][1] >= limited[3][1]
    assert sharding.STICKY_ANY_SIZE == N.STICKY_GLOBAL_MAX_PARTITIONS > sharding.STICKY_MAX_PARTITIONS == 4096


def test_the_new_names_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "lagassign.h")).read()
    kernels = open(os.path.join(ROOT, "kafka_lag_based_assignor_amd", "csrc", "la_kernels.h")).read()
    lib = N.load()
    assert hasattr(lib, "la_sticky_ties_device") and "la_sticky_ties_device" in N.EXPORTED_SYMBOLS
    assert "la_sticky_large.hip" in build.SOURCES
    assert re.search(r"later, WITHOUT a bump:.*?LA_FLAG_STICKY_LARGE, LA_COOP_STICKY_LARGE", header, re.S)
    for define, value in (("LA_FLAG_STICKY_LARGE", N.LA_FLAG_STICKY_LARGE), ("LA_COOP_STICKY_LARGE", N.LA_COOP_STICKY_LARGE),
                          ("LA_STICKY_GLOBAL_LAUNCHES", N.STICKY_GLOBAL_LAUNCHES)):
        m = re.search(r"#define %s\s+(\d+)" % define, header)
        assert m and int(m.group(1)) == value, define
    assert N.LA_FLAG_STICKY_LARGE == 16384 and N.LA_COOP_STICKY_LARGE == 2
    m = re.search(r"kStickyOwnLaunches = (\d+);", kernels)
    assert m and N.STICKY_GLOBAL_LAUNCHES == int(m.group(1)) + 1 + 8 * 4
    # no flag of the batch shares the bit
    flags = {k: int(v) for k, v in re.findall(r"#define (LA_FLAG_[A-Z_]+)\s+(\d+)", header)}
    assert sum(1 for v in flags.values() if v == 16384) == 1


def test_a_null_context_is_einval():
    assert N.load().la_sticky_ties_device(None, None, None, None) == N.LA_EINVAL


def test_the_mirror_reads_the_large_key():
    from kafka_lag_based_assignor_amd.assignor import LagBasedPartitionAssignor
    for value, large in ((None, False), ("true", True), ("TRUE", True), ("yes", False), ("false", False)):
        a = LagBasedPartitionAssignor()
        conf = {"group.id": "g", "lag.assignor.sticky.ties": "true"}
        if value is not None:
            conf["lag.assignor.sticky.ties.large"] = value
        a.configure(conf)
        assert a.sticky_ties() and a.sticky_ties_large() is large, value
    a = LagBasedPartitionAssignor()
    a.configure({"group.id": "g", "lag.assignor.sticky.ties.large": "true"})
    assert not a.sticky_ties() and a.sticky_ties_large()           # read, and without effect: the other key is off
