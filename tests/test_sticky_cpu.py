"""sharding.sticky_ties_numpy -- the host restatement of la_sticky_ties_device and the yardstick of test_sticky_gpu.py -- against
an independent dict model of the five rules, against brute force over every lag-preserving permutation of short runs, and
against the consequences the header states; then the C ABI's declaration, binding and build list.  No GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import build, sharding

import sticky_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = np.iinfo(np.int64)


def _check(w, res, prev, what=""):
    """sticky_ties_numpy against the model and every stated consequence; returns its four results."""
    sticky, kept, saved, summary = S.expect(w, res, prev)
    m_sticky, m_before, m_after = S.model(w, res, prev)
    np.testing.assert_array_equal(sticky, m_sticky, err_msg="sticky order %s" % what)
    np.testing.assert_array_equal(kept, m_after, err_msg="kept after %s" % what)
    np.testing.assert_array_equal(saved, m_after - m_before, err_msg="saved %s" % what)
    assert (saved >= 0).all(), what
    np.testing.assert_array_equal(kept, S.min_sum(w, res, prev), err_msg="kept after is the min-sum %s" % what)
    # every run is a permutation of itself: the lag at every position stays, so ranks and totals stay valid
    np.testing.assert_array_equal(S.lag_at_positions(w, (sticky,)), S.lag_at_positions(w, res), err_msg="lag per position %s" % what)
    lag = S.lag_at_positions(w, res)
    for t in range(w.n_topics):
        a, z = int(w.part_off[t]), int(w.part_off[t + 1])
        assert sorted(sticky[a:z]) == sorted(res[0][a:z]), (what, t)
        single = np.ones(z - a, bool)                               # positions that are a run of their own
        if z - a > 1:
            same = lag[a + 1:z] == lag[a:z - 1]
            single[1:] &= ~same
            single[:-1] &= ~same
        np.testing.assert_array_equal(sticky[a:z][single], res[0][a:z][single], err_msg="%s topic %d" % (what, t))
    changed = sum(1 for t in range(w.n_topics) if (sticky[w.part_off[t]:w.part_off[t + 1]] != res[0][w.part_off[t]:w.part_off[t + 1]]).any())
    assert list(summary) == [int(m_before.sum()), int(m_after.sum()), changed, 0], what
    # the sticky order verifies as 0 or exactly ORDER
    verdict, _ = sharding.verify_assignment_numpy(w.part_off, w.partition_id, w.cons_off, w.cons_rank, sticky, res[1], res[2], lag=w.lag)
    assert set(verdict.tolist()) <= {0, sharding.VERDICT_ORDER}, (what, verdict)
    return sticky, kept, saved, summary


@pytest.mark.parametrize("p", [p for p in S.SHAPE_P if p <= 257])
def test_rules_against_the_model_at_the_gpu_shapes(p):
    w = S.shape_case(p)
    res = S.target(w)
    for kind in ("mixed", "shifted", "own", "none"):
        _check(w, res, S.draw_prev_owner(w, res, 3, kind), "P = %d, %s" % (p, kind))


def test_runs_across_the_edges_and_runs_of_two():
    w = S.straddle_case()
    res = S.target(w)
    lag = S.lag_at_positions(w, res)
    assert lag[63] == lag[64] and lag[255] == lag[256] and lag[59] != lag[60]
    for seed in (1, 2):
        sticky = _check(w, res, S.draw_prev_owner(w, res, seed), "straddle")[0]
    assert (sticky != res[0]).any()
    _check(w, res, S.draw_prev_owner(w, res, 1, "shifted"), "straddle, shifted")


def test_a_member_with_more_and_with_fewer_previous_partitions_than_places():
    w, res, prev = S.uneven_case()
    sticky, kept, saved, summary = _check(w, res, prev, "uneven")
    a = int(w.cons_rank[0])
    # first run: |S_a| = 4 < |W_a| = 7 -- the FIRST four of a's previous partitions land on a's places, in order
    s_a = [i for i in range(12) if res[1][i] == a]
    w_a = [i for i in range(12) if prev[i] == a]
    assert [int(sticky[d]) for d in s_a] == [int(res[0][s]) for s in w_a[:4]]
    # second run: |S_a| = 4 > |W_a| = 1 -- a's first place takes it
    s_a2 = [i for i in range(12, 24) if res[1][i] == a]
    assert int(sticky[s_a2[0]]) == int(res[0][12])
    assert int(kept[0]) == int(S.min_sum(w, res, prev)[0]) and int(summary[2]) == 1


def test_brute_force_kept_after_is_the_maximum_over_lag_preserving_permutations():
    """Runs of up to 6 partitions: no permutation inside the runs keeps more partitions with their owner."""
    rng = np.random.default_rng(21)
    checked = 0
    for trial in range(120):
        lengths = [int(x) for x in rng.integers(1, 7, int(rng.integers(1, 4)))]
        c = int(rng.integers(1, 5))
        w = S.workload([(S.lags_of_runs(lengths, rng), c)], 100 + trial)
        res = S.target(w)
        members = list(w.cons_rank) + [-1, int(w.cons_rank.max()) + 3]
        prev = np.array([members[int(x)] for x in rng.integers(0, len(members), w.n_partitions)], np.int32)
        kept = S.expect(w, res, prev)[1]
        best, at = 0, 0
        for n in lengths:                                           # (the target lists the runs in this order)
            own, q = res[1][at:at + n], prev[at:at + n]
            best += max(sum(1 for d in range(n) if q[perm[d]] >= 0 and q[perm[d]] == own[d]) for perm in itertools.permutations(range(n)))
            at += n
        assert int(kept[0]) == best, (trial, lengths, c)
        checked += 1
    assert checked == 120


def test_distinct_lags_owners_of_minus_one_and_no_previous_owner_give_identity():
    rng = np.random.default_rng(5)
    w = S.workload([(rng.permutation(200).astype(np.int64), 7), (np.zeros(100, np.int64), 0), (S.mixed_lags(150, rng), 4)], 5)
    res = S.target(w)
    assert (res[1][200:300] == -1).all()
    prev = S.draw_prev_owner(w, res, 6)
    sticky, kept, saved, summary = _check(w, res, prev, "identity")
    np.testing.assert_array_equal(sticky[:300], res[0][:300])       # all lags distinct; a topic without consumers
    assert saved[0] == 0 and saved[1] == 0 and kept[1] == 0
    sticky, kept, saved, summary = _check(w, res, S.draw_prev_owner(w, res, 6, "none"), "nobody owned anything")
    np.testing.assert_array_equal(sticky, res[0])
    assert list(summary) == [0, 0, 0, 0]
    sticky, kept, saved, summary = _check(w, res, S.draw_prev_owner(w, res, 6, "own"), "everything kept already")
    np.testing.assert_array_equal(sticky, res[0])
    assert summary[0] == summary[1] == int((res[1] >= 0).sum())


def test_previous_owners_that_match_nothing():
    """-1, -2, INT32_MAX and a rank that subscribes elsewhere only: no match, no index, the partitions fill the places left."""
    w = S.workload([(np.zeros(40, np.int64), 4), (np.zeros(8, np.int64), 2)], 8)
    res = S.target(w)
    elsewhere = int(np.setdiff1d(w.cons_rank[4:], w.cons_rank[:4])[0]) if np.setdiff1d(w.cons_rank[4:], w.cons_rank[:4]).size else 1 << 20
    for q in (-1, -2, S.I32_MAX, elsewhere):
        prev = np.full(w.n_partitions, q, np.int32)
        prev[40:] = -1
        sticky, kept, saved, summary = _check(w, res, prev, "q = %d" % q)
        np.testing.assert_array_equal(sticky, res[0])
        assert list(summary) == [0, 0, 0, 0]
    prev = np.full(w.n_partitions, -2, np.int32)
    prev[7] = int(res[1][0])                                         # one real previous owner among them
    sticky = _check(w, res, prev, "one real owner")[0]
    assert sticky[0] == res[0][7] and sorted(sticky[:40]) == sorted(res[0][:40])


def test_negative_lags_and_ties_at_the_ends_of_int64():
    lag = np.array([I64.max] * 5 + [I64.min] * 6 + [-3] * 4 + [-1, 0, 7, I64.max - 1, I64.min + 1], np.int64)
    w = S.workload([(np.random.default_rng(2).permutation(lag), 3)], 9)
    res = S.target(w)
    at = S.lag_at_positions(w, res)
    assert list(at[:5]) == [I64.max] * 5 and list(at[-6:]) == [I64.min] * 6
    sticky = _check(w, res, S.draw_prev_owner(w, res, 4, "shifted"), "int64 ends")[0]
    assert (sticky != res[0]).any()


def test_caught_up_group_keeps_at_least_what_it_kept():
    w, res, prev, _ = S.caught_up(20, 256, 32, 0.01, 31)
    sticky, kept, saved, summary = _check(w, res, prev, "caught up, 20 x 256 x 32")
    assert summary[1] >= summary[0]


def test_a_topic_over_the_limit_is_passed_through_and_the_two_einval_conditions_raise():
    rng = np.random.default_rng(3)
    w = S.workload([(S.mixed_lags(50, rng), 3), (np.zeros(S.LIMIT + 1, np.int64), 2), (np.zeros(30, np.int64), 3)], 10)
    res = S.target(w)
    prev = S.draw_prev_owner(w, res, 2, "shifted")
    sticky, kept, saved, summary = S.expect(w, res, prev)
    a, z = int(w.part_off[1]), int(w.part_off[2])
    np.testing.assert_array_equal(sticky[a:z], res[0][a:z])
    assert saved[1] == 0 and kept[1] == int(((prev[a:z] >= 0) & (prev[a:z] == res[1][a:z])).sum()) and summary[3] == 1
    assert (sticky[z:] != res[0][z:]).any() and saved[2] > 0
    # the same topics at a limit that passes the first one through as well
    assert S.expect(w, res, prev, max_partitions=49)[3][3] == 2
    small = S.workload([(np.zeros(6, np.int64), 2), (np.zeros(5, np.int64), 2)], 11)
    s_res, s_prev = S.target(small), np.zeros(11, np.int32)
    dup = small.partition_id.copy()
    dup[1] = dup[0]
    with pytest.raises(ValueError, match="twice in the input"):
        sharding.sticky_ties_numpy(small.part_off, dup, small.lag, s_res[0], s_res[1], s_prev)
    for bad in (99, int(s_res[0][1])):                               # no input id of the topic; an input id twice
        out = s_res[0].copy()
        out[0] = bad
        with pytest.raises(ValueError, match="no input id"):
            sharding.sticky_ties_numpy(small.part_off, small.partition_id, small.lag, out, s_res[1], s_prev)
        got = sharding.sticky_ties_numpy(small.part_off, small.partition_id, small.lag, out, s_res[1], s_prev, strict=False)
        np.testing.assert_array_equal(got[0][:6], out[:6])          # passed through as it came, the other topic re-matched
        assert got[3][3] == 1
    with pytest.raises(ValueError, match="offsets"):
        sharding.sticky_ties_numpy(np.array([0, 12], np.int64), small.partition_id, small.lag, s_res[0], s_res[1], s_prev)


@pytest.mark.parametrize("threads", [64, 256])
def test_the_kernels_keys_bisections_and_scans_give_the_rules(threads):
    """sticky_cases.kernel_model walks a topic as the kernel does; it must land where the rules do."""
    for w in (S.straddle_case(), S.shape_case(65), S.shape_case(257)):
        res = S.target(w)
        lag = S.lag_at_positions(w, res)
        for kind in ("mixed", "shifted"):
            prev = S.draw_prev_owner(w, res, 9, kind)
            sticky, kept, _, _ = S.expect(w, res, prev)
            for t in range(w.n_topics):
                a, z = int(w.part_off[t]), int(w.part_off[t + 1])
                got, got_kept = S.kernel_model([int(x) for x in lag[a:z]], [int(x) for x in res[1][a:z]], [int(x) for x in prev[a:z]],
                                               [int(x) for x in res[0][a:z]], threads)
                assert got == [int(x) for x in sticky[a:z]] and got_kept == int(kept[t]), (kind, t)


def test_empty_batches():
    e32, e64 = np.empty(0, np.int32), np.empty(0, np.int64)
    sticky, kept, saved, summary = sharding.sticky_ties_numpy(np.zeros(1, np.int64), e32, e64, e32, e32, e32)
    assert sticky.size == kept.size == saved.size == 0 and list(summary) == [0, 0, 0, 0]
    sticky, kept, saved, summary = sharding.sticky_ties_numpy(np.zeros(4, np.int64), e32, e64, e32, e32, e32)
    assert sticky.size == 0 and list(kept) == [0, 0, 0] and list(saved) == [0, 0, 0] and list(summary) == [0, 0, 0, 0]


# ---- the C ABI: declared, exported, bound, built -------------------------------------------------------------------------------
def test_the_call_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "lagassign.h")).read()
    lib = N.load()
    name = "la_sticky_ties_device"
    assert re.search(r"\bint %s\(" % name, header) and name in N.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "la_sticky.hip" in build.SOURCES
    assert re.search(r"later, WITHOUT a bump:.*?la_sticky_ties_device", header, re.S)
    assert header.count("LA_VERDICT_ORDER") >= 3                    # said at the verify call and at this one
    # the binding's struct is the header's: field order and types
    body = header[header.index("typedef struct la_sticky_args {"):header.index("} la_sticky_args;")]
    fields = re.findall(r"^\s*(?:const\s+)?(int32_t|int64_t)\s*(\*?)\s*(\w+);", body, re.M)
    declared = [(n, "p" if star else t) for t, star, n in fields]
    bound = [(n, "p" if t is ctypes.c_void_p else {ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t"}[t]) for n, t in N.StickyArgs._fields_]
    assert declared == bound and ctypes.sizeof(N.StickyArgs) == 8 + 5 * 8
    assert sharding.STICKY_MAX_PARTITIONS == N.VERIFY_MAX_PARTITIONS
    assert callable(N.Context.sticky_ties_device)


def test_a_null_context_is_einval():
    lib = N.load()
    assert lib.la_sticky_ties_device(None, None, None, None) == N.LA_EINVAL
