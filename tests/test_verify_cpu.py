"""sharding.verify_assignment_numpy -- the yardstick of test_verify_gpu.py -- held to the oracle, without a GPU: all-zero verdicts on
the oracle's results at every shape the GPU file runs, and after every fault of the catalogue (verify_cases.CATALOGUE) a non-zero
verdict exactly for the topics whose result differs from the oracle's.  Plus the binding: prototypes, constants, argument errors."""
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding

import offset_cases
import verify_cases as V


def _certified(w, what, **kw):
    exp = V.oracle_result(w) if "end" not in kw else kw.pop("exp")
    verdict, summary = V.yardstick(w, exp, **kw)
    assert not verdict.any(), "%s: topics %s are not certified: %s" % (what, np.flatnonzero(verdict)[:8], verdict[verdict != 0][:8])
    np.testing.assert_array_equal(summary, [0, 0, -1, -1])


@pytest.mark.parametrize("p", V.SHAPE_P)
def test_oracle_results_are_certified_at_every_shape(p):
    _certified(V.batch(V.shapes_of(p), p), "P = %d" % p)


def test_oracle_results_are_certified_with_full_and_partial_last_rounds():
    _certified(V.batch(V.ROUND_SHAPES, 1), "round shapes")


@pytest.mark.parametrize("lags", ["equal", "zero", "wrap", "negative"])
@pytest.mark.parametrize("ids", ["shuffled", "full", "4096", "2^20"])
def test_oracle_results_are_certified_for_every_kind_of_value(lags, ids):
    _certified(V.batch([(256, 32), (1000, 7), (5, 9), (300, 0), (0, 4), (65, 64), (700, 300)], 2, lags=lags, ids=ids), "%s / %s" % (lags, ids))


def test_wrapping_totals_are_decided_by_the_signed_compare():
    w = V.batch([(1000, 7), (256, 32)], 3, lags="wrap")
    tot = V.oracle_result(w)[2]
    exact = sum(int(x) for x in w.lag[:1000])                        # topic 0 in unbounded integers
    assert exact != sum(int(x) for x in tot[:7]) and (exact - sum(int(x) for x in tot[:7])) % (1 << 64) == 0, "the totals of this batch wrap"
    _certified(w, "wrap")


@pytest.mark.parametrize("latest", [True, False])
@pytest.mark.parametrize("regime", offset_cases.REGIMES)
def test_lags_from_hostile_offsets(regime, latest):
    from oracle import oracle
    shapes = ((256, 32), (100, 16), (1000, 7), (5, 0), (0, 3))
    w = offset_cases.make_case(shapes, regime, "50%")
    lag = offset_cases.java_lags(w.begin, w.end, w.committed, latest)
    exp = oracle.assign_flat(w.part_off, w.partition_id, lag, w.cons_off, w.cons_rank)
    verdict, summary = V.yardstick(w, exp, begin=w.begin, end=w.end, committed=w.committed, reset_latest=latest)
    assert not verdict.any()
    if latest:                                                       # no begin array: only LATEST may leave it out
        verdict, _ = V.yardstick(w, exp, begin=None, end=w.end, committed=w.committed, reset_latest=True)
        assert not verdict.any()
    other = V.yardstick(w, exp, begin=w.begin, end=w.end, committed=w.committed, reset_latest=not latest)[0]
    assert other.any(), "the other reset mode gives other lags: the result is not its result"


@pytest.mark.parametrize("shape", V.CATALOGUE_SHAPES)
def test_every_fault_of_the_catalogue_is_found_in_its_topic_only(shape):
    w = V.catalogue_batch(shape)
    exp = V.oracle_result(w)
    cases = V.catalogue_cases(w, exp)
    if shape in ((256, 32), (1000, 7)):
        missing = set(V.CATALOGUE) - {c[0] for c in cases}
        if shape == (256, 32):                                       # eight full rounds
            missing -= {"partial last round: an unpicked consumer for the last picked"}
        assert not missing, "no place in %s for %s" % (shape, missing)
    for name, t, res in cases:
        assert V.differing_topics(w, res, exp) == [t], "%s: the mutation must change topic %d and no other" % (name, t)
        verdict, summary = V.yardstick(w, res)
        assert verdict[t] & V.CATALOGUE[name], "%s at %s: verdict %d lacks its class bit" % (name, shape, verdict[t])
        assert not verdict[t] & V.UNCHECKED
        assert list(np.flatnonzero(verdict)) == [t], "%s at %s: verdicts %s" % (name, shape, verdict)
        np.testing.assert_array_equal(summary, [1, 0, t, -1])


def test_the_catalogue_names_every_class_bit_and_every_entry_has_a_place():
    named = 0
    for bits in V.CATALOGUE.values():
        named |= bits
    assert named == V.IDS | V.ORDER | V.OWNER | V.GREEDY | V.TOTALS
    placed = set()
    for shape in V.CATALOGUE_SHAPES:
        w = V.catalogue_batch(shape)
        placed |= {c[0] for c in V.catalogue_cases(w, V.oracle_result(w))}
    assert placed == set(V.CATALOGUE)


def test_totals_are_optional():
    w = V.catalogue_batch((256, 32))
    exp = V.oracle_result(w)
    res = V.mutate("total + 1", w, exp, 1)
    assert V.yardstick(w, res)[0][1] == V.TOTALS
    verdict, _ = sharding.verify_assignment_numpy(w.part_off, w.partition_id, w.cons_off, w.cons_rank, res[0], res[1], None, lag=w.lag)
    assert not verdict.any()


def test_unverifiable_topics_read_unchecked_and_nothing_else():
    w = V.batch([(64, 8), (V.LIMIT + 1, 8), (30, 5), (64, V.LIMIT + 1), (20, 3)], 4)
    verdict, summary = V.yardstick(w, V.oracle_result(w))
    np.testing.assert_array_equal(verdict, [0, V.UNCHECKED, 0, V.UNCHECKED, 0])
    np.testing.assert_array_equal(summary, [0, 2, -1, 1])
    w = V.batch([(64, 8), (50, 8), (30, 5), (40, 6)], 5)
    exp = V.oracle_result(w)
    pid = w.partition_id.copy()
    pid[64 + 7] = pid[64 + 20]                                       # duplicate input ids in topic 1
    ranks = w.cons_rank.copy()
    a = int(w.cons_off[3])
    ranks[[a + 1, a + 2]] = ranks[[a + 2, a + 1]]                    # topic 3's ranks do not ascend
    verdict, summary = sharding.verify_assignment_numpy(w.part_off, pid, w.cons_off, ranks, exp[0], exp[1], exp[2], lag=w.lag)
    np.testing.assert_array_equal(verdict, [0, V.UNCHECKED, 0, V.UNCHECKED])
    np.testing.assert_array_equal(summary, [0, 2, -1, 1])
    ranks = w.cons_rank.copy()
    ranks[a + 1] = ranks[a]                                          # ... or repeat
    assert sharding.verify_assignment_numpy(w.part_off, w.partition_id, w.cons_off, ranks, exp[0], exp[1], exp[2], lag=w.lag)[0][3] == V.UNCHECKED


def test_summary_of_failed_and_unchecked_topics_together():
    w = V.batch([(64, 8), (50, 8), (V.LIMIT + 1, 2), (40, 6), (30, 5)], 6)
    exp = V.oracle_result(w)
    res = V.mutate("total + 1", w, exp, 3)
    res = V.mutate("foreign id", w, res, 4)
    verdict, summary = V.yardstick(w, res)
    np.testing.assert_array_equal(verdict != 0, [False, False, True, True, True])
    np.testing.assert_array_equal(summary, [2, 1, 3, 2])
    po = w.part_off.copy()
    po[2] = w.n_partitions + 1
    with pytest.raises(ValueError):
        sharding.verify_assignment_numpy(po, w.partition_id, w.cons_off, w.cons_rank, exp[0], exp[1], exp[2], lag=w.lag)


def test_empty_batches():
    e32, e64 = np.empty(0, np.int32), np.empty(0, np.int64)
    verdict, summary = sharding.verify_assignment_numpy(np.zeros(1, np.int64), e32, np.zeros(1, np.int64), e32, e32, e32, e64, lag=e64)
    assert verdict.size == 0
    np.testing.assert_array_equal(summary, [0, 0, -1, -1])
    w = V.batch([(0, 3), (0, 0), (0, 2)], 7)
    _certified(w, "N = 0")
    bad = (e32, e32, np.array([0, 0, 0, 1, 0], np.int64))            # a total without a partition behind it
    verdict, _ = V.yardstick(w, bad)
    np.testing.assert_array_equal(verdict, [0, 0, V.TOTALS])


# ---- the binding -------------------------------------------------------------------------------------------------------------
def test_constants_match_the_header():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lagassign.h")).read()
    for name in ("IDS", "ORDER", "OWNER", "GREEDY", "TOTALS", "UNCHECKED"):
        value = int(re.search(r"#define LA_VERDICT_%s\s+(\d+)" % name, header).group(1))
        assert getattr(N, "LA_VERDICT_" + name) == value == getattr(sharding, "VERDICT_" + name)
    assert int(re.search(r"#define LA_VERSION (\d+)", header).group(1)) == 500
    assert N.VERIFY_MAX_PARTITIONS == N.VERIFY_MAX_CONSUMERS == V.LIMIT


def test_ctypes_prototypes_exist():
    lib = N.load()
    batch_p = ctypes.POINTER(N.DeviceBatch)
    assert lib.la_verify_assignment_device.restype is ctypes.c_int
    assert lib.la_verify_assignment_device.argtypes == [ctypes.c_void_p, batch_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.la_verify_assignment_device_on.restype is ctypes.c_int
    assert lib.la_verify_assignment_device_on.argtypes == [ctypes.c_void_p, ctypes.c_int, batch_p, ctypes.c_void_p, ctypes.c_void_p,
                                                           ctypes.c_void_p]
    assert {"la_verify_assignment_device", "la_verify_assignment_device_on"} <= set(N.EXPORTED_SYMBOLS)
    assert callable(N.Context.verify_assignment_device)


def test_a_null_context_is_refused_without_a_device():
    lib = N.load()
    b = N.DeviceBatch()
    assert lib.la_verify_assignment_device(None, ctypes.byref(b), None, None, None) == N.LA_EINVAL
    assert lib.la_verify_assignment_device_on(None, 0, ctypes.byref(b), None, None, None) == N.LA_EINVAL
