"""The yardstick of test_verify_large_gpu.py -- sharding.verify_assignment_numpy with max_partitions / max_consumers raised -- held to
the oracle on topics over the 4 096 x 4 096 limit, without a GPU: all-zero verdicts on the oracle's results at the shapes of
verify_large_cases, and after every fault of the catalogue a non-zero verdict with the fault's class bit exactly in the mutated
topic.  These tests pin the yardstick (it takes the limits as arguments since it was written); the binding's new constants too."""
import os
import re

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N

import verify_cases as V
import verify_large_cases as L


def test_the_shape_batch_is_what_the_issue_lists():
    w = L.shape_batch()
    assert len(L.LARGE) == 12 and [L.is_large(w, t) for t in range(w.n_topics)] == [t in L.LARGE for t in range(w.n_topics)]
    assert w.n_partitions <= 260_000


@pytest.mark.parametrize("lags", L.LAGS)
def test_oracle_results_are_certified_at_every_large_shape(lags):
    w = L.shape_batch(lags=lags, ids="full")
    exp = V.oracle_result(w)
    verdict, summary = L.yardstick(w, exp)
    assert not verdict.any(), "%s: topics %s are not certified: %s" % (lags, np.flatnonzero(verdict), verdict[verdict != 0])
    np.testing.assert_array_equal(summary, [0, 0, -1, -1])
    verdict, summary = V.yardstick(w, exp)                           # the limits as they are without the flag
    want_v, want_s = L.unflagged_pattern(w)
    np.testing.assert_array_equal(verdict, want_v)
    np.testing.assert_array_equal(summary, want_s)


@pytest.mark.parametrize("shape", L.CATALOGUE_SHAPES)
def test_every_fault_of_the_catalogue_is_found_in_its_large_topic_only(shape):
    w = L.catalogue_batch(shape)
    exp = V.oracle_result(w)
    cases = [c for c in V.catalogue_cases(w, exp) if c[1] == 1]
    if shape == (5000, 37):                                          # every fault but the one that needs a topic without consumers
        missing = set(V.CATALOGUE) - {c[0] for c in cases} - {"rank in a topic without consumers"}
        assert not missing, "no place in %s for %s" % (shape, missing)
    assert cases
    for name, t, res in cases:
        assert V.differing_topics(w, res, exp) == [t], "%s: the mutation must change topic %d and no other" % (name, t)
        verdict, summary = L.yardstick(w, res)
        assert verdict[t] & V.CATALOGUE[name], "%s at %s: verdict %d lacks its class bit" % (name, shape, verdict[t])
        assert not verdict[t] & V.UNCHECKED
        assert list(np.flatnonzero(verdict)) == [t], "%s at %s: verdicts %s" % (name, shape, verdict)
        np.testing.assert_array_equal(summary, [1, 0, t, -1])


def test_constants_match_the_header_and_the_kernels():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lagassign.h")).read()
    kernels = open(os.path.join(root, "kafka_lag_based_assignor_amd", "csrc", "la_kernels.h")).read()
    assert int(re.search(r"#define LA_FLAG_VERIFY_LARGE\s+(\d+)", header).group(1)) == N.LA_FLAG_VERIFY_LARGE == 8192
    flags = [int(m) for m in re.findall(r"#define LA_FLAG_\w+\s+(\d+)", header)]
    assert len(flags) == len(set(flags)), "two flags share a value"
    assert int(re.search(r"kVerifyGlobalLaunches = (\d+);", kernels).group(1)) + 1 == N.VERIFY_MAX_LAUNCHES <= 8
    assert "at most %d kernel launches" % N.VERIFY_MAX_LAUNCHES in header
    assert N.VERIFY_GLOBAL_MAX_PARTITIONS == (1 << 30) - 2
