"""The yardstick of the hostile-offset tests and their inputs, checked without a GPU: java_lags (tests/offset_cases.py) against
the two readings of computePartitionLag the suite already has, on every triple of the corner values; and the coverage check on
every batch that test_hostile_offsets_gpu.py runs."""
import numpy as np
import pytest

from oracle import literal_py, oracle
import offset_cases as oc


def _grid():
    b, e, c = np.meshgrid(oc.CORNERS, oc.CORNERS, oc.CORNERS, indexing="ij")
    return b.ravel().copy(), e.ravel().copy(), c.ravel().copy()


def test_corners_are_the_fourteen():
    assert oc.CORNERS.size == 14 and (np.diff(oc.CORNERS) > 0).all()
    assert oc.CORNERS[0] == np.iinfo(np.int64).min and oc.CORNERS[-1] == np.iinfo(np.int64).max
    assert all(v in oc.CORNERS for v in oc.NONE_CODES)


@pytest.mark.parametrize("latest", [False, True])
def test_three_readings_agree_on_every_corner_triple(latest):
    begin, end, com = _grid()
    assert end.size == 14 ** 3
    mine = oc.java_lags(begin, end, com, latest)
    np.testing.assert_array_equal(mine, oracle.compute_lags(begin, end, com, latest))
    mode = "latest" if latest else "earliest"
    lit = [literal_py.compute_partition_lag(None if c < 0 else int(c), int(b), int(e), mode) for b, e, c in zip(begin, end, com)]
    np.testing.assert_array_equal(mine, np.array(lit, np.int64))
    one = [oracle.compute_partition_lag(None if c < 0 else int(c), int(b), int(e), mode) for b, e, c in zip(begin[::7], end[::7], com[::7])]
    np.testing.assert_array_equal(mine[::7], np.array(one, np.int64))
    assert (mine >= 0).all()
    if latest:
        np.testing.assert_array_equal(mine, oc.java_lags(None, end, com, True))            # begin is never read
        np.testing.assert_array_equal(mine[com < 0], 0)
    else:
        # the grid is no tame one: most lags clamp to 0, a fifth are beyond 2^62
        assert 0.5 < (mine == 0).mean() < 0.65 and 0.15 < (mine > (1 << 62)).mean() < 0.3
        zero_begin = oc.java_lags(None, end, com, False)                                     # no begin array: begin 0
        np.testing.assert_array_equal(zero_begin, oc.java_lags(np.zeros_like(end), end, com, False))
        np.testing.assert_array_equal(zero_begin, oracle.compute_lags(None, end, com, False))


def test_the_named_wraps():
    mn, mx = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    lag = oc.java_lags(np.array([0, 0, -5, mx]), np.array([mn, -1, 5, mn]), np.array([1, mx, -1, -2]), False)
    assert lag.tolist() == [mx, 0, 10, 1]


@pytest.mark.parametrize("regime", oc.REGIMES)
def test_every_gpu_batch_passes_the_coverage_check(regime):
    """make_case runs check_coverage on what it generates; here also: the check is not vacuous for the batches that matter."""
    mixed = 0
    for shapes, patterns in oc.gpu_batches():
        for pattern in patterns:
            w = oc.make_case(shapes, regime, pattern)
            assert w.n_partitions == sum(s[0] for s in shapes)
            mixed += oc.is_mixed(w.n_partitions, pattern)
            none = w.committed < 0
            assert none.any() == (pattern != "never") and (~none).any() == (pattern != "all")
    assert mixed >= 20


@pytest.mark.parametrize("regime", oc.REGIMES)
@pytest.mark.parametrize("pattern", ["even", "odd", "50%"])
def test_coverage_at_the_smallest_mixed_size(regime, pattern):
    for seed in range(20):
        b, e, c = oc.hostile(np.random.default_rng(seed), 64, regime, pattern)
        oc.check_coverage(b, e, c, regime, pattern)


def test_the_coverage_check_notices_a_hollow_case():
    rng = np.random.default_rng(1)
    b, e, c = oc.hostile(rng, 256, "tame-range", "50%")
    tame = np.where(c < 0, np.int64(-1), c)                                  # one none-encoding only
    with pytest.raises(AssertionError):
        oc.check_coverage(b, e, tame, "tame-range", "50%")
    with pytest.raises(AssertionError):
        oc.check_coverage(b, np.maximum(e, np.maximum(c, b)), c, "tame-range", "50%")     # nothing clamps
    with pytest.raises(AssertionError):
        oc.check_coverage(np.zeros_like(b), e, c, "tame-range", "50%")       # begin not poisoned
