"""tools/settle_model.py -- the numpy replay of settle_lanes_p64 (csrc/la_sort64.h): even / odd exchange passes, the stop
rule, the cap of K pairs and the fall-back to the network give np.sort of every row, and the stop rule never fires on a row
that is not sorted.  The GPU tests (test_tile_settle_gpu.py) choose their cases with this model."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import settle_model as M  # noqa: E402

D, K = M.D_DEFAULT, M.K_DEFAULT
SENT = M.SENTINEL


def _check(rows, lc, d=D, k=K):
    got, info = M.settle_wave(rows, lc, d, k)
    for g, r in zip(got, rows):
        np.testing.assert_array_equal(g, np.sort(np.asarray(r, np.uint64)))
    assert not info["stopped_unsorted"]
    assert info["pairs"] <= k and info["passes"] <= 2 * k
    return info


def _unique_row(rng, n, live=None):
    live = n if live is None else live
    r = np.full(n, SENT, np.uint64)
    r[:live] = (np.sort(rng.choice(1 << 40, live, replace=False)).astype(np.uint64) << np.uint64(6)) | rng.permutation(live).astype(np.uint64)
    return r


def _with_descents(rng, n, want):
    """A row of n unique elements with exactly `want` descents: want + 1 ascending runs of a random permutation (None where
    two runs happen to join ascending: the caller draws again)."""
    vals = np.sort(rng.choice(1 << 30, n, replace=False)).astype(np.uint64)
    cuts = np.sort(rng.choice(np.arange(1, n), want, replace=False))
    row = vals[np.concatenate([np.sort(r) for r in np.split(rng.permutation(n), cuts)])]
    return row if M.descents(row) == want else None


@pytest.mark.parametrize("n", [32, 64])
def test_random_rows_sort(n):
    rng = np.random.default_rng(n)
    seen = set()
    for _ in range(300):
        seen.add(_check([rng.permutation(n).astype(np.uint64)], n)["outcome"])
        r = np.arange(n, dtype=np.uint64)                          # nearly ordered: a few neighbour swaps
        for i in rng.choice(n - 1, int(rng.integers(0, 4)), replace=False):
            r[i], r[i + 1] = r[i + 1], r[i]
        seen.add(_check([r, _unique_row(rng, n)], n)["outcome"])
    assert {"in_order", "settled", "not_tried"} <= seen


@pytest.mark.parametrize("want", range(1, 9))
def test_rows_with_exact_descent_counts(want):
    rng = np.random.default_rng(want)
    done = 0
    outcomes = set()
    while done < 100:
        row = _with_descents(rng, 32, want)
        if row is None:
            continue
        done += 1
        info = _check([row], 32)
        assert info["descents"] == want
        outcomes.add(info["outcome"])
    if want > D:
        assert outcomes == {"not_tried"}
    else:
        assert "not_tried" not in outcomes and "in_order" not in outcomes


@pytest.mark.parametrize("n,k", [(32, 3), (32, 4), (64, 4), (64, 6)])
def test_smallest_element_too_far_right_forces_the_give_up(n, k):
    """The smallest element 2K + 1 places right of its home needs 2K + 1 passes: K pairs cannot settle it."""
    row = np.arange(1, n + 1, dtype=np.uint64)
    row = np.concatenate([row[1:2 * k + 2], row[:1], row[2 * k + 2:]])
    assert int(np.argmin(row)) == 2 * k + 1 and M.descents(row) == 1
    info = _check([row], n, D, k)
    assert info["outcome"] == "gave_up" and info["pairs"] == k
    # one place nearer and the last odd pass finds nothing left to do
    row = np.arange(1, n + 1, dtype=np.uint64)
    row = np.concatenate([row[1:2 * k], row[:1], row[2 * k:]])
    info = _check([row], n, D, k)
    assert info["outcome"] == "settled" and info["pairs"] == k


@pytest.mark.parametrize("lc", [32, 64])
def test_sentinels_at_every_consumer_count(lc):
    rng = np.random.default_rng(lc)
    for c in range(1, lc + 1):
        for _ in range(4):
            row = _unique_row(rng, lc, c)
            for i in rng.choice(max(c - 1, 1), min(2, max(c - 1, 0)), replace=False) if c > 1 else []:
                row[i], row[i + 1] = row[i + 1], row[i]
            got, info = M.settle_wave([row], lc)
            np.testing.assert_array_equal(got[0], np.sort(row))
            assert np.all(got[0][c:] == SENT) and not info["stopped_unsorted"]


def test_fewer_than_32_lanes_take_the_network():
    row = np.array([1, 0] + list(range(2, 16)), np.uint64)
    assert _check([row], 16)["outcome"] == "not_tried"


def test_stop_rule_never_fires_on_an_unsorted_row():
    """Every order of 6 elements beside a sorted neighbour group, with a cap large enough that the settle always ends by its
    stop rule: it stops only on sorted rows."""
    import itertools
    other = np.arange(6, dtype=np.uint64)
    for perm in itertools.permutations(range(6)):
        row = np.array(perm, np.uint64)
        got, info = M.settle_wave([row, other], 32, d=6, k=6)
        assert not info["stopped_unsorted"] and info["outcome"] in ("in_order", "settled")
        assert M.descents(got[0]) == 0
    rng = np.random.default_rng(9)
    for _ in range(500):
        for k in (1, 2, 3, 4, 6):
            _check([rng.permutation(32).astype(np.uint64), np.arange(32, dtype=np.uint64)], 32, d=32, k=k)


def test_decisions_are_per_wavefront():
    """The group with the most descents decides whether the settle is tried; the slowest group how many pairs run."""
    rng = np.random.default_rng(5)
    calm = np.arange(32, dtype=np.uint64)
    wild = rng.permutation(32).astype(np.uint64)
    assert M.descents(wild) > D
    assert _check([calm, wild], 32)["outcome"] == "not_tried"
    assert _check([wild, calm], 32)["outcome"] == "not_tried"
    one = calm.copy()
    one[[4, 5]] = one[[5, 4]]
    far = np.concatenate([calm[1:2 * K], calm[:1], calm[2 * K:]])
    a, b = _check([one, far], 32), _check([far, one], 32)
    assert a["pairs"] == b["pairs"] == K and a["outcome"] == "settled"
    assert _check([one, calm], 32)["pairs"] == 1


def test_replay_matches_the_literal_greedy():
    """replay_wave's bins are the reference's: after the last round the totals per consumer equal oracle.assign_flat's."""
    from kafka_lag_based_assignor_amd import synth
    from oracle import oracle
    for dist, p, c in (("zipf", 256, 32), ("pareto", 250, 31), ("uniform40", 96, 17)):
        w = synth.make_uniform("m", 6, 2, p, c, dist, offsets=False)
        _, _, totals = oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
        for t in range(2):
            s = M.sorted_lags(w.lag[t * p:(t + 1) * p], w.partition_id[t * p:(t + 1) * p])
            bins = np.arange(c, dtype=np.uint64)
            entering = {}
            for q in range((p + c - 1) // c):
                entering[q] = bins.copy()
                bins = np.sort(bins)
                take = s[q * c:(q + 1) * c].astype(np.uint64)
                bins[:take.size] += take << np.uint64(6)
            got = np.zeros(c, np.int64)
            got[(bins & np.uint64(63)).astype(np.int64)] = (bins >> np.uint64(6)).astype(np.int64)
            np.testing.assert_array_equal(got, totals[t * c:(t + 1) * c])
            # the rows the model hands to the settle are those bins, round by round, sentinels behind them
            seen = 0
            for q, found, info in M.replay_wave([(s, c)], 32):
                np.testing.assert_array_equal(found[0][:c], entering[q])
                assert np.all(found[0][c:] == SENT)
                seen += 1
            assert seen == (p + c - 1) // c - 2
