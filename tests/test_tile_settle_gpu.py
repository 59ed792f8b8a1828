"""Greedy rounds whose nearly ordered bins are settled by neighbour exchanges (settle_lanes_p64, csrc/la_sort64.h), bit for
bit against the literal oracle: ids, member ranks and totals.

From the third round on a wavefront of the packed tile kernel counts the descents of its consumer bins; with none the round
sorts nothing, with at most D per group it runs (even, odd) exchange passes until one exchanges nothing, at most K pairs, and
only then -- or with more descents, or with fewer than 32 lanes of bins -- the bitonic network.  All decisions are per
wavefront.  tools/settle_model.py replays the rounds; the tests below ASSERT with it that their lags reach every branch.

Group widths are reached as in test_tile_chain_gpu.py: a batch of more than 2 048 topics of up to 256 x 32 stays at L = 32 (two
topics per wavefront), a small one is widened to L = 64 (one topic per wavefront, 32 lanes of bins); 64 consumers are L = 64.
"""
import functools
import os
import sys

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from gpu_helpers import _same3
# the guarded device call, the shared oracle cache and the lag-carrying batch builder live in test_tile_chain_gpu.py (not in
# gpu_helpers.py): this file runs the same forms on the same footing, so it takes them from there by name
from test_tile_chain_gpu import PACK_BOUNDS, _call, _expect, _with_lags

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import settle_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

# kSettleMaxDescents / kSettleMaxPairs of csrc/la_sort64.h (LA_SETTLE_D / LA_SETTLE_K)
D, K = 4, 4
assert (D, K) == (M.D_DEFAULT, M.K_DEFAULT)

FAMILIES = ("zipf0.8", "zipf1.1", "zipf1.5", "pareto", "uniform", "equal", "zero", "giant")


def _family(kind, p, rng, scale=1.0):
    k = np.arange(1, p + 1, dtype=np.float64)
    if kind.startswith("zipf"):
        lag = np.floor(1e9 * scale / k ** float(kind[4:]))
    elif kind == "pareto":
        lag = np.floor(np.minimum(float(1 << 40), 1000.0 * (1.0 - rng.random(p)) ** (-1.0 / 1.5)))
    elif kind == "uniform":
        lag = rng.integers(0, 1 << 40, p)
    elif kind == "equal":
        lag = np.full(p, 12345)
    elif kind == "zero":
        lag = np.zeros(p)
    else:
        lag = rng.integers(0, 1000, p)
        lag[int(rng.integers(0, p))] = 1 << 40                   # one giant lag
    return rng.permutation(np.asarray(lag, np.int64))


def _crafted(order, p, c, rng):
    """Lags of a p x c topic whose bins, when the THIRD round's sort starts, are ordered like `order` (a permutation of
    0..c-1) and stay in order afterwards.  Round 0 gives the bin that the second round finds at place j the lag base + 100 j,
    round 1 adds order[j] + 100 (c - 1 - j): together base + 100 (c - 1) + order[j].  All later lags are zero."""
    order = np.asarray(order, np.int64)
    assert sorted(order.tolist()) == list(range(c)) and p >= 3 * c
    j = np.arange(c, dtype=np.int64)
    first = 1000000 + 100 * j                                    # ascending in j = the reverse of round 0's descending lags
    second = order + 100 * (c - 1 - j)                           # descending in j, all below `first`
    assert np.all(np.diff(second) < 0) and second.max() < first.min()
    lag = np.concatenate([first[::-1], second, np.zeros(p - 2 * c, np.int64)])
    return rng.permutation(lag)


def _far(c, pos):
    """0..c-1 with the smallest element `pos` places right of its home: one descent, settled by exactly `pos` passes."""
    return list(range(1, pos + 1)) + [0] + list(range(pos + 1, c))


def _swap(c, i):
    o = list(range(c))
    o[i], o[i + 1] = o[i + 1], o[i]
    return o


def _orders(c, rng):
    """Named bin orders for _crafted, by what the settle does with them."""
    out = {"in order": list(range(c)), "not tried": list(range(c))[::-1], "gives up": _far(c, 2 * K + 1)}
    for pairs in range(1, K + 1):
        out["%d pairs" % pairs] = _far(c, 2 * pairs - 1)
    wild = rng.permutation(c).tolist()
    assert M.descents(np.array(wild, np.uint64)) > D
    out["shuffled"] = wild
    for i in (15, 31, 47):
        if i + 1 < c:
            out["only %d|%d" % (i, i + 1)] = _swap(c, i)
    return out


def _wave_pairs(p, c, rng):
    """Pairs of topics of one p x c shape that share a wavefront at L = 32, as (name, lags) pairs: the lag families next to
    each other, the crafted orders in both lane orders, and a topic whose totals are all above its neighbour's."""
    fam = [(f, _family(f, p, rng)) for f in FAMILIES]
    pairs = [(fam[i], fam[i + 1]) for i in range(0, len(fam), 2)] + [(fam[1], fam[1]), (fam[2], fam[0])]
    if p >= 3 * c:
        o = {k: (k, _crafted(v, p, c, rng)) for k, v in _orders(c, rng).items()}
        both = [("in order", "gives up"), ("in order", "not tried"), ("in order", "shuffled"), ("1 pairs", "%d pairs" % K)]
        both += [("in order", k) for k in o if k.startswith("only")]
        for a, b in both:
            pairs += [(o[a], o[b]), (o[b], o[a])]
        pairs += [(o["%d pairs" % n], o["%d pairs" % n]) for n in range(1, K + 1)]
    hi = ("zipf1.1 x 1000", _family("zipf1.1", p, rng, 1000.0))
    lo = ("zipf1.1 / 1000", _family("zipf1.1", p, rng, 0.001))
    assert np.sort(hi[1])[::-1][:c].min() > lo[1].sum()           # after round 0 every bin of `hi` is above every bin `lo` ever has
    return pairs + [(hi, lo), (lo, hi)]


def _classes(topics, l):
    """Classes (settle_model.classify) over the wavefronts of a plain batch: 64 / l consecutive topics each."""
    g = 64 // l
    out = set()
    for t in range(0, len(topics) - g + 1, g):
        out |= M.classify([(np.sort(lag)[::-1], c) for _, c, lag in topics[t:t + g]], l, D, K)
    return out


ALL_CLASSES = {"in_order", "gave_up", "not_tried"} | {"settled_%d" % n for n in range(1, K + 1)}


def _batch(topics, seed):
    return _with_lags([(p, c) for p, c, _ in topics], [lag for _, _, lag in topics], seed)


def _forms(ctx, key, w, small):
    """Two-launch form, bounded single launch and bounded with wire elements out; a small batch also the resident single-launch
    form (flags 0) and each of them through the topic list."""
    exp = _expect(key, w)
    bounds = (PACK_BOUNDS, int(w.partition_id.max(initial=0)))
    _same3(_call(ctx, w, N.LA_FLAG_DEFER_WIDE), exp, key + " two launches")
    _same3(_call(ctx, w, 0, bounds), exp, key + " bounded")
    assert ctx.last_launches() == 1, key
    _same3(_call(ctx, w, 0, bounds, wire=True), exp, key + " bounded, wire out")
    assert ctx.last_launches() == 1, key
    if small:
        _same3(_call(ctx, w, 0), exp, key + " resident")
        _same3(_call(ctx, w, N.LA_FLAG_RAGGED), exp, key + " resident, topic list")
        _same3(_call(ctx, w, N.LA_FLAG_DEFER_WIDE, bounds), exp, key + " bounded, two-launch flags")


SHAPES_32 = [(256, 32), (250, 32), (256, 31), (200, 17), (96, 32)]


@functools.lru_cache(maxsize=None)
def _topics_32():
    rng = np.random.default_rng(32)
    topics = []
    for p, c in SHAPES_32:
        for (_, a), (_, b) in _wave_pairs(p, c, rng):
            topics += [(p, c, a), (p, c, b)]
    return topics


def test_two_groups_per_wavefront(ctx):
    """L = 32: 256 x 32, 250 x 32 (partial last round), 256 x 31 and 200 x 17 (sentinels inside the 32 lanes), 96 x 32 (three
    rounds: the settle runs exactly once) -- every pair of _wave_pairs in one wavefront, then fillers of 8 x 1 up to 2 052
    topics so that the batch keeps its narrow shape."""
    topics = _topics_32()
    assert len(topics) % 2 == 0 and len(topics) < 2052
    got = _classes(topics, 32)
    assert ALL_CLASSES | {"only_15|16"} <= got, sorted(ALL_CLASSES - got)
    # 96 x 32: rounds 0, 1, 2 -- one settle per topic
    assert all(len(list(M.replay_wave([(np.sort(lag)[::-1], c)], 32))) == 1 for p, c, lag in topics if p == 96)
    fill = [(8, 1, np.zeros(8, np.int64))] * (2052 - len(topics))
    _forms(ctx, "settle L=32", _batch(topics + fill, 1), small=False)


@pytest.mark.parametrize("shape", SHAPES_32)
def test_small_batch_one_group_of_64_lanes_32_bins(ctx, shape):
    """The same topics as a small batch: widened to one 64-lane group per topic, its bins on 32 lanes (LC = 32 < L = 64), the
    resident single-launch form included.  Each wavefront decides for its one topic."""
    topics = [t for t in _topics_32() if (t[0], t[1]) == shape]
    got = _classes(topics, 64)
    want = ALL_CLASSES if shape[0] >= 3 * shape[1] else {"in_order", "not_tried"}
    assert want <= got, sorted(want - got)
    _forms(ctx, "settle small %dx%d" % shape, _batch(topics, 2), small=True)


@pytest.mark.parametrize("shape", [(1024, 64), (512, 33)])
def test_one_group_of_64_bins(ctx, shape):
    """L = 64, LC = 64: exchange pairs across lanes 15|16, 31|32 and 47|48 (the DPP rows' and the 32-lane halves' borders)."""
    p, c = shape
    rng = np.random.default_rng(p)
    topics = [(p, c, _family(f, p, rng)) for f in FAMILIES]
    topics += [(p, c, _crafted(v, p, c, rng)) for v in _orders(c, rng).values()]
    got = _classes(topics, 64)
    want = ALL_CLASSES | {"only_15|16", "only_31|32"} | ({"only_47|48"} if c > 48 else set())
    assert want <= got, sorted(want - got)
    _forms(ctx, "settle L=64 %dx%d" % shape, _batch(topics, 3), small=True)


def test_sixteen_bins_take_the_network(ctx):
    """128 x 16: LC = 16, the settle is compiled out; every round with a descent is "not tried"."""
    rng = np.random.default_rng(16)
    topics = [(128, 16, _family(f, 128, rng)) for f in FAMILIES]
    topics += [(128, 16, _crafted(v, 128, 16, rng)) for v in _orders(16, rng).values()]
    got = _classes(topics, 64)                                    # (a small batch: widened to L = 64, bins on 16 lanes)
    assert got & (ALL_CLASSES - {"in_order", "not_tried"}) == set() and "not_tried" in got
    _forms(ctx, "settle LC=16", _batch(topics, 4), small=True)
