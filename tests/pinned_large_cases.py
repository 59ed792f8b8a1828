"""Cases of la_assign_pinned_device with LA_FLAG_PINNED_LARGE shared by tests/test_pinned_large_cpu.py,
tests/test_pinned_large_gpu.py and tests/test_assign_coop_pinned_large_gpu.py: the smallest shapes that reach each edge of the
large form, built on pinned_cases.  The expectation is pinned_cases.dict_model with its partition limit lifted -- written
independently of sharding.assign_pinned_numpy, which tests/test_pinned_large_cpu.py holds against it.  Not a test module."""
import functools

import numpy as np

import pinned_cases
from pinned_cases import I64, MAX_C, MAX_P, PinnedCase, drawn, topic

ANY_SIZE = (1 << 30) - 2                # LA_PINNED_LARGE_MAX_PARTITIONS


def model(c):
    """dict_model(c) with the partition limit at ANY_SIZE (the consumer limit stays)."""
    keep = pinned_cases.MAX_P
    pinned_cases.MAX_P = ANY_SIZE
    try:
        return pinned_cases.dict_model(c)
    finally:
        pinned_cases.MAX_P = keep


def is_large(c):
    """Per topic: what the flagged call sends through the large form."""
    return (np.diff(c.part_off) > MAX_P) & (np.diff(c.cons_off) <= MAX_C)


def _held(seed, p, holds, lags="u20"):
    """One topic of p partitions over len(holds) consumers: consumer k owns holds[k] of them, the rest is free."""
    rng = np.random.default_rng(seed)
    t = topic(rng, p, range(len(holds)), lags)
    who = np.repeat(np.arange(len(holds)), holds)
    assert who.size <= p
    claims = [(int(k), 0, int(i)) for k, i in zip(who, t[0][:who.size])]
    return PinnedCase([t], len(holds), claims)


def _extreme():
    rng = np.random.default_rng(71)
    ids, lags, ranks = topic(rng, MAX_P + 1, [0, 2, 3], "full")
    lags[:40] = I64.max - rng.integers(0, 3, 40)
    lags[40:80] = I64.min + rng.integers(0, 3, 40)
    lags[80:120] = -rng.integers(0, 5, 40)
    order = rng.permutation(lags.size)
    t = (ids, lags[order], ranks)
    return PinnedCase([t], 4, pinned_cases.owners(rng, [t], 4, 0.5, 0.0))


def _duplicate_id():
    rng = np.random.default_rng(72)
    ids, lags, ranks = topic(rng, MAX_P + 1, [0, 1, 2])
    ids[7] = ids[3000]                                                   # one id twice, and owned: both entries are pinned
    t = (ids, lags, ranks)
    claims = [(int(rng.integers(0, 3)), 0, int(i)) for i in np.unique(ids)[::2]]
    if not any(i == int(ids[7]) for _, _, i in claims):
        claims.append((1, 0, int(ids[7])))
    return PinnedCase([t], 3, claims)


CASES = {
    "one past": lambda: drawn(60, [(MAX_P + 1, 3)], 4, owned=0.5),
    "nothing owned": lambda: drawn(61, [(MAX_P + 1, 5), (2 * MAX_P + 1, 7), (4 * MAX_P + 1, 3)], 9, lags="ties", owned=0.0),
    "neighbours": lambda: drawn(62, [(21, 3), (MAX_P + 1, 4), (0, 2), (MAX_P, 5), (5000, 0), (9, 2)], 7, owned=0.5, foreign=0.1),
    "two large": lambda: drawn(63, [(MAX_P + 1, 4), (6000, 9)], 9, owned=0.6, foreign=0.1),
    "three large": lambda: drawn(63, [(MAX_P + 1, 4), (6000, 9), (4500, 2)], 9, owned=0.6, foreign=0.1),
    "caught up": lambda: drawn(64, [(3 * MAX_P + 1, 6)], 7, lags="zero", owned=0.5),
    "extreme lags": _extreme,
    "duplicate id": _duplicate_id,
    "lone consumer alone": lambda: drawn(65, [(4200, 1)], 2, owned=0.5, foreign=0.3),
    "lone consumer: the run ends at m2": lambda: _held(66, 4200, [0] + [520] * 7),
    "lone consumer: the run ends at F": lambda: _held(67, 4200, [0] + [557] * 6 + [558]),
    "short last level": lambda: _held(68, 4100, [580] * 7),
    "foreign and stale": lambda: drawn(69, [(MAX_P + 1, 4)], 8, owned=0.6, foreign=0.33, n_stale=9, n_unmapped=4, head=2, tail=3),
    "2048 consumers": lambda: drawn(70, [(MAX_P + 1, MAX_C)], MAX_C, owned=0.3),
}

# a topic over the consumer limit next to a large one that must still be exact: LA_ESHAPE, the topic untouched
OVER_CONSUMERS = lambda: drawn(73, [(MAX_P + 1, MAX_C), (MAX_P + 1, MAX_C + 1)], MAX_C + 1, owned=0.3)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case and its expectation, computed once (neither is to be modified)."""
    c = CASES[name]()
    return c, model(c)
