"""Batches for la_verify_assignment_device with LA_FLAG_VERIFY_LARGE: topics over the 4 096 x 4 096 limit of one workgroup's LDS,
which the global form (tables in device memory) verifies.  Not a test module: test_verify_large_cpu.py (the yardstick with its
limits raised, against the oracle) and test_verify_large_gpu.py (the kernels against that yardstick) import it by name, so both
run the same cases.  Batches and their oracle results are built once and shared: treat them as read-only."""
import numpy as np

import verify_cases as V

NO_LIMIT = 1 << 62              # max_partitions / max_consumers of the yardstick: nothing is over the limit

# the smallest shapes at which the global form can go wrong, small topics around them:
#   4097 x 8, 4096 x 4097, 64 x 4097    each side of the routing boundary; 64 x 4097 is one partial round, 4 033 consumers left out
#   8193 x 1, 20000 x 3, 100003 x 2     the two-level scan with a ragged last chunk
#   12289 x 4099                        three rounds, 8 consumers left out
#   70001 x 600                         positions beyond 16 bits
#   5000 x 0                            large, no consumers
SHAPES = [(64, 8), (4097, 8), (64, 4097), (5000, 5000), (10000, 128), (8193, 1), (20000, 3), (100003, 2), (4097, 4096), (4096, 4097),
          (5000, 0), (70001, 600), (12289, 4099), (30, 5)]
LARGE = [t for t, (p, c) in enumerate(SHAPES) if p > V.LIMIT or c > V.LIMIT]
CATALOGUE_SHAPES = ((5000, 37), (4100, 4097), (8193, 1))
LAGS = ("mixed", "equal", "zero", "wrap", "negative")

_batches = {}


def is_large(w, t):
    return int(w.part_off[t + 1] - w.part_off[t]) > V.LIMIT or int(w.cons_off[t + 1] - w.cons_off[t]) > V.LIMIT


def batch(shapes, seed, **kw):
    """V.batch, built once per argument set."""
    key = (tuple(shapes), seed, tuple(sorted(kw.items())))
    if key not in _batches:
        _batches[key] = V.batch(list(shapes), seed, **kw)
    return _batches[key]


def shape_batch(lags="mixed", ids="shuffled"):
    return batch(SHAPES, 21, lags=lags, ids=ids)


def catalogue_batch(shape):
    """[(64, 8), shape, (40, 0), (30, 5)]: small topics on both sides of the large one; the faults go into topic 1."""
    return batch([(64, 8), shape, (40, 0), (30, 5)], 5)


def two_large_batch():
    """Two large topics, one by its partitions and one by its consumers, between small ones, an empty one among them."""
    return batch([(37, 3), (5000, 37), (1, 1), (300, 4097), (0, 2), (1025, 9)], 55)


def yardstick(w, res, **kw):
    """sharding.verify_assignment_numpy without a size limit: what the flagged call computes."""
    return V.yardstick(w, res, max_partitions=NO_LIMIT, max_consumers=NO_LIMIT, **kw)


def unflagged_pattern(w):
    """The verdicts of an unflagged call on the oracle's results: UNCHECKED for every topic over the limit, 0 elsewhere."""
    v = np.array([V.UNCHECKED if is_large(w, t) else 0 for t in range(w.n_topics)], np.int32)
    hit = np.flatnonzero(v)
    return v, np.array([0, hit.size, -1, int(hit[0]) if hit.size else -1], np.int64)
