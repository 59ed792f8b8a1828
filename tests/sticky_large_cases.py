"""Case builders for la_sticky_ties_device with LA_FLAG_STICKY_LARGE (topics of more than 4096 partitions, re-matched through
tables in device memory).  Not a test module: test_sticky_large_cpu.py (the yardstick without a limit against the independent
model, and that the case table reaches the edges it names) and test_sticky_large_gpu.py (the device against the yardstick)
import it by name.  The yardstick is S.expect(w, res, prev, max_partitions=sharding.STICKY_ANY_SIZE).  Every case stays within
50 000 partitions; cases are built once and shared: treat them as read-only."""
import functools

import numpy as np

from kafka_lag_based_assignor_amd import sharding

import sticky_cases as S

LIMIT = sharding.STICKY_MAX_PARTITIONS
ANY = sharding.STICKY_ANY_SIZE
I64 = np.iinfo(np.int64)
SHAPE_P = (LIMIT + 1, 2 * LIMIT + 1, 4 * LIMIT + 1)
KINDS = ("mixed", "shifted", "own")
# the sort's tiles hold 4 096 or 8 192 elements, and a position is two elements: positions and elements both cross a tile edge here
EDGES = (2048, 4096, 8192)


def expect(w, res, prev, **kw):
    return S.expect(w, res, prev, max_partitions=ANY, **kw)


def big_topics(w):
    """Indices of the topics the global form takes."""
    return [t for t in range(w.n_topics) if int(w.part_off[t + 1] - w.part_off[t]) > LIMIT]


def concat_positions(w):
    """Position in the concatenated list of all large topics' positions -> batch position."""
    return np.concatenate([np.arange(int(w.part_off[t]), int(w.part_off[t + 1])) for t in big_topics(w)] + [np.empty(0, np.int64)]).astype(np.int64)


def _shape(p):
    rng = np.random.default_rng(100 + p)
    return S.workload([(S.mixed_lags(p, rng), 7)], 100 + p)


def _neighbours():
    return S.workload([(np.zeros(LIMIT + 1, np.int64), 3), (np.zeros(LIMIT + 2, np.int64), 5)], 21)


def _mixed_batch():
    rng = np.random.default_rng(22)
    return S.workload([(S.mixed_lags(LIMIT + 1, rng), 7), (S.mixed_lags(50, rng), 3), (np.empty(0, np.int64), 2),
                       (np.zeros(LIMIT, np.int64), 4), (S.caught_up_lags(5000, 0.01, rng), 16), (S.mixed_lags(300, rng), 5),
                       (S.mixed_lags(LIMIT + 7, rng), 0)], 22)


def _one_run():
    return S.workload([(np.full(3 * LIMIT + 1, 77, np.int64), 9)], 23)


def _no_ties():
    rng = np.random.default_rng(24)
    return S.workload([(rng.permutation(LIMIT + 1).astype(np.int64) + 1, 6)], 24)


def _extremes():
    rng = np.random.default_rng(25)
    values = np.array([I64.min, I64.max, I64.min + 1, I64.max - 1, -5, -1, 0, 1], np.int64)
    return S.workload([(values[rng.integers(0, values.size, LIMIT + 1)], 5), (values[rng.integers(0, 3, LIMIT + 3)], 4)], 25)


def _caught_up():
    rng = np.random.default_rng(26)
    return S.workload([(S.caught_up_lags(12000, 0.01, rng), 16)], 26)


def _straddle():
    """Runs across positions 2 048, 4 096 and 8 192 of the concatenated list (topic 0 ends at 4 200): [1900, 2300), [4000, 4200)
    and, in topic 1, positions 3 900 .. 5 000 = [8100, 9200) of the list; three consumers, so every member's places in such a
    run lie on both sides of the edge."""
    rng = np.random.default_rng(27)
    return S.workload([(S.lags_of_runs([1900, 400, 1700, 200], rng), 3), (S.lags_of_runs([3900, 1100], rng), 3)], 27)


def _three_of(total):
    rng = np.random.default_rng(28)
    p = total // 3
    return S.workload([(S.mixed_lags(p, rng), 7), (S.mixed_lags(p, rng), 7), (S.mixed_lags(total - 2 * p, rng), 7)], 28)


def _one_of(total):
    rng = np.random.default_rng(29)
    return S.workload([(S.mixed_lags(total, rng), 7)], 29)


def _two_large():
    rng = np.random.default_rng(30)
    return S.workload([(S.mixed_lags(LIMIT + 5, rng), 6), (S.mixed_lags(30, rng), 3), (S.mixed_lags(LIMIT + 100, rng), 4)], 30)


def _small_only():
    rng = np.random.default_rng(31)
    return S.workload([(S.mixed_lags(LIMIT, rng), 6), (S.mixed_lags(65, rng), 3), (np.empty(0, np.int64), 1)], 31)


BUILDERS = {"neighbours": _neighbours, "mixed batch": _mixed_batch, "one run": _one_run, "no ties": _no_ties,
            "extremes": _extremes, "caught up": _caught_up, "straddle": _straddle, "three large": lambda: _three_of(3 * LIMIT + 9),
            "one large": lambda: _one_of(3 * LIMIT + 9), "two large": _two_large, "small only": _small_only}
BUILDERS.update({"shape %d" % p: functools.partial(_shape, p) for p in SHAPE_P})
NAMES = tuple(BUILDERS)
LARGE = tuple(n for n in NAMES if n != "small only")


@functools.lru_cache(maxsize=None)
def case(name):
    """(workload, the oracle's target) of a named case."""
    w = BUILDERS[name]()
    assert w.n_partitions <= 50000
    return w, S.target(w)


def skewed_prev(w, res, seed=3):
    """prev_owner: the topic's lowest rank owned 60 % of everything, the others what they have now: |W| > |S| and |S| > |W|."""
    rng = np.random.default_rng(seed)
    first = np.repeat([int(w.cons_rank[int(w.cons_off[t])]) if w.cons_off[t + 1] > w.cons_off[t] else -1 for t in range(w.n_topics)],
                      np.diff(w.part_off)).astype(np.int32)
    return np.where(rng.random(w.n_partitions) < 0.6, first, res[1]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def prev_of(name, kind="mixed", seed=3):
    w, res = case(name)
    if kind == "skewed":
        return skewed_prev(w, res, seed)
    return S.draw_prev_owner(w, res, seed, kind)


@functools.lru_cache(maxsize=None)
def expected(name, kind="mixed", seed=3):
    """The unlimited yardstick of a named case (computed once)."""
    w, res = case(name)
    return expect(w, res, prev_of(name, kind, seed))


def offsets_case(latest=False, seed=32):
    """S.offsets_case with a large topic: lags from begin / end / committed with some committed < 0, few distinct values."""
    from kafka_lag_based_assignor_amd import synth
    from oracle import oracle
    rng = np.random.default_rng(seed)
    ps, cs = [70, LIMIT + 33, 130], [5, 9, 0]
    n = sum(ps)
    committed = rng.integers(0, 1 << 30, n).astype(np.int64)
    end = committed + rng.integers(0, 4, n) * 10
    begin = end - rng.integers(0, 3, n) * 10
    committed[rng.random(n) < 0.3] = -1
    lag = oracle.compute_lags(begin, end, committed, latest)
    w = S.workload(list(zip(np.split(lag, np.cumsum(ps)[:-1]), cs)), seed)
    return synth.Workload("sticky", w.n_topics, w.part_off, w.partition_id, begin, end, committed, w.lag, w.cons_off, w.cons_rank,
                          w.max_partitions, w.max_consumers)


def groups_of(w, res, prev):
    """Per large topic, what the re-matching sees, in positions of the concatenated list: [(run start, run end, {member: (S, W)})]
    with S / W the ascending position lists of rules 1 and 2."""
    lag = S.lag_at_positions(w, res)
    at = concat_positions(w)
    topic = np.searchsorted(w.part_off, at, side="right") - 1
    runs = []
    q = 0
    while q < at.size:
        z = q + 1
        while z < at.size and topic[z] == topic[q] and lag[at[z]] == lag[at[q]]:
            z += 1
        groups = {}
        for x in range(q, z):
            c, p = int(res[1][at[x]]), int(prev[at[x]])
            if c >= 0:
                groups.setdefault(c, ([], []))[0].append(x)
            if p >= 0:
                groups.setdefault(p, ([], []))[1].append(x)
        runs.append((q, z, groups))
        q = z
    return runs
