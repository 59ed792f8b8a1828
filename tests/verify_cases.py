"""Batches, oracle results and the mutation catalogue for la_verify_assignment_device.  Not a test module: test_verify_cpu.py
(the numpy yardstick against the oracle) and test_verify_gpu.py (the kernel against the yardstick) import it by name, so both
run the same cases.  Oracle results are computed once per batch and shared: treat them as read-only."""
import numpy as np

from kafka_lag_based_assignor_amd import sharding, synth
from oracle import oracle

IDS, ORDER, OWNER, GREEDY, TOTALS, UNCHECKED = (sharding.VERDICT_IDS, sharding.VERDICT_ORDER, sharding.VERDICT_OWNER,
                                                sharding.VERDICT_GREEDY, sharding.VERDICT_TOTALS, sharding.VERDICT_UNCHECKED)
LIMIT = 4096
I32 = np.iinfo(np.int32)

# ---- shapes at which the kernel can go wrong --------------------------------------------------------------------------------
SHAPE_P = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096)


def shapes_of(p):
    """(p, c) for c in {0, 1, 2, 31, 64, 65, p - 1, p, p + 1} within the limit."""
    cs = sorted({c for c in (0, 1, 2, 31, 64, 65, p - 1, p, p + 1) if 0 <= c <= LIMIT})
    return [(p, c) for c in cs]


ROUND_SHAPES = [(k * c + extra, c) for c in (3, 32, 100) for k in (1, 4) for extra in (0, 1, c - 1)]      # P = kC, kC + 1, kC + C - 1
CATALOGUE_SHAPES = ((256, 32), (1000, 7), (5, 9), (4096, 4096))


def batch(shapes, seed, lags="mixed", ids="shuffled", first_rank=0):
    """A batch of topics with the given (partitions, consumers) shapes: distinct ids per topic, ascending ranks with gaps (every
    topic draws from the same rank space, so topics share some members and not others).
    lags: mixed (half drawn from seven values: ties; half below 2^40) | equal | zero | wrap | negative
    ids:  shuffled (a permutation of 0 .. P-1) | full (any int32, the corners included) | 4096 | 2^20 (strided)"""
    rng = np.random.default_rng(seed)
    ps, cs = [s[0] for s in shapes], [s[1] for s in shapes]
    part_off = np.concatenate([[0], np.cumsum(ps)]).astype(np.int64)
    cons_off = np.concatenate([[0], np.cumsum(cs)]).astype(np.int64)
    pid, lag, ranks = [], [], []
    for t, (p, c) in enumerate(shapes):
        if ids == "shuffled":
            i = rng.permutation(p)
        elif ids == "full":
            s = set([I32.min, -1, 0, I32.max, -4096, 1 << 20][:p])
            while len(s) < p:
                s.update(rng.integers(I32.min, I32.max, p - len(s), endpoint=True).tolist())
            i = rng.permutation(np.array(sorted(s), np.int64))
        else:
            i = (rng.permutation(p) - p // 2) * {"4096": 4096, "2^20": 1 << 20}[ids]
            assert p == 0 or (I32.min <= i.min() and i.max() <= I32.max)
        pid.append(i)
        if lags == "mixed":
            l = np.where(rng.random(p) < 0.5, rng.integers(0, 7, p) * 1000, rng.integers(0, 1 << 40, p))
        elif lags == "equal":
            l = np.full(p, 12345)
        elif lags == "zero":
            l = np.zeros(p, np.int64)
        elif lags == "wrap":                # totals wrap after two entries: the signed compare of wrapped totals decides
            l = np.array([(1 << 63) - 1, 1 << 62, -(1 << 62), (1 << 62) + 1], np.int64)[rng.integers(0, 4, p)]
        elif lags == "negative":
            l = rng.integers(-(1 << 63), (1 << 63) - 1, p)
        else:
            raise ValueError(lags)
        lag.append(np.asarray(l, np.int64))
        ranks.append(np.sort(rng.choice(3 * c + 5, c, replace=False)) + first_rank)
    cat = lambda xs, dt: np.concatenate(xs + [np.empty(0, np.int64)]).astype(dt)
    n = int(part_off[-1])
    lag = cat(lag, np.int64)
    return synth.Workload("verify", len(shapes), part_off, cat(pid, np.int32), np.zeros(n, np.int64), lag.copy(), np.zeros(n, np.int64),
                          lag, cons_off, cat(ranks, np.int32), max(ps) if ps else 0, max(cs) if cs else 0)


_results = {}


def oracle_result(w, lag=None):
    """(out_partition, out_member_rank, out_total_lag) of the oracle for `w` (keyed by the object: computed once)."""
    key = id(w)
    if lag is None and key in _results and _results[key][0] is w:
        return _results[key][1]
    res = oracle.assign_flat(w.part_off, w.partition_id, w.lag if lag is None else lag, w.cons_off, w.cons_rank)
    for a in res:
        a.setflags(write=False)
    if lag is None:
        _results[key] = (w, res)
    return res


def yardstick(w, res, **kw):
    """sharding.verify_assignment_numpy on `w` and the results `res`; lags: w.lag unless offsets are given (end=...)."""
    if "lag" not in kw and "end" not in kw:
        kw["lag"] = w.lag
    return sharding.verify_assignment_numpy(w.part_off, w.partition_id, w.cons_off, w.cons_rank, res[0], res[1], res[2], **kw)


def differing_topics(w, res, exp):
    """Topics whose (partition, member, totals) triple differs from the oracle's."""
    out = []
    for t in range(w.n_topics):
        a, z, ca, cz = int(w.part_off[t]), int(w.part_off[t + 1]), int(w.cons_off[t]), int(w.cons_off[t + 1])
        if not (np.array_equal(res[0][a:z], exp[0][a:z]) and np.array_equal(res[1][a:z], exp[1][a:z]) and
                np.array_equal(res[2][ca:cz], exp[2][ca:cz])):
            out.append(t)
    return out


# ---- the mutation catalogue: one fault in one topic ----------------------------------------------------------------------------
CATALOGUE = {
    "swap neighbours, different lags": ORDER,
    "swap neighbours, equal lags": ORDER,
    "foreign id": IDS,
    "repeated id": IDS,
    "swap owners inside a round": GREEDY,
    "swap owners inside a round, totals tie": GREEDY,
    "owner of the neighbour in the round": OWNER,
    "rank that subscribes elsewhere": OWNER,
    "-1 in a topic with consumers": OWNER,
    "rank in a topic without consumers": OWNER,
    "partial last round: an unpicked consumer for the last picked": GREEDY,
    "owner one round early": OWNER | GREEDY,
    "total + 1": TOTALS,
    "total + 2^63": TOTALS,
}


def mutate(name, w, exp, t):
    """The oracle's result `exp` with the fault `name` in topic t -> (out_partition, out_member_rank, out_total_lag), or None
    when topic t has no place for that fault (too few partitions, no partial round, ...)."""
    a, z, ca, cz = int(w.part_off[t]), int(w.part_off[t + 1]), int(w.cons_off[t]), int(w.cons_off[t + 1])
    p, c = z - a, cz - ca
    op, om, ot = exp[0].copy(), exp[1].copy(), exp[2].copy()
    ids = w.partition_id[a:z]
    by_id = np.argsort(ids, kind="stable")
    l = w.lag[a:z][by_id[np.searchsorted(ids[by_id], op[a:z])]] if p else np.empty(0, np.int64)      # lags in assignment order
    rnd = np.arange(p) // max(c, 1)
    same_round = (rnd[:-1] == rnd[1:]) if (p > 1 and c > 0) else np.zeros(max(p - 1, 0), bool)

    def first(mask):
        hits = np.flatnonzero(mask)
        return None if hits.size == 0 else int(hits[0])

    if name.startswith("swap neighbours"):
        i = first(l[:-1] != l[1:]) if "different" in name else first(l[:-1] == l[1:])
        if i is None:
            return None
        if "different" in name:
            op[[a + i, a + i + 1]] = op[[a + i + 1, a + i]]
            om[[a + i, a + i + 1]] = om[[a + i + 1, a + i]]
        else:
            op[[a + i, a + i + 1]] = op[[a + i + 1, a + i]]
    elif name == "foreign id":
        if p == 0:
            return None
        op[a + p // 2] = int(ids.max()) + 1 if int(ids.max()) < I32.max else int(ids.min()) - 1
    elif name == "repeated id":
        if p < 2:
            return None
        op[a + p // 2] = op[a + p // 2 - 1]
    elif name.startswith("swap owners inside a round"):
        if c < 2 or p < 2:
            return None
        before = _before(om[a:z], w.cons_rank[ca:cz], l)
        tie = before[:-1] == before[1:]
        i = first(same_round & (tie if "tie" in name else ~tie))
        if i is None:
            return None
        om[[a + i, a + i + 1]] = om[[a + i + 1, a + i]]
    elif name == "owner of the neighbour in the round":
        i = first(same_round)
        if i is None:
            return None
        om[a + i] = om[a + i + 1]
    elif name == "rank that subscribes elsewhere":
        others = np.setdiff1d(w.cons_rank, w.cons_rank[ca:cz])
        if c == 0 or p == 0 or others.size == 0:
            return None
        om[a + p // 2] = others[others.size // 2]
    elif name == "-1 in a topic with consumers":
        if c == 0 or p == 0:
            return None
        om[a + p // 2] = -1
    elif name == "rank in a topic without consumers":
        if c != 0 or p == 0 or w.cons_rank.size == 0:
            return None
        om[a + p // 2] = w.cons_rank[0]
    elif name.startswith("partial last round"):
        if c == 0 or p % c == 0:
            return None
        unpicked = np.setdiff1d(w.cons_rank[ca:cz], om[a + (p // c) * c:z])
        om[z - 1] = unpicked[0]
    elif name == "owner one round early":
        if c < 2 or p <= c:
            return None
        i = c                                                      # the first entry of round 1: its owner also takes ...
        j = first(om[a:a + c] != om[a + i])                        # ... an entry of round 0 that was another consumer's
        om[a + j] = om[a + i]
    elif name == "total + 1":
        if c == 0:
            return None
        ot[ca + c // 2] += 1
    elif name == "total + 2^63":
        if c == 0:
            return None
        ot[ca + c // 2] ^= np.int64(-(1 << 63))
    else:
        raise ValueError(name)
    return op, om, ot


def _before(owners, ranks, l):
    """Every entry's owner's wrapping total over the entries before it (the oracle's owners: one per round)."""
    k = np.searchsorted(ranks, owners)
    tot = np.zeros(ranks.size, np.uint64)
    out = np.empty(l.size, np.uint64)
    lu = np.ascontiguousarray(l).view(np.uint64)
    with np.errstate(over="ignore"):
        for i in range(l.size):
            out[i] = tot[k[i]]
            tot[k[i]] += lu[i]
    return out.view(np.int64)


def catalogue_batch(shape, seed=5):
    """[(64, 8), shape, (40, 0), (30, 5)]: the faults go into topic 1 (topic 2 for the one that needs a topic without consumers)."""
    return batch([(64, 8), shape, (40, 0), (30, 5)], seed)


def catalogue_cases(w, exp):
    """(name, topic, mutated result) for every catalogue entry that has a place in `w`."""
    out = []
    for name in CATALOGUE:
        t = 2 if name == "rank in a topic without consumers" else 1
        res = mutate(name, w, exp, t)
        if res is not None:
            out.append((name, t, res))
    return out
