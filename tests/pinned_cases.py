"""Cases of la_assign_pinned_device shared by tests/test_pinned_cpu.py, tests/test_pinned_gpu.py and
tests/test_assign_coop_pinned_gpu.py: a table of the smallest shapes at which the kernel can go wrong, seeded draws, the settling
scenario and a dictionary model written independently of sharding.assign_pinned_numpy (no heap, no shared helper: an argmin
over numpy bins per free partition).  Not a test module."""
import numpy as np

from kafka_lag_based_assignor_amd import sharding

from coop_cases import owned_arrays

I64 = np.iinfo(np.int64)
OUTPUTS = ("out_partition", "out_member_rank", "totals", "topic_free", "summary")
MAX_P, MAX_C = 4096, 2048               # LA_PINNED_MAX_PARTITIONS / LA_PINNED_MAX_CONSUMERS


class PinnedCase:
    """A batch in lags form and the owned lists, on the host."""

    def __init__(self, topics, m, claims, head=0, tail=0, seed=0):
        """topics: [(ids, lags, ranks), ...]; claims: [(member, topic, id), ...] (topic -1: unmapped)."""
        ps, cs = [len(t[0]) for t in topics], [len(t[2]) for t in topics]
        cat = lambda xs, dt: np.concatenate([np.asarray(x, np.int64) for x in xs] + [np.empty(0, np.int64)]).astype(dt)
        self.part_off = np.concatenate([[0], np.cumsum(ps)]).astype(np.int64)
        self.cons_off = np.concatenate([[0], np.cumsum(cs)]).astype(np.int64)
        self.pid, self.lag = cat([t[0] for t in topics], np.int32), cat([t[1] for t in topics], np.int64)
        self.cons_rank = cat([t[2] for t in topics], np.int32)
        self.m = int(m)
        self.owned_off, self.owned_topic, self.owned_pid = owned_arrays(self.m, claims, head, tail, seed)
        self.t, self.n, self.k, self.n_owned = len(topics), self.pid.size, self.cons_rank.size, self.owned_topic.size

    def args(self):
        return (self.part_off, self.pid, self.lag, self.cons_off, self.cons_rank, self.m, self.owned_off, self.owned_topic,
                self.owned_pid)

    def expect(self, strict=True):
        return sharding.assign_pinned_numpy(*self.args(), strict=strict)

    def over_limit(self):
        """Per topic: over LA_PINNED_MAX_PARTITIONS or LA_PINNED_MAX_CONSUMERS."""
        return (np.diff(self.part_off) > MAX_P) | (np.diff(self.cons_off) > MAX_C)


def topic(rng, p, ranks, lags="u20", ids="shuffled"):
    """(ids, lags, ranks) of one topic."""
    if ids == "shuffled":
        i = rng.permutation(p)
    elif ids == "negative":
        i = -1 - rng.permutation(p) * 3
    else:
        assert ids == "spread", ids
        i = rng.choice(np.arange(-(1 << 31), 1 << 31, 1 << 12), p, replace=False) + rng.integers(0, 1 << 12, p)
    if isinstance(lags, str):
        lags = {"u20": lambda: rng.integers(0, 1 << 20, p), "ties": lambda: rng.integers(0, 4, p) * 1000,
                "zero": lambda: np.zeros(p, np.int64), "full": lambda: rng.integers(I64.min, I64.max, p, endpoint=True),
                "huge": lambda: I64.max - rng.integers(0, 5, p)}[lags]()
    return np.asarray(i, np.int64), np.asarray(lags, np.int64), np.asarray(sorted(ranks), np.int64)


def owners(rng, topics, m, owned=0.7, foreign=0.0):
    """Claims over the topics: every partition is owned with probability `owned`, by one of its topic's consumers -- or, with
    probability `foreign`, by any member (which may consume the topic or not)."""
    claims = []
    for t, (ids, _, ranks) in enumerate(topics):
        for i in ids.tolist():
            if rng.random() >= owned or m == 0:
                continue
            if ranks.size == 0 or rng.random() < foreign:
                claims.append((int(rng.integers(0, m)), t, i))
            else:
                claims.append((int(rng.choice(ranks)), t, i))
    return claims


def drawn(seed, shapes, m, lags="u20", ids="shuffled", owned=0.7, foreign=0.1, n_stale=0, n_unmapped=0, head=0, tail=0):
    """A case drawn from `seed`: topics of the given (partitions, consumers) shapes over m members."""
    rng = np.random.default_rng(seed)
    topics = [topic(rng, p, rng.choice(m, c, replace=False) if c else [], lags, ids) for p, c in shapes]
    claims = owners(rng, topics, m, owned, foreign)
    have = {(t, i) for _, t, i in claims} | {(t, int(i)) for t, tp in enumerate(topics) for i in tp[0]}
    while n_stale > 0 and topics and m:
        key = (int(rng.integers(0, len(topics))), int(rng.integers(-(1 << 31), 1 << 31)))
        if key not in have:
            have.add(key)
            claims.append((int(rng.integers(0, m)), key[0], key[1]))
            n_stale -= 1
    claims += [(int(rng.integers(0, m)), -1, k // 2) for k in range(n_unmapped if m else 0)]
    return PinnedCase(topics, m, claims, head, tail, seed + 1)


def _worked():
    t = (np.arange(6), np.array([50, 40, 30, 20, 10, 5]), np.array([0, 1, 2]))
    return PinnedCase([t], 3, [(0, 0, 0), (0, 0, 1), (1, 0, 2)])


def _catch_up():
    # consumer 0 holds nothing, the seven others 40 each; 60 free partitions: 40 levels of one, then levels of eight
    rng = np.random.default_rng(15)
    t = topic(rng, 7 * 40 + 60, range(8), "u20")
    claims = [(1 + j // 40, 0, int(i)) for j, i in enumerate(t[0][:280])]
    return PinnedCase([t], 8, claims)


def _few_free():
    # twelve consumers level at 3, five free partitions: fewer than the consumers of the minimal level
    rng = np.random.default_rng(16)
    t = topic(rng, 41, range(2, 14), "u20")
    claims = [(2 + j % 12, 0, int(i)) for j, i in enumerate(t[0][:36])]
    return PinnedCase([t], 14, claims)


def _same_id_two_topics():
    rng = np.random.default_rng(11)
    a, b = topic(rng, 9, [0, 1, 2]), topic(rng, 9, [0, 1, 2])
    claims = [(0, 0, i) for i in range(0, 9, 2)] + [(1, 1, i) for i in range(0, 9, 2)] + [(2, 1, 1)]
    return PinnedCase([a, b], 3, claims)


def _rank_ties():
    # all lags 0 and nothing owned by most: (count, total) tie everywhere, the lowest rank takes each turn
    rng = np.random.default_rng(13)
    t = topic(rng, 23, [3, 5, 9, 10], "zero")
    return PinnedCase([t], 11, [(9, 0, int(t[0][0])), (5, 0, int(t[0][1]))])


def _wrapping():
    # totals wrap: lags next to INT64_MAX and any int64, negative ones among them
    rng = np.random.default_rng(14)
    a, b = topic(rng, 40, [0, 1, 2], "huge"), topic(rng, 77, [1, 2, 3, 4], "full", "spread")
    return PinnedCase([a, b], 5, owners(rng, [a, b], 5, 0.5, 0.0))


def _foreign():
    # member 1 consumes topic 1 only and claims partitions of topic 0, whose ranks lie on both sides of it
    rng = np.random.default_rng(8)
    a, b = topic(rng, 12, [0, 2, 3]), topic(rng, 5, [1])
    claims = [(1, 0, 0), (1, 0, 5), (2, 0, 7), (0, 0, 3), (1, 1, 2)]
    return PinnedCase([a, b], 4, claims)


def _above():
    # the claimant's rank lies above every consumer of the topic (the bisection ends on the last one)
    rng = np.random.default_rng(9)
    a = topic(rng, 10, [0, 1])
    return PinnedCase([a, topic(rng, 3, [4])], 5, [(4, 0, 2), (4, 0, 9), (1, 0, 4)])


def _unmapped_and_outside():
    return drawn(10, [(30, 3), (0, 2), (17, 4)], 6, n_stale=7, n_unmapped=5, head=4, tail=3)


def _everything_owned():
    rng = np.random.default_rng(6)
    topics = [topic(rng, 50, [0, 1, 2, 3], "ties"), topic(rng, 1, [2]), topic(rng, 129, range(5), "full")]
    return PinnedCase(topics, 5, owners(rng, topics, 5, 1.0, 0.0))


def _limit():
    rng = np.random.default_rng(18)
    t = topic(rng, MAX_P, range(MAX_C), "u20", "spread")
    return PinnedCase([t, topic(rng, 9, [5, 7])], MAX_C, owners(rng, [t], MAX_C, 0.5, 0.0))


CASES = {
    "P = 0": lambda: PinnedCase([topic(np.random.default_rng(1), 0, [0, 1, 2]), topic(np.random.default_rng(1), 4, [1])], 3, [(1, 1, 2), (0, 0, 0)]),
    "C = 0 with claims": lambda: PinnedCase([topic(np.random.default_rng(2), 4, []), topic(np.random.default_rng(2), 3, [0, 1])], 2,
                                            [(0, 0, 1), (1, 0, 3), (1, 1, 0)]),
    "C = 1": lambda: drawn(3, [(5, 1), (64, 1)], 3, owned=0.5, foreign=0.5),
    "P = 1": lambda: PinnedCase([topic(np.random.default_rng(4), 1, [0, 1]), topic(np.random.default_rng(4), 1, [0, 1])], 2, [(1, 1, 0)]),
    "nothing owned": lambda: drawn(5, [(40, 3), (0, 0), (65, 7), (7, 9)], 9, lags="ties", owned=0.0),
    "everything owned": _everything_owned,
    "the worked case": _worked,
    "a foreign claimant": _foreign,
    "a claimant above every consumer": _above,
    "topic -1 and entries outside the offsets": _unmapped_and_outside,
    "one id, two topics, two members": _same_id_two_topics,
    "equal lags: the id decides": lambda: drawn(12, [(33, 4), (70, 3)], 5, lags="ties", ids="negative"),
    "ties in (count, total): the rank decides": _rank_ties,
    "negative lags, totals that wrap": _wrapping,
    "one consumer at 0, the others at 40": _catch_up,
    "fewer free partitions than consumers at the level": _few_free,
    "64 and 65 consumers": lambda: drawn(17, [(200, 64), (200, 65)], 70, owned=0.6),
    "1024 and 1025 partitions": lambda: drawn(19, [(1024, 5), (1025, 70)], 80, lags="ties", owned=0.8, n_stale=3),
    "4096 x 2048: the limit": _limit,
}

# a topic over a limit next to a small one that must still be exact: LA_ESHAPE, the large topic untouched
OVER = {
    "4097 partitions": lambda: drawn(20, [(21, 3), (MAX_P + 1, 4), (9, 2)], 6, owned=0.5),
    "2049 consumers": lambda: drawn(21, [(MAX_C + 1, MAX_C + 1), (30, 4)], MAX_C + 1, owned=0.3),
}


def broken(bad):
    """A small case with one thing wrong -> (case, the topics that must still be exact)."""
    c = drawn(30, [(20, 3), (31, 4), (12, 2)], 6, owned=0.8, foreign=0.2)
    lo, hi = int(c.owned_off[0]), int(c.owned_off[-1])
    if bad == "unsorted ranks":
        c0 = int(c.cons_off[1])
        c.cons_rank[c0], c.cons_rank[c0 + 1] = c.cons_rank[c0 + 1], c.cons_rank[c0]
        return c, [0, 2]
    if bad == "equal ranks":
        c0 = int(c.cons_off[1])
        c.cons_rank[c0 + 1] = c.cons_rank[c0]
        return c, [0, 2]
    if bad == "owned topic T":
        c.owned_topic[lo + 1] = c.t
    elif bad == "owned topic -2":
        c.owned_topic[lo + 1] = -2
    elif bad == "claimed twice":
        c.owned_topic[hi - 1], c.owned_pid[hi - 1] = c.owned_topic[lo], c.owned_pid[lo]
    elif bad == "descending owned offsets":
        c.owned_off[1], c.owned_off[2] = c.owned_off[2] + 1, c.owned_off[1]
    elif bad == "owned offset beyond n_owned":
        c.owned_off[-1] = c.n_owned + 1
    else:
        raise ValueError(bad)
    return c, []


BROKEN = {"unsorted ranks": "LA_EINVAL", "equal ranks": "LA_EINVAL", "owned topic T": "LA_EINVAL", "owned topic -2": "LA_EINVAL",
          "claimed twice": "LA_EINVAL", "descending owned offsets": "LA_ESHAPE", "owned offset beyond n_owned": "LA_ESHAPE"}


def dict_model(c):
    """The five rules with a Python dict from (topic, id) to member and numpy bins -> the five outputs, or ValueError for what
    the device reports."""
    off = c.owned_off.tolist()
    if any(b < a for a, b in zip(off, off[1:])) or off[0] < 0 or off[-1] > c.n_owned:
        raise ValueError("owned offsets")
    claimed, looked_at = {}, 0
    for r in range(c.m):
        for j in range(off[r], off[r + 1]):
            looked_at += 1
            t, i = int(c.owned_topic[j]), int(c.owned_pid[j])
            if t == -1:
                continue
            if t < -1 or t >= c.t:
                raise ValueError("owned topic")
            if (t, i) in claimed:
                raise ValueError("claimed twice")
            claimed[(t, i)] = r
    out_pid, out_rank = np.empty(c.n, np.int32), np.empty(c.n, np.int32)
    totals, topic_free = np.empty(c.k, np.int64), np.zeros(c.t, np.int64)
    pinned = free = foreign = hits = 0
    for t in range(c.t):
        p0, p1, c0, c1 = (int(x) for x in (c.part_off[t], c.part_off[t + 1], c.cons_off[t], c.cons_off[t + 1]))
        ranks = c.cons_rank[c0:c1].astype(np.int64)
        if (np.diff(ranks) <= 0).any():
            raise ValueError("ranks")
        if p1 - p0 > MAX_P or c1 - c0 > MAX_C:
            raise ValueError("limits")
        count, total = np.zeros(ranks.size, np.int64), np.zeros(ranks.size, np.int64)
        parts = sorted(((-int(c.lag[j]), int(c.pid[j])) for j in range(p0, p1)))      # lag descending, id ascending
        q = [claimed.get((t, i), -1) for _, i in parts]
        where = {int(r): k for k, r in enumerate(ranks)}
        with np.errstate(over="ignore"):
            for (neg, _), who in zip(parts, q):                                       # seed: every pinned partition first
                if who in where:
                    count[where[who]] += 1
                    total[where[who]] += np.int64(-neg)
            for pos, ((neg, i), who) in enumerate(zip(parts, q)):
                out_pid[p0 + pos] = i
                hits += who >= 0
                if who in where:
                    pinned += 1
                    out_rank[p0 + pos] = who
                    continue
                free += 1
                foreign += who >= 0
                topic_free[t] += 1
                if ranks.size == 0:
                    out_rank[p0 + pos] = -1
                    continue
                least = np.flatnonzero(count == count.min())
                k = int(least[np.flatnonzero(total[least] == total[least].min())[0]])      # ranks ascend: the first is the lowest
                out_rank[p0 + pos] = ranks[k]
                count[k] += 1
                total[k] += np.int64(-neg)
        totals[c0:c1] = total
    return out_pid, out_rank, totals, topic_free, np.array([pinned, free, foreign, looked_at - hits], np.int64)


def same(got, exp, what=""):
    for k, g, e in zip(OUTPUTS, got, exp):
        np.testing.assert_array_equal(g, e, err_msg="%s %s" % (k, what))


# ---- the settling scenario: a lagging group whose offsets move between two rebalances ---------------------------------------------
class Scenario:
    """T topics x P partitions x C consumers (every member consumes every topic), lags uniform in [0, 100 000) that grow by
    uniform [0, 2 000) between two rebalances; every member obeys each adjusted assignment."""

    def __init__(self, seed, t, p, c):
        self.rng = np.random.default_rng(seed)
        self.t, self.p, self.m = t, p, c
        self.part_off = np.arange(t + 1, dtype=np.int64) * p
        self.cons_off = np.arange(t + 1, dtype=np.int64) * c
        self.pid = np.tile(np.arange(p, dtype=np.int32), t)
        self.cons_rank = np.tile(np.arange(c, dtype=np.int32), t)
        self.lag = self.rng.integers(0, 100000, t * p).astype(np.int64)
        self.owned = (np.zeros(c + 1, np.int64), np.empty(0, np.int32), np.empty(0, np.int32))

    def grow(self):
        self.lag = self.lag + self.rng.integers(0, 2000, self.lag.size)

    def inputs(self):
        return (self.part_off, self.pid, self.lag, self.cons_off, self.cons_rank, self.m) + self.owned

    def obey(self, out_partition, coop_member_rank):
        self.owned = sharding.owned_after_round(self.part_off, out_partition, coop_member_rank, self.m)
