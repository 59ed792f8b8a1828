"""Cases of la_cooperative_round_sticky_device shared by tests/test_coop_sticky_cpu.py and tests/test_coop_sticky_gpu.py: a
target and owned lists (coop_cases), the batch's inputs in an order of their own with lags whose runs are chosen per case
(the lag makers of sticky_cases), and a dictionary model of the whole call.  Cases are built once and shared: treat them as
read-only.  Not a test module."""
import functools

import numpy as np

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding
from oracle import oracle

import coop_cases as C
import sticky_cases as S

I32, I64 = np.iinfo(np.int32), np.iinfo(np.int64)
LE, LO, LM, LT = N.COOP_STICKY_ENTRIES, N.COOP_STICKY_OWNED, N.COOP_STICKY_MEMBERS, N.COOP_STICKY_TOPICS
TOPIC_LIMIT = sharding.STICKY_MAX_PARTITIONS
STICKY = ("sticky", "topic_kept", "topic_saved", "sticky_summary")
ROUND = C.OUTPUTS + ("member_off", "grouped_topic", "grouped_partition")
ALL = STICKY + ROUND


class StickyCase:
    """A CoopCase (the target, in `coop`) and the batch it came from: partition_id / lag in INPUT order, optionally the offsets
    the lags come from (then `latest` says how), the batch's hint."""

    def __init__(self, coop, partition_id, lag, hint=None, offsets=None, latest=True):
        self.coop = coop
        self.partition_id = np.ascontiguousarray(partition_id, np.int32)
        self.lag = np.ascontiguousarray(lag, np.int64)
        sizes = np.diff(coop.part_off)
        self.hint = int(hint if hint is not None else (sizes.max() if sizes.size else 0))
        self.offsets, self.latest = offsets, latest

    @property
    def cap(self):
        """Partitions of a topic the device re-matches: the hint, or the limit where the hint is not usable."""
        return self.hint if 0 < self.hint <= TOPIC_LIMIT else TOPIC_LIMIT

    @property
    def small(self):
        c = self.coop
        return c.n <= LE and c.n_owned <= LO and c.m <= LM and c.t <= LT

    def expect(self):
        c = self.coop
        return sharding.cooperative_round_sticky_numpy(c.part_off, self.partition_id, self.lag, c.pid, c.rank, c.m, c.owned_off,
                                                       c.owned_topic, c.owned_pid, max_partitions=self.cap)

    def plain_round(self):
        c = self.coop
        return sharding.cooperative_round_numpy(c.part_off, c.pid, c.rank, c.m, c.owned_off, c.owned_topic, c.owned_pid)

    def copy(self):
        off = None if self.offsets is None else tuple(a.copy() for a in self.offsets)
        return StickyCase(self.coop.copy(), self.partition_id.copy(), self.lag.copy(), self.hint, off, self.latest)


def with_lags(coop, lag_at_position, seed, **kw):
    """The batch behind a target: the input order of every topic is a shuffle of the target's, every partition keeps its lag."""
    rng = np.random.default_rng(seed)
    lag_at_position = np.asarray(lag_at_position, np.int64)
    assert lag_at_position.size == coop.n
    order = np.concatenate([coop.part_off[t] + rng.permutation(int(p)) for t, p in enumerate(np.diff(coop.part_off))] +
                           [np.empty(0, np.int64)]).astype(np.int64)
    return StickyCase(coop, coop.pid[order], lag_at_position[order], **kw)


def descending(lags_per_topic):
    """Per topic the lags in the order an assignment has them: descending, equal lags side by side."""
    return np.concatenate([np.sort(np.asarray(l, np.int64))[::-1] for l in lags_per_topic] + [np.empty(0, np.int64)])


def drawn(seed, sizes, m, maker, ids="shuffled", hint=None, **owned):
    """coop_cases.synthetic with lags from `maker(p, rng)` per topic, in descending order."""
    rng = np.random.default_rng(seed + 100)
    coop = C.synthetic(seed, sizes, m, ids, **owned)
    return with_lags(coop, descending([maker(int(p), rng) for p in sizes]), seed + 200, hint=hint)


caught_up = lambda p, rng: S.caught_up_lags(p, 0.05, rng)
mixed = lambda p, rng: S.mixed_lags(p, rng)
zeros = lambda p, rng: np.zeros(p, np.int64)


def explicit(sizes, pid, rank, m, claims, lag_at_position, seed=0, **kw):
    part_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    coop = C.CoopCase(part_off, np.asarray(pid, np.int32), np.asarray(rank, np.int32), m, *C.owned_arrays(m, claims, seed=seed))
    return with_lags(coop, lag_at_position, seed + 1, **kw)


def _adjacent_equal_topics():
    """Two topics of six, every lag 0.  In topic 0 member 0 has two places and owned four of its partitions before, in topic 1 it
    has four places and owned two; member 1 the other way round.  One run per topic: each topic is re-matched inside itself.  One
    run over both would carry member 0's two surplus partitions of topic 0 over to its places in topic 1."""
    pid = [10, 11, 12, 13, 14, 15, 10, 11, 12, 13, 14, 15]
    rank = [0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1]
    claims = [(1, 0, 10), (1, 0, 11), (0, 0, 12), (0, 0, 13), (0, 0, 14), (0, 0, 15),
              (1, 1, 10), (1, 1, 11), (1, 1, 12), (1, 1, 13), (0, 1, 14), (0, 1, 15)]
    return explicit([6, 6], pid, rank, 2, claims, np.zeros(12, np.int64), 3)


def _run_starts_at_last_position():
    """Topic 0 ends with the first position of the lag-0 value; topic 1 is all 0.  The run that starts at position 3 has length
    one: the topic ends there."""
    pid = [1, 2, 3, 4, 1, 2, 3, 4]
    rank = [0, 1, 0, 1, 1, 0, 1, 0]
    claims = [(0, 0, 4), (1, 0, 3), (0, 1, 1), (0, 1, 3), (1, 1, 2), (1, 1, 4)]
    return explicit([4, 4], pid, rank, 2, claims, [9, 5, 3, 0, 0, 0, 0, 0], 5)


def _no_consumers_between():
    rng = np.random.default_rng(7)
    coop = C.synthetic(7, [40, 30, 50], 4, owned_frac=0.9)
    coop.rank[40:70] = -1
    coop.rank[:40] = rng.integers(0, 4, 40)
    coop.rank[70:] = rng.integers(0, 4, 50)
    return with_lags(coop, descending([S.caught_up_lags(p, 0.1, rng) for p in (40, 30, 50)]), 8)


def _foreign_previous_owner():
    """One run of six owned today by members 0 and 1; member 2 owned two of its partitions before and owns nothing in the run
    (it owns the single partition of the second run): those two match nobody and fill what is left over."""
    pid = [5, 6, 7, 8, 9, 10, 11]
    rank = [0, 1, 0, 1, 0, 1, 2]
    claims = [(2, 0, 5), (2, 0, 6), (1, 0, 7), (0, 0, 8), (0, 0, 10), (1, 0, 11)]
    return explicit([7], pid, rank, 3, claims, [4, 4, 4, 4, 4, 4, 1], 9)


def _extreme_lags():
    """Negative lags (what la_assign_batch_lags accepts) and the ends of int64 side by side, each value twice."""
    vals = [I64.max, I64.max, I64.max - 1, I64.max - 1, 1, 1, 0, 0, -1, -1, -7, -7, I64.min + 1, I64.min + 1, I64.min, I64.min]
    coop = C.synthetic(11, [16, 16], 3, owned_frac=1.0)
    return with_lags(coop, np.array(vals + vals, np.int64), 12)


def _offsets(latest):
    """Lags from begin / end / committed with partitions that have no committed offset; four values of end - committed."""
    rng = np.random.default_rng(13)
    sizes = [70, 1, 130, 0, 56]
    coop = C.synthetic(13, sizes, 5, owned_frac=0.9, n_stale=3)
    n = coop.n
    committed = rng.integers(0, 1 << 30, n).astype(np.int64)
    end = committed + rng.integers(0, 4, n) * 10
    begin = end - rng.integers(0, 3, n) * 10
    committed[rng.random(n) < 0.3] = -1
    lag = oracle.compute_lags(begin, end, committed, latest)
    # the target's order: per topic by lag descending (the offsets travel with their partition)
    by = np.concatenate([coop.part_off[t] + np.argsort(-lag[coop.part_off[t]:coop.part_off[t + 1]], kind="stable")
                         for t in range(coop.t)]).astype(np.int64)
    begin, end, committed, lag = begin[by], end[by], committed[by], lag[by]
    rng2 = np.random.default_rng(14)
    order = np.concatenate([coop.part_off[t] + rng2.permutation(int(p)) for t, p in enumerate(sizes)]).astype(np.int64)
    return StickyCase(coop, coop.pid[order], lag[order], offsets=(begin[order], end[order], committed[order]), latest=latest)


def _limit(which, over):
    if which == "N":
        return drawn(30, [(LE + over) // 4 + (LE + over) % 4, 0, (LE + over) // 4, (LE + over) // 4, (LE + over) // 4], 5, caught_up,
                     owned_frac=0.5, head=1)
    if which == "n_owned":
        k = drawn(31, [700, 0, 800], 6, caught_up, ids="negative", owned_frac=1.0, n_stale=LO + over - 1500)
        assert k.coop.n_owned == LO + over
        return k
    if which == "M":
        return drawn(32, [300, 0, 299, 1], LM + over, mixed, owned_frac=0.7, n_unmapped=3, tail=2)
    assert which == "T"
    return drawn(33, [1] * 100 + [0] * (LT + over - 101) + [5], 4, zeros, owned_frac=0.8)


def _ids(kind):
    if kind == "descending":
        coop = C.synthetic(40, [90, 33, 64], 5, owned_frac=0.9, n_stale=4)
        for t in range(coop.t):                                     # the target's ids descend inside every topic; claims follow the ids
            a, z = int(coop.part_off[t]), int(coop.part_off[t + 1])
            coop.pid[a:z] = np.arange(z - a, 0, -1) * 3
        claims = C.claims_from(41, coop.part_off, coop.pid, coop.m, owned_frac=0.9)
        coop = C.CoopCase(coop.part_off, coop.pid, coop.rank, coop.m, *C.owned_arrays(coop.m, claims, seed=42))
        rng = np.random.default_rng(43)
        return with_lags(coop, descending([S.caught_up_lags(p, 0.05, rng) for p in (90, 33, 64)]), 44)
    return drawn(45, [12, 70, 0, 65, 9], 6, caught_up, ids={"shuffled": "shuffled", "hostile": "full"}[kind], owned_frac=0.9, n_stale=5,
                 n_unmapped=2, head=1, tail=1)


@functools.lru_cache(maxsize=None)
def case(name):
    e32 = np.empty(0, np.int32)
    if name == "no topics":
        return StickyCase(C.CoopCase(np.zeros(1, np.int64), e32, e32, 3, *C.owned_arrays(3, [(0, -1, 4)])), e32, np.empty(0, np.int64))
    if name == "no entries":
        return StickyCase(C.CoopCase(np.zeros(4, np.int64), e32, e32, 3, *C.owned_arrays(3, [(0, -1, 4), (1, 2, 9)], 1, 1)), e32,
                          np.empty(0, np.int64))
    if name == "nothing owned":
        return drawn(1, [40, 0, 7, 64, 30], 6, zeros, owned_frac=0.0)
    if name == "one partition":
        return drawn(2, [1], 1, zeros, owned_frac=1.0)
    if name == "adjacent topics, all lags 0":
        return _adjacent_equal_topics()
    if name == "equal lag across topics of 63, 64, 65":
        return drawn(3, [63, 64, 65], 5, lambda p, rng: np.full(p, 7, np.int64), owned_frac=0.9)
    if name == "run starts at a topic's last position":
        return _run_starts_at_last_position()
    if name == "topic without consumers between two":
        return _no_consumers_between()
    if name == "previous owner owns nothing in the run":
        return _foreign_previous_owner()
    if name == "stale, unmapped, head and tail claims":
        return drawn(4, [200, 31, 300, 0, 77], 5, caught_up, n_stale=10, n_unmapped=3, head=2, tail=2)
    if name == "negative and extreme lags":
        return _extreme_lags()
    if name == "offsets, latest":
        return _offsets(True)
    if name == "offsets, earliest":
        return _offsets(False)
    if name.startswith("at the limit of ") or name.startswith("one over the limit of "):
        return _limit(name.rsplit(" ", 1)[1], 0 if name.startswith("at") else 1)
    if name == "topic of 4097":
        return drawn(5, [50, TOPIC_LIMIT + 1, 30], 4, zeros, owned_frac=0.3)
    if name == "topic over the hint":
        return drawn(6, [50, 90, 30], 4, zeros, hint=64, owned_frac=0.9)
    if name.startswith("ids "):
        return _ids(name[4:])
    if name == "mixed lags":
        return drawn(8, [257, 100, 0, 300, 64], 7, mixed, owned_frac=0.9, n_stale=7)
    raise KeyError(name)


LIMITS = ("N", "n_owned", "M", "T")
NAMES = ("no topics", "no entries", "nothing owned", "one partition", "adjacent topics, all lags 0",
         "equal lag across topics of 63, 64, 65", "run starts at a topic's last position", "topic without consumers between two",
         "previous owner owns nothing in the run", "stale, unmapped, head and tail claims", "negative and extreme lags",
         "offsets, latest", "offsets, earliest") + tuple("at the limit of " + w for w in LIMITS) + \
        tuple("one over the limit of " + w for w in LIMITS) + ("topic of 4097", "topic over the hint", "ids shuffled",
                                                                "ids descending", "ids hostile", "mixed lags")
CLEAN = tuple(n for n in NAMES if n != "topic over the hint")      # the others end without an error


# ---- the dictionary model -----------------------------------------------------------------------------------------------------------
def dict_model(k):
    """The whole call on dicts, lists and loops -> the fifteen outputs in the order of ALL.  Shares no code with sharding: the
    owner of every (topic, id) from the owned lists; per topic the lag of every position through a dict on the id, runs of equal
    lag, per run and member the k-th partition it owned to the k-th place it owns, the rest in order; then every entry's class
    at the sticky order and every member's list."""
    c = k.coop
    po, off = c.part_off.tolist(), c.owned_off.tolist()
    owner, looked_at = {}, 0
    for r in range(c.m):
        for j in range(off[r], off[r + 1]):
            looked_at += 1
            if int(c.owned_topic[j]) >= 0:
                assert (int(c.owned_topic[j]), int(c.owned_pid[j])) not in owner
                owner[(int(c.owned_topic[j]), int(c.owned_pid[j]))] = r
    sticky = [int(x) for x in c.pid]
    kept, saved = [0] * c.t, [0] * c.t
    changed = passed = 0
    for t in range(c.t):
        a, z = po[t], po[t + 1]
        ids = [int(x) for x in k.partition_id[a:z]]
        lag_by_id = dict(zip(ids, (int(x) for x in k.lag[a:z])))
        out = [int(x) for x in c.pid[a:z]]
        own = [int(x) for x in c.rank[a:z]]
        q = [owner.get((t, i), -1) for i in out]
        before = sum(1 for i in range(z - a) if q[i] >= 0 and q[i] == own[i])
        kept[t] = before
        if z - a > k.cap or len(lag_by_id) != len(ids) or sorted(out) != sorted(ids):
            passed += 1
            continue
        lag = [lag_by_id[i] for i in out]
        runs, start = [], 0
        for i in range(1, z - a + 1):
            if i == z - a or lag[i] != lag[start]:
                runs.append(range(start, i))
                start = i
        src_of = {}
        for run in runs:
            placed = set()
            for member in sorted({own[i] for i in run if own[i] >= 0}):
                places = [i for i in run if own[i] == member]
                theirs = [i for i in run if q[i] == member]
                for src, dst in zip(theirs, places):
                    src_of[dst] = src
                    placed.add(src)
            rest = [i for i in run if i not in placed]
            holes = [i for i in run if i not in src_of]
            assert len(rest) == len(holes)
            src_of.update(zip(holes, rest))
        for d in range(z - a):
            sticky[a + d] = out[src_of[d]]
        kept[t] = sum(1 for d in range(z - a) if q[src_of[d]] >= 0 and q[src_of[d]] == own[d])
        saved[t] = kept[t] - before
        changed += any(src_of[d] != d for d in range(z - a))
    summary = [sum(kept) - sum(saved), sum(kept), changed, passed]
    at = C.CoopCase(c.part_off, np.array(sticky, np.int32), c.rank, c.m, c.owned_off, c.owned_topic, c.owned_pid)
    adjusted = C.dict_model(at)
    lists = [[] for _ in range(c.m + 1)]                            # nobody first, then member by member, in the order of the entries
    for t in range(c.t):
        for e in range(po[t], po[t + 1]):
            lists[int(adjusted[1][e]) + 1].append((t, sticky[e]))
    member_off = np.cumsum([len(l) for l in lists]).astype(np.int64)
    flat = [x for l in lists for x in l]
    return (np.array(sticky, np.int32), np.array(kept, np.int64), np.array(saved, np.int64), np.array(summary, np.int64)) + \
        tuple(adjusted) + (member_off, np.array([x[0] for x in flat], np.int32), np.array([x[1] for x in flat], np.int32))


def same(got, exp, what=""):
    for name, g, e in zip(ALL, got, exp):
        np.testing.assert_array_equal(g, e, err_msg="%s %s" % (name, what))


# ---- what the GPU tests break, one thing per run --------------------------------------------------------------------------------------
def break_input(k, bad):
    """A copy of `k` with one thing wrong with the batch's ids: (copy, the topic that is passed through)."""
    b = k.copy()
    c = b.coop
    t = int(np.flatnonzero(np.diff(c.part_off) >= 3)[0])
    a = int(c.part_off[t])
    if bad == "duplicate input id":
        b.partition_id[a + 1] = b.partition_id[a]
    elif bad == "foreign output id":
        ids = set(b.partition_id[a:int(c.part_off[t + 1])].tolist())
        c.pid[a + 1] = next(x for x in range(1 << 20, (1 << 20) + 5000) if x not in ids)
    else:
        raise ValueError(bad)
    return b, t


# ---- la_assign_batch_cooperative_sticky: a rebalance on host arrays -------------------------------------------------------------------
class HostCase:
    """The inputs of one cooperative rebalance of a group that has caught up: the layout, lags with long runs of 0, offsets that
    give those lags, who subscribes to what, and what every member owns -- the oracle's assignment of the same group one
    rebalance earlier, when other partitions lagged."""

    def __init__(self, seed, sizes, m):
        rng = np.random.default_rng(seed)
        self.part_off, self.pid = C.layout(seed, sizes)
        self.m, self.t, self.n = m, len(sizes), int(self.pid.size)
        segs = [np.sort(rng.choice(m, int(rng.integers(1, m + 1)), replace=False)) for _ in sizes]
        self.cons_off = np.concatenate([[0], np.cumsum([x.size for x in segs])]).astype(np.int64)
        self.cons_rank = np.concatenate(segs + [np.empty(0, np.int64)]).astype(np.int32)
        self.k = int(self.cons_rank.size)
        before = S.caught_up_lags(self.n, 0.05, rng)
        self.lag = S.caught_up_lags(self.n, 0.05, rng)
        was = oracle.assign_flat(self.part_off, self.pid, before, self.cons_off, self.cons_rank)
        self.owned = tuple(np.ascontiguousarray(x) for x in sharding.group_by_member_numpy(self.part_off, was[0], was[1], m))
        # offsets: EARLIEST gives self.lag everywhere, LATEST gives it where there is a committed offset and 0 elsewhere
        self.committed = rng.integers(0, 1 << 20, self.n).astype(np.int64)
        self.committed[rng.random(self.n) < 0.3] = -1
        self.begin = rng.integers(0, 1 << 19, self.n).astype(np.int64)
        self.end = np.where(self.committed >= 0, self.committed, self.begin) + self.lag

    def lag_of(self, mode):
        return np.where(self.committed >= 0, self.lag, 0) if mode == "latest" else self.lag

    def expect(self, mode):
        """The eighteen outputs: the target's three, then those of cooperative_round_sticky_numpy."""
        return sharding.assign_cooperative_sticky_numpy(self.part_off, self.pid, self.lag_of(mode), self.cons_off, self.cons_rank, self.m,
                                                        *self.owned, assign=oracle.assign_flat)

    def inputs(self, mode):
        """Keyword arguments of Context.assign_batch_cooperative[_sticky] for mode "lag", "dense", "sparse" or "latest"."""
        if mode == "lag":
            return dict(lag=self.lag)
        kw = dict(end=self.end, committed=self.committed, reset_mode=N.LA_RESET_LATEST if mode == "latest" else N.LA_RESET_EARLIEST)
        if mode == "dense":
            kw["begin"] = self.begin
        elif mode == "sparse":
            kw["none_index"], kw["none_begin"] = N.sparse_begin(self.begin, self.committed)
        return kw


HOST_MODES = ("lag", "dense", "sparse", "latest")


@functools.lru_cache(maxsize=None)
def host_case(name):
    return {"tiny": lambda: HostCase(50, [3, 0, 2], 2), "at the limit": lambda: HostCase(51, [LE // 4] * 4, 8),
            "one over the limit": lambda: HostCase(52, [LE // 4] * 3 + [LE // 4 + 1], 8)}[name]()


HOST_NAMES = ("tiny", "at the limit", "one over the limit")
