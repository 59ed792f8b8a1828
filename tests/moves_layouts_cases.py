"""Two assignments with a layout each, for the tests of la_assignment_moves_device's two-layout form (test_moves_layouts_cpu /
test_moves_layouts_gpu).  Not a test module."""
import numpy as np

from kafka_lag_based_assignor_amd import sharding

I32 = np.iinfo(np.int32)


class LCase:
    """Today's assignment over `part_off`, the previous one over `prev_part_off`, on the host."""

    def __init__(self, part_off, cur_pid, cur_rank, prev_part_off, prev_pid, prev_rank, m, rank_map=None, prev_topic=None, hint=None):
        i32, i64 = (lambda a: np.ascontiguousarray(a, np.int32)), (lambda a: np.ascontiguousarray(a, np.int64))
        self.part_off, self.prev_part_off = i64(part_off), i64(prev_part_off)
        self.cur_pid, self.cur_rank, self.prev_pid, self.prev_rank = i32(cur_pid), i32(cur_rank), i32(prev_pid), i32(prev_rank)
        self.m = int(m)
        self.rank_map = None if rank_map is None else i32(rank_map)
        self.prev_topic = None if prev_topic is None else i32(prev_topic)
        self.t, self.n = self.part_off.size - 1, int(self.part_off[-1])
        self.t_prev, self.n_prev = self.prev_part_off.size - 1, int(self.prev_part_off[-1])
        sizes = np.concatenate([np.diff(self.part_off), np.diff(self.prev_part_off), [0]])
        self.hint = int(sizes.max()) if hint is None else int(hint)

    def copy(self):
        c = lambda a: None if a is None else a.copy()
        return LCase(c(self.part_off), c(self.cur_pid), c(self.cur_rank), c(self.prev_part_off), c(self.prev_pid), c(self.prev_rank),
                     self.m, c(self.rank_map), c(self.prev_topic), self.hint)

    def expect(self):
        return sharding.assignment_moves_layouts_numpy(self.part_off, self.cur_pid, self.cur_rank, self.prev_part_off, self.prev_pid,
                                                       self.prev_rank, self.m, self.rank_map, self.prev_topic)

    def segment_of(self, t):
        """(first, size) of the previous segment of today's topic t; size 0 for a new topic."""
        s = t if self.prev_topic is None else int(self.prev_topic[t])
        if s < 0:
            return 0, 0
        return int(self.prev_part_off[s]), int(self.prev_part_off[s + 1] - self.prev_part_off[s])


def id_pool(rng, kind, count, corners):
    """`count` distinct int32 ids in random order.  shuffled: 0 .. count-1; full: any int32 (with the four corners where asked);
    4096 / 2^20: strided, which a masking hash would chain."""
    if kind == "shuffled":
        return rng.permutation(count).astype(np.int64)
    if kind == "full":
        ids = set([I32.min, -1, 0, I32.max][:count] if corners else [])
        while len(ids) < count:
            ids.update(rng.integers(I32.min, I32.max, count - len(ids), endpoint=True).tolist())
        return rng.permutation(np.array(sorted(ids), np.int64))
    step = {"4096": 4096, "2^20": 1 << 20}[kind]
    assert (count // 2 + 1) * step <= I32.max, "strided ids of %d entries leave int32" % count
    return (rng.permutation(count).astype(np.int64) - count // 2) * step


def build(seed, pairs, m, ids="shuffled", m_prev=None, rank_map=None, topic_map="identity", extra_prev=(), hint=None):
    """pairs: (P_prev, P) or (P_prev, P, how) per topic of today.  P_prev None: the topic is new (map entry -1; needs a map).
    how: "nested" (default: the smaller side's ids are a subset of the larger side's -- a grown or a shrunk topic), "disjoint"
    (no id in common) or "half" (half of today's ids are previous ones).  Each side comes in an order of its own; ranks are
    uniform over [-1, M) / [-1, M_prev).
    topic_map: "identity" (no map), "same" (a map that is the identity) or "permute" (the previous topics in another order,
    with the unreferenced topics of `extra_prev` sizes among them -- their entries are duplicates with ranks out of range, which
    nobody may look at)."""
    rng = np.random.default_rng(seed)
    mp = m_prev or m
    cur_pid, cur_rank, prev_segs = [], [], []
    for t, pair in enumerate(pairs):
        pp, p = pair[0], pair[1]
        how = pair[2] if len(pair) > 2 else "nested"
        n_prev = pp or 0
        pool = id_pool(rng, ids, n_prev + p, t == 0)
        prev_ids = pool[:n_prev]
        if how == "nested":
            cur_ids = pool[:p]
        elif how == "disjoint":
            cur_ids = pool[n_prev:n_prev + p]
        else:
            assert how == "half" and n_prev >= p // 2, pair
            cur_ids = np.concatenate([pool[:p // 2], pool[n_prev:n_prev + p - p // 2]])
        cur_pid.append(cur_ids[rng.permutation(p)])
        cur_rank.append(rng.integers(-1, m, p))
        prev_segs.append(None if pp is None else (prev_ids[rng.permutation(n_prev)], rng.integers(-1, mp, n_prev)))
    cat = lambda xs, dt: np.concatenate(list(xs) + [np.empty(0, dt)]).astype(dt)
    part_off = np.concatenate([[0], np.cumsum([pr[1] for pr in pairs])])
    if topic_map in ("identity", "same"):
        assert not extra_prev and all(s is not None for s in prev_segs)
        order = list(range(len(pairs)))
        prev_topic = None if topic_map == "identity" else np.arange(len(pairs))
    else:
        assert topic_map == "permute", topic_map
        order = [t for t in rng.permutation(len(pairs)).tolist() if prev_segs[t] is not None]
        for size in extra_prev:                                      # unreferenced previous topics, anywhere in the layout
            order.insert(int(rng.integers(0, len(order) + 1)), -1 - size)
        prev_topic = np.full(len(pairs), -1)
    segs = []
    for s, t in enumerate(order):
        if t < 0:
            size = -1 - t
            segs.append((np.full(size, 7), np.full(size, I32.max)))         # would be LA_EINVAL if read
        else:
            segs.append(prev_segs[t])
            if prev_topic is not None:
                prev_topic[t] = s
    prev_part_off = np.concatenate([[0], np.cumsum([len(x[0]) for x in segs])])
    return LCase(part_off, cat(cur_pid, np.int64), cat(cur_rank, np.int64), prev_part_off, cat([x[0] for x in segs], np.int64),
                 cat([x[1] for x in segs], np.int64), m, rank_map, prev_topic, hint)


def naive(c):
    """A per-topic dict join, deliberately plain: what assignment_moves_layouts_numpy has to equal."""
    owner = np.empty(c.n, np.int32)
    topic = [np.zeros(c.t, np.int64) for _ in range(3)]              # moved, added, removed
    gained, lost = np.zeros(c.m, np.int64), np.zeros(c.m, np.int64)
    for t in range(c.t):
        q0, nq = c.segment_of(t)
        before = {}
        for j in range(q0, q0 + nq):
            p = int(c.prev_rank[j])
            assert int(c.prev_pid[j]) not in before
            before[int(c.prev_pid[j])] = -1 if p < 0 else (p if c.rank_map is None else int(c.rank_map[p]))
        for i in range(int(c.part_off[t]), int(c.part_off[t + 1])):
            cur = int(c.cur_rank[i])
            if int(c.cur_pid[i]) not in before:
                owner[i] = sharding.MOVES_NO_PREVIOUS
                topic[1][t] += 1
                if cur >= 0:
                    gained[cur] += 1
                continue
            q = before.pop(int(c.cur_pid[i]))
            owner[i] = q
            if q != cur:
                topic[0][t] += 1
                if cur >= 0:
                    gained[cur] += 1
                if q >= 0:
                    lost[q] += 1
        for q in before.values():
            topic[2][t] += 1
            if q >= 0:
                lost[q] += 1
    return (owner, topic[0], topic[1], topic[2], gained, lost, int(topic[0].sum()), int(topic[1].sum()), int(topic[2].sum()))


NAMES = ("prev_owner", "topic_moved", "topic_added", "topic_removed", "gained", "lost", "moved", "added", "removed")


def same(got, exp, what=""):
    for k, g, e in zip(NAMES, got, exp):
        np.testing.assert_array_equal(g, e, err_msg="%s %s" % (k, what))
