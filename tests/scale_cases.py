"""Cases that take the three device-memory forms -- la_assign_pinned_device with LA_FLAG_PINNED_LARGE, la_sticky_ties_device with
LA_FLAG_STICKY_LARGE, la_verify_assignment_device with LA_FLAG_VERIFY_LARGE -- past the sizes their own suites stop at: past one
grid of workgroup steps, past one chunk word per scan thread, past one topic per levels workgroup, past one sort tile class.  Not a
test module: test_scale_cases_cpu.py (every case crosses the threshold it names, and no more than 1.7 x) and test_scale_gpu.py
(the device against the yardsticks) import it by name.

The thresholds are restated here in plain arithmetic, written from the sources and never read from the library:
  step      a workgroup step is 1 024 positions of ONE large topic: steps = sum(ceil(P_t / 1024)) over the large topics
  grid      a phase launches min(steps, 8 x CUs) workgroups; `for (step = blockIdx.x; step < steps; step += gridDim.x)` takes a
            second trip only when steps > 8 x CUs
  scan      the one-workgroup chunk scans have 1 024 threads of per = ceil(steps / 1024) words each; per > 1 runs the serial
            in-thread part, and a thread whose share starts at or past `steps` is idle (its i0 is clamped to n)
  levels    pinned_levels_kernel launches min(n_big, 2 x CUs) workgroups: a workgroup meets a second topic when n_big > 2 x CUs
  class     the radix sort's workgroup width by element count: 256 below 2^17, 512 below 3 x 2^20, 1 024 from there on.  The pinned
            form sorts every large topic on its own (P_t elements), the sticky form sorts 2 x n_pos elements in one go
  mask      the sticky sort's key passes: the 4 member digits and digit 8 + d of a run start while n_pos >> 8 d != 0; digit 10
            (the third byte) from n_pos = 65 536 on, digit 11 from 2^24 on
  match     sticky_match_kernel launches at most 2 048 workgroups of 256: it strides when 2 x n_pos > 524 288
Every builder takes the CU count (the GPU tests pass the device's, the CPU tests 256 and 304).  Cases and their expectations are
built once per CU count and shared: treat them as read-only.  SECONDS holds what building each reference took."""
import functools
import time

import numpy as np

from kafka_lag_based_assignor_amd import sharding

import sticky_cases as S
import sticky_large_cases as SL
import verify_cases as V
import verify_large_cases as VL

LIMIT = 4096                    # a topic of more partitions goes through the device-memory form
MAX_C = 2048                    # LA_PINNED_MAX_CONSUMERS
STEP = 1024
GRID_PER_CU = 8
LEVEL_GROUPS_PER_CU = 2
SCAN_THREADS = 1024
SORT_DIGITS = 12                # digit passes of the radix sort, launched once per tile class of a pinned call
MATCH_ELEMENTS = 2048 * 256     # what one grid of sticky_match_kernel covers without striding
CAP = 1.7                       # large-topic positions of a case <= CAP x what its threshold needs
SECONDS = {}                    # (what, name, ...) -> seconds spent on the CPU reference of a case


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------
def steps_of(ps):
    return sum(-(-int(p) // STEP) for p in ps)


def grid_of(cus):
    return GRID_PER_CU * cus


def scan_per(n_steps):
    return -(-n_steps // SCAN_THREADS)


def idle_scan_threads(n_steps):
    """Threads of a chunk scan whose share starts at or past n_steps."""
    return SCAN_THREADS - -(-n_steps // scan_per(n_steps))


def tile_class(n):
    return 1024 if n >= 3 << 20 else 512 if n >= 1 << 17 else 256


def sticky_pass_mask(n_pos):
    mask = 0xF << 4
    for d in range(4):
        if n_pos >> (8 * d):
            mask |= 1 << (8 + d)
    return mask


def _timed(key, f):
    t0 = time.perf_counter()
    out = f()
    SECONDS[key] = SECONDS.get(key, 0.0) + time.perf_counter() - t0
    return out


# ---- pinned ----------------------------------------------------------------------------------------------------------------------
class Pinned:
    """pinned_cases.PinnedCase's attributes and args(), from arrays: topics = [(ids, lags, ranks)], the claims as three arrays
    (member, topic, id).  Every member's slice of the owned lists is shuffled."""

    def __init__(self, topics, m, member, topic, pid, seed):
        cat = lambda xs, dt: np.concatenate([np.asarray(x, np.int64) for x in xs] + [np.empty(0, np.int64)]).astype(dt)
        ps, cs = [t[0].size for t in topics], [t[2].size for t in topics]
        self.part_off = np.concatenate([[0], np.cumsum(ps)]).astype(np.int64)
        self.cons_off = np.concatenate([[0], np.cumsum(cs)]).astype(np.int64)
        self.pid, self.lag = cat([t[0] for t in topics], np.int32), cat([t[1] for t in topics], np.int64)
        self.cons_rank = cat([t[2] for t in topics], np.int32)
        self.m = int(m)
        member, topic, pid = cat(member, np.int64), cat(topic, np.int64), cat(pid, np.int64)
        mix = np.random.default_rng(seed).permutation(member.size)
        order = mix[np.argsort(member[mix], kind="stable")]
        self.owned_off = np.concatenate([[0], np.cumsum(np.bincount(member, minlength=self.m))]).astype(np.int64)
        self.owned_topic, self.owned_pid = topic[order].astype(np.int32), pid[order].astype(np.int32)
        self.t, self.n, self.k, self.n_owned = len(topics), self.pid.size, self.cons_rank.size, self.owned_topic.size
        for a in (self.part_off, self.cons_off, self.pid, self.lag, self.cons_rank, self.owned_off, self.owned_topic, self.owned_pid):
            a.setflags(write=False)

    def args(self):
        return (self.part_off, self.pid, self.lag, self.cons_off, self.cons_rank, self.m, self.owned_off, self.owned_topic,
                self.owned_pid)

    def shapes(self):
        return list(zip(np.diff(self.part_off).tolist(), np.diff(self.cons_off).tolist()))


def pinned_large(shapes):
    """The partition counts of the topics the flagged pinned call lists."""
    return [p for p, c in shapes if p > LIMIT and c <= MAX_C]


def build_pinned(seed, shapes, m, owned=0.5, foreign=0.05, n_stale=0, held=None, lags=None):
    """Topics of the given (partitions, consumers) shapes over m members, drawn from `seed` in numpy throughout.  owned: the
    share of a topic's partitions that is claimed (a number, or one per topic), by one of the topic's consumers or, with
    probability `foreign`, by any member.  held: {topic: holdings per consumer} -- consumer k of that topic owns holds[k] of its
    partitions and nothing else is claimed there (pinned_large_cases._held).  n_stale: claims of ids their topic does not have.
    lags: per topic "u20" (default; at these sizes a value repeats, so the id decides too) or "ties" (four values)."""
    rng = np.random.default_rng(seed)
    held = held or {}
    topics, member, topic, pid = [], [], [], []
    for t, (p, c) in enumerate(shapes):
        ids = rng.permutation(p).astype(np.int64)
        kind = lags[t] if lags else "u20"
        lag = rng.integers(0, 1 << 20, p) if kind == "u20" else rng.integers(0, 4, p) * 1000
        ranks = np.sort(rng.choice(m, c, replace=False)).astype(np.int64)
        topics.append((ids, lag.astype(np.int64), ranks))
        if t in held:
            who = np.repeat(ranks, held[t])
            assert who.size <= p
            mine = ids[:who.size]
        else:
            share = owned[t] if isinstance(owned, (list, tuple)) else owned
            mine = ids[rng.random(p) < share]
            anyone = (rng.random(mine.size) < foreign) | (c == 0)
            who = np.where(anyone, rng.integers(0, m, mine.size), ranks[rng.integers(0, max(c, 1), mine.size)] if c else 0)
        member.append(who)
        topic.append(np.full(who.size, t))
        pid.append(mine)
    for j in range(n_stale):
        t = j % len(shapes)
        member.append([int(rng.integers(0, m))])
        topic.append([t])
        pid.append([shapes[t][0] + 7 + j])                               # (the ids of a topic are 0 .. P-1)
    return Pinned(topics, m, member, topic, pid, seed + 1)


OUT_OF_ORDER_SHAPES = [(131072, 5), (4097, 3), (21, 2), (131071, 4), (131073, 9)]


def _classes_out_of_order(cus):
    # two tile classes in one call: the class-ordered item list is (4097, 131071 | 131072, 131073), the topic list is not
    return build_pinned(201, OUT_OF_ORDER_SHAPES, 9, owned=0.5, foreign=0.1, n_stale=6)


def three_classes_shapes(cus):
    shapes = [(3 * 2**20 + 1, 2048), (4097, 3), (131072, 9)]
    while steps_of(pinned_large(shapes)) <= grid_of(cus):                # (more than 384 CUs)
        shapes.append((4097, 3))
    return shapes


def _three_classes(cus):
    return build_pinned(202, three_classes_shapes(cus), 2048, owned=0.5, foreign=0.02, n_stale=5)


TOPIC_CONSUMERS = (1, 2, 7, 64, 65, 2048, 0)
TOPIC_OWNED = (0.0, 0.5, 1.0)


SECOND_TOPIC = (LIMIT + 1, 7)               # the one topic a levels workgroup meets second, whatever the CU count: half of it free


def more_topics_shapes(cus):
    """2 x CUs topics whose consumer counts cycle, then SECOND_TOPIC: the levels grid is 2 x CUs workgroups, so topic 2 x CUs is
    the second topic of workgroup 0, behind topic 0 (one consumer, a lone-consumer run)."""
    return [(LIMIT + 1, TOPIC_CONSUMERS[t % 7]) for t in range(LEVEL_GROUPS_PER_CU * cus)] + [SECOND_TOPIC]


def more_topics_owned(cus):
    """The owned share per topic: the cycle, and 0.5 for the topic met second."""
    return [TOPIC_OWNED[t % 3] for t in range(LEVEL_GROUPS_PER_CU * cus)] + [0.5]


def more_topics_held(cus):
    """Every fifth topic: its first consumer holds nothing and every other one the same count, so the levels begin with a run
    for a lone consumer (a topic's only consumer is one anyway)."""
    held = {}
    for t, (p, c) in enumerate(more_topics_shapes(cus)):
        if t % 5 == 0 and c > 0 and t < LEVEL_GROUPS_PER_CU * cus:
            held[t] = [0] + [max(1, (p * 6 // 10) // c)] * (c - 1)
    return held


def _more_topics(cus):
    shapes = more_topics_shapes(cus)
    return build_pinned(203, shapes, 2048, owned=more_topics_owned(cus), foreign=0.05, n_stale=9,
                        held=more_topics_held(cus), lags=["ties" if t % 4 == 3 else "u20" for t in range(len(shapes))])


PINNED = {"classes out of order": _classes_out_of_order, "three classes": _three_classes,
          "more topics than level workgroups": _more_topics}
PINNED_PAST_ONE_GRID = ("three classes", "more topics than level workgroups")
PINNED_SHAPES = {"classes out of order": lambda cus: OUT_OF_ORDER_SHAPES, "three classes": three_classes_shapes,
                 "more topics than level workgroups": more_topics_shapes}


def pinned_need(name, cus):
    """The fewest large-topic positions that reach the case's threshold."""
    if name == "classes out of order":      # a topic below, at and above the 256 -> 512 switch and one of the 256 class between them
        return 131071 + 131072 + 131073 + (LIMIT + 1)
    if name == "three classes":             # one topic per class; the 1 024 class alone is 3 073 steps
        return 3 * 2**20 + 131072 + (LIMIT + 1)
    return (LEVEL_GROUPS_PER_CU * cus + 1) * (LIMIT + 1)


@functools.lru_cache(maxsize=None)
def pinned_case(name, cus):
    """(case, expectation): sharding.assign_pinned_numpy without the partition limit."""
    c = PINNED[name](cus)
    exp = _timed(("pinned", name, cus), lambda: sharding.assign_pinned_numpy(*c.args(), max_partitions=sharding.PINNED_ANY_SIZE))
    return c, exp


# ---- sticky ----------------------------------------------------------------------------------------------------------------------
def lags_with_runs(p, rng, specials=(), dense_until=None):
    """Lags of one topic whose descending order starts with a run of ONE position, holds the runs `specials` = [(start, length)]
    at exactly these positions of the topic and is cut at random elsewhere: runs of 2.5 positions on average before
    `dense_until`, of 50 behind it."""
    at = np.arange(p)
    cut = rng.random(p) < np.where(at < (p // 2 if dense_until is None else dense_until), 0.4, 0.02)
    cut[:2] = True
    for s, n in specials:
        assert 2 <= s and s + n <= p
        cut[s] = True
        cut[s + 1:s + n] = False
        if s + n < p:
            cut[s + n] = True
    starts = np.flatnonzero(cut)
    return S.lags_of_runs(np.diff(np.append(starts, p)), rng)


def _digit10_edge(p):
    rng = np.random.default_rng(300 + p)
    return S.workload([(S.mixed_lags(p, rng), 7)], 300 + p)


DIGIT10_RUNS = (70000, 70000 + 65536)       # two run starts of the first topic that differ in the third byte only


def _digit10_in_use(cus):
    rng = np.random.default_rng(310)
    first = lags_with_runs(150000, rng, [(s, 9) for s in DIGIT10_RUNS])
    return S.workload([(first, 7), (S.mixed_lags(30, rng), 3), (S.mixed_lags(LIMIT + 1, rng), 5), (S.mixed_lags(60000, rng), 3)], 310)


def _match_strides(cus):
    rng = np.random.default_rng(320)
    total = MATCH_ELEMENTS // 2 + 9
    p = total // 3
    return S.workload([(S.mixed_lags(p, rng), 7), (S.mixed_lags(p, rng), 5), (S.mixed_lags(total - 2 * p, rng), 7)], 320)


def past_one_grid_shapes(cus):
    """One topic of 1.6 M, one of 300 000, then topics of 4 097 .. 9 000 until the positions pass one grid of steps."""
    rng = np.random.default_rng(330)
    shapes = [(1600000, 7), (300000, 5)]
    while sum(p for p, _ in shapes) <= STEP * grid_of(cus):
        shapes.append((int(rng.integers(LIMIT + 1, 9001)), int(rng.integers(3, 8))))
    return shapes


def past_one_grid_runs(cus):
    """The two runs the case promises, in the first topic (whose positions are the list's): one that covers a whole share of a
    scan thread, so it crosses two share boundaries of K3, and one that ends exactly on a multiple of 1 024."""
    share = scan_per(steps_of(p for p, _ in past_one_grid_shapes(cus))) * STEP
    return [(100 * share - 700, share + 1400), (700 * STEP - 37, 37)]


def _past_one_grid(cus):
    rng = np.random.default_rng(331)
    shapes = past_one_grid_shapes(cus)
    topics = [(lags_with_runs(shapes[0][0], rng, past_one_grid_runs(cus)), shapes[0][1])]
    topics += [(lags_with_runs(p, rng), c) for p, c in shapes[1:]]
    return S.workload(topics, 331)


STICKY = {"digit 10, below": lambda cus: _digit10_edge(65535), "digit 10, at": lambda cus: _digit10_edge(65536),
          "digit 10, above": lambda cus: _digit10_edge(65537), "digit 10 in use": _digit10_in_use, "match strides": _match_strides,
          "past one grid": _past_one_grid}
STICKY_SMALL = tuple(n for n in STICKY if n != "past one grid")
STICKY_RUNS = [(n, k) for n in STICKY for k in (("mixed", "shifted", "skewed") if n in STICKY_SMALL else ("mixed", "shifted"))]


def sticky_need(name, cus):
    if name.startswith("digit 10,"):
        return 65536
    if name == "digit 10 in use":           # two run starts 65 536 apart and a topic that begins behind them
        return 2 * 65536 + (LIMIT + 1)
    if name == "match strides":
        return MATCH_ELEMENTS // 2 + 1
    return max(STEP * grid_of(cus) + 1, 3 * 2**19)


@functools.lru_cache(maxsize=None)
def sticky_case(name, cus):
    """(workload, the oracle's target)."""
    w = STICKY[name](cus)
    return w, _timed(("sticky target", name, cus), lambda: S.target(w))


@functools.lru_cache(maxsize=None)
def sticky_prev(name, cus, kind, seed=3):
    w, res = sticky_case(name, cus)
    if kind == "skewed":
        return SL.skewed_prev(w, res, seed)
    return S.draw_prev_owner(w, res, seed, kind)


@functools.lru_cache(maxsize=None)
def sticky_expected(name, cus, kind):
    w, res = sticky_case(name, cus)
    prev = sticky_prev(name, cus, kind)
    return _timed(("sticky", name, cus, kind), lambda: SL.expect(w, res, prev))


def run_bounds(w, res):
    """(starts, ends) of every run of the large topics in positions of the concatenated list: sticky_large_cases.groups_of
    without the groups, in numpy (test_scale_cases_cpu.py holds it to groups_of on a small case)."""
    lag, topic = [], []
    for t in SL.big_topics(w):
        a, z = int(w.part_off[t]), int(w.part_off[t + 1])
        by_id = np.argsort(w.partition_id[a:z], kind="stable")
        lag.append(w.lag[a:z][by_id[np.searchsorted(w.partition_id[a:z][by_id], res[0][a:z])]])
        topic.append(np.full(z - a, t))
    lag, topic = np.concatenate(lag), np.concatenate(topic)
    head = np.ones(lag.size, bool)
    head[1:] = (lag[1:] != lag[:-1]) | (topic[1:] != topic[:-1])
    starts = np.flatnonzero(head)
    return starts, np.append(starts[1:], lag.size)




# ---- verify ----------------------------------------------------------------------------------------------------------------------
# The global form walks three domains, each in steps numbered through the large topics: partitions (max(1, ceil(P / 1024)) steps
# of a topic), consumers (ceil(C / 1024)) and (chunk, consumer) pairs (ceil(chunks x C / 256), chunks = ceil(rounds /
# ceil(sqrt(rounds))), rounds = ceil(P / C)).  Phases 0 and 5 walk partitions then consumers, phase 1 partitions, phase 2
# partitions then pairs, phase 3 consumers, phase 4 pairs.  A topic is large by its partitions OR by its consumers.
VERIFY_WIDE = 1                             # the topic of 4 100 consumers among those that are large by their partitions
CONSUMER_LARGE = (8, LIMIT + 1)             # large by its consumers alone: 1 partition step, 5 consumer steps, 17 pair steps
PAIR_STEP = 256


def verify_partition_topics(cus):
    return LEVEL_GROUPS_PER_CU * cus + 2


def domain_steps(shape):
    """(partition, consumer, pair) steps of one large topic."""
    p, c = shape
    rounds = -(-p // c) if c else 0
    chunk_rounds = (0 if rounds == 0 else int(np.sqrt(rounds - 1)) + 1)
    while chunk_rounds * chunk_rounds < rounds:                          # (ceil(sqrt(rounds)) whatever the float gave)
        chunk_rounds += 1
    chunks = -(-rounds // chunk_rounds) if rounds else 0
    return max(1, -(-p // STEP)), -(-c // STEP), -(-(chunks * c) // PAIR_STEP)


def verify_consumer_topics(cus):
    """As many topics of CONSUMER_LARGE as put the first consumer step of the last one at 8 x CUs or later."""
    before = (verify_partition_topics(cus) - 1) * domain_steps((LIMIT + 1, 64))[1] + domain_steps((LIMIT + 1, 4100))[1]
    return -(-(grid_of(cus) - before) // domain_steps(CONSUMER_LARGE)[1]) + 1


def verify_shapes(cus):
    """2 x CUs + 1 topics of 4 097 x 64 with one of 4 097 x 4 100 among them, then the topics that are large by consumers."""
    shapes = [(LIMIT + 1, 64)] * (verify_partition_topics(cus) - 1)
    shapes.insert(VERIFY_WIDE, (LIMIT + 1, 4100))
    return shapes + [CONSUMER_LARGE] * verify_consumer_topics(cus)


def first_steps(shapes):
    """Per topic the first step of each domain, and the three totals behind them."""
    at, out = [0, 0, 0], []
    for s in shapes:
        out.append(tuple(at))
        at = [a + d for a, d in zip(at, domain_steps(s))]
    return out, tuple(at)


def verify_need(cus):
    """Positions up to the partition-large topic of the first planted fault (its first partition step is 8 x CUs or later) and
    the six behind it, and those of the consumer-large topics, which the consumer domain needs to pass 8 x CUs."""
    return (-(-grid_of(cus) // 5) + 7) * (LIMIT + 1) + verify_consumer_topics(cus) * CONSUMER_LARGE[0]


@functools.lru_cache(maxsize=None)
def verify_case(cus):
    """(batch, the oracle's result, the yardstick's verdicts and summary of it)."""
    w = VL.batch(verify_shapes(cus), 401)
    res = _timed(("verify target", cus), lambda: V.oracle_result(w))
    return w, res, _timed(("verify", cus), lambda: VL.yardstick(w, res))


LAST_POSITION = "last position: foreign id, owner -1"
LEFT_OUT = "partial last round: an unpicked consumer for the last picked"


def verify_faults(cus):
    """{topic: fault}: a fault of every class, each class in a topic of its own, every one in a step of index 8 x CUs or later
    of the phase that finds it.  IDS, ORDER, OWNER and GREEDY in the last partition-large topics (phases 1, 2 and 5, partition
    steps), the last of them with two faults at its last position, the only one of its last 1 024-block.  TOTALS in the last
    consumer-large topic (phase 3, consumer steps); in the one before it a consumer the partial last round left out, which phase
    5 finds in a consumer step from what phase 4 left in a pair step."""
    base, t = verify_partition_topics(cus), len(verify_shapes(cus))
    return {base - 1: LAST_POSITION, base - 2: "swap neighbours, different lags", base - 3: "-1 in a topic with consumers",
            base - 4: "swap owners inside a round", base - 5: "repeated id", t - 2: LEFT_OUT, t - 1: "total + 1"}


FAULT_CLASS = dict(V.CATALOGUE, **{LAST_POSITION: V.IDS | V.OWNER})


@functools.lru_cache(maxsize=None)
def verify_planted(cus):
    """(the result with verify_faults planted, the yardstick's verdicts and summary of it)."""
    w, res, _ = verify_case(cus)
    for t, name in verify_faults(cus).items():
        if name in V.CATALOGUE:
            res = V.mutate(name, w, res, t)
            assert res is not None, name
        else:
            op, om = res[0].copy(), res[1].copy()
            last = int(w.part_off[t + 1]) - 1
            op[last], om[last] = LIMIT + 1, -1                           # (the ids of a topic are 0 .. P-1)
            res = (op, om, res[2])
    return res, _timed(("verify planted", cus), lambda: VL.yardstick(w, res))
