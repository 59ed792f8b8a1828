"""Case builders for la_sticky_ties_device.  Not a test module: test_sticky_cpu.py (sharding.sticky_ties_numpy against an
independent model and brute force) and test_sticky_gpu.py (the kernel against sticky_ties_numpy) import it by name, so both run
the same cases.  Targets are oracle assignments of small workloads, computed once per workload and shared: treat them as
read-only.  prev_owner is drawn per case."""
import numpy as np

from kafka_lag_based_assignor_amd import sharding, synth
from oracle import oracle

import verify_cases as V

LIMIT = sharding.STICKY_MAX_PARTITIONS
I32_MAX = int(np.iinfo(np.int32).max)
SHAPE_P = (0, 1, 2, 63, 64, 65, 256, 257, 4096)


def workload(topics, seed):
    """A batch from per-topic (lags int64[P], consumers C): ids a shuffled 0 .. P-1, ascending ranks with gaps drawn from one
    rank space, so topics share some members and not others."""
    rng = np.random.default_rng(seed)
    ps, cs = [int(np.asarray(l).size) for l, _ in topics], [int(c) for _, c in topics]
    part_off = np.concatenate([[0], np.cumsum(ps)]).astype(np.int64)
    cons_off = np.concatenate([[0], np.cumsum(cs)]).astype(np.int64)
    cat = lambda xs, dt: np.concatenate(list(xs) + [np.empty(0, np.int64)]).astype(dt)
    pid = cat([rng.permutation(p) for p in ps], np.int32)
    lag = cat([np.asarray(l, np.int64) for l, _ in topics], np.int64)
    ranks = cat([np.sort(rng.choice(3 * c + 5, c, replace=False)) for c in cs], np.int32)
    n = int(part_off[-1])
    return synth.Workload("sticky", len(topics), part_off, pid, np.zeros(n, np.int64), lag.copy(), np.zeros(n, np.int64), lag,
                          cons_off, ranks, max(ps) if ps else 0, max(cs) if cs else 0)


def lags_of_runs(lengths, rng=None):
    """Lags whose descending order has runs of exactly these lengths, handed to the partitions in a shuffled order."""
    lag = np.repeat((len(lengths) - np.arange(len(lengths), dtype=np.int64)) * 1000, lengths)
    return lag if rng is None else rng.permutation(lag)


def mixed_lags(p, rng):
    """Half of the partitions from seven values (long runs), the rest below 2^40 (runs of one)."""
    return np.where(rng.random(p) < 0.5, rng.integers(0, 7, p) * 1000, rng.integers(0, 1 << 40, p)).astype(np.int64)


def caught_up_lags(p, rate, rng):
    """A group that has caught up: lag 0 but for a share `rate` of the partitions."""
    return np.where(rng.random(p) < rate, rng.integers(1, 1 << 30, p), 0).astype(np.int64)


def target(w, lag=None):
    """(out_partition, out_member_rank, out_total_lag) of the oracle for `w` (computed once per workload)."""
    return V.oracle_result(w, lag)


def lag_at_positions(w, res):
    """lag_i of every position: the lag of the input partition whose id is out_partition[i] (a dict per topic, on purpose not
    the searchsorted join of sticky_ties_numpy)."""
    out = np.zeros(w.n_partitions, np.int64)
    for t in range(w.n_topics):
        a, z = int(w.part_off[t]), int(w.part_off[t + 1])
        by_id = {int(i): int(l) for i, l in zip(w.partition_id[a:z], w.lag[a:z])}
        out[a:z] = [by_id[int(i)] for i in res[0][a:z]]
    return out


def draw_prev_owner(w, res, seed, kind="mixed"):
    """prev_owner per position.  mixed: a subscriber of the topic drawn at random (half of the positions), the position's own
    owner, -1, -2 (LA_MOVES_NO_PREVIOUS), INT32_MAX or a rank that subscribes elsewhere only; own: the owner itself; none: -1;
    shifted: the owner of the next position of the topic (nearly everything moves, all of it inside the topic's members)."""
    rng = np.random.default_rng(seed)
    own = np.asarray(res[1], np.int32)
    q = np.full(w.n_partitions, -1, np.int32)
    if kind == "none":
        return q
    if kind == "own":
        return own.copy()
    all_ranks = np.unique(w.cons_rank)
    for t in range(w.n_topics):
        a, z = int(w.part_off[t]), int(w.part_off[t + 1])
        r = w.cons_rank[int(w.cons_off[t]):int(w.cons_off[t + 1])]
        p = z - a
        if p == 0:
            continue
        if kind == "shifted":
            q[a:z] = np.roll(own[a:z], -1)
            continue
        elsewhere = np.setdiff1d(all_ranks, r)
        pick = rng.random(p)
        seg = np.where(pick < 0.2, own[a:z], -1).astype(np.int64)
        if r.size:
            seg = np.where(pick >= 0.5, r[rng.integers(0, r.size, p)], seg)
        seg = np.where((pick >= 0.2) & (pick < 0.3), -2, seg)
        seg = np.where((pick >= 0.3) & (pick < 0.35), I32_MAX, seg)
        if elsewhere.size:
            seg = np.where((pick >= 0.35) & (pick < 0.45), elsewhere[rng.integers(0, elsewhere.size, p)], seg)
        q[a:z] = seg
    return q


def prev_owner_from(w, res, prev_res):
    """prev_owner of `res` when the previous rebalance of the same topics and members ended as `prev_res`."""
    return sharding.assignment_moves_numpy(w.part_off, res[0], res[1], prev_res[0], prev_res[1], int(w.cons_rank.max()) + 1)[0]


def expect(w, res, prev, **kw):
    """sharding.sticky_ties_numpy on the workload's lags."""
    return sharding.sticky_ties_numpy(w.part_off, w.partition_id, w.lag, res[0], res[1], prev, **kw)


def model(w, res, prev):
    """The five rules once more, topic by topic and run by run on dicts and sorted lists -> (sticky, kept before per topic, kept
    after per topic).  Shares no code with sticky_ties_numpy."""
    lag = lag_at_positions(w, res)
    sticky = np.array(res[0], np.int32)
    before, after = np.zeros(w.n_topics, np.int64), np.zeros(w.n_topics, np.int64)
    for t in range(w.n_topics):
        a, z = int(w.part_off[t]), int(w.part_off[t + 1])
        runs = {}
        for i in range(a, z):
            runs.setdefault(int(lag[i]), []).append(i)          # (the target is sorted by lag: equal lags are consecutive)
        for positions in runs.values():
            assert positions == list(range(positions[0], positions[-1] + 1))
            moves = {}
            for c in sorted({int(res[1][i]) for i in positions if res[1][i] >= 0}):
                s = [i for i in positions if res[1][i] == c]
                wc = [i for i in positions if prev[i] == c]
                moves.update(dict(zip(wc, s)))                  # zip stops at the shorter: k < min(|S_c|, |W_c|)
            rest = [i for i in positions if i not in moves]
            holes = sorted(set(positions) - set(moves.values()))
            moves.update(dict(zip(rest, holes)))
            for src, dst in moves.items():
                sticky[dst] = res[0][src]
                after[t] += 1 if prev[src] >= 0 and prev[src] == res[1][dst] else 0
        before[t] = sum(1 for i in range(a, z) if prev[i] >= 0 and prev[i] == res[1][i])
    return sticky, before, after


def min_sum(w, res, prev):
    """Sum over the runs and members c >= 0 of min(|S_c|, |W_c|), per topic: what kept after must equal."""
    lag = lag_at_positions(w, res)
    out = np.zeros(w.n_topics, np.int64)
    for t in range(w.n_topics):
        a, z = int(w.part_off[t]), int(w.part_off[t + 1])
        s_count, w_count = {}, {}
        start = a
        for i in range(a, z):
            if i > a and lag[i] != lag[i - 1]:
                start = i
            if res[1][i] >= 0:
                s_count[(start, int(res[1][i]))] = s_count.get((start, int(res[1][i])), 0) + 1
            if prev[i] >= 0:
                w_count[(start, int(prev[i]))] = w_count.get((start, int(prev[i])), 0) + 1
        out[t] = sum(min(n, w_count.get(key, 0)) for key, n in s_count.items())
    return out


def kernel_model(lag, own, prev, out, threads=64):
    """One topic the way csrc/la_sticky.hip walks it (phases 4 to 7): run heads by a max-scan over per-thread chunks, keys
    run << 44 | member << 12 | position, two sorted key arrays, bisections for the group of a candidate, one packed scan over
    (not placed, not filled), the scatter -> (sticky, kept after).  Integers only, so that a slip in the key layout or in the
    pairing shows here, without a GPU."""
    import bisect
    p = len(lag)
    per = -(-p // threads) if p else 0
    chunks = [(min(p, t * per), min(p, t * per + per)) for t in range(threads)]
    heads = [max([i for i in range(a, z) if i == 0 or lag[i] != lag[i - 1]] or [0]) for a, z in chunks]
    key_s, key_w = [], []
    for t, (a, z) in enumerate(chunks):
        run = max(heads[:t] or [0])                                 # the exclusive max-scan
        for i in range(a, z):
            if i == 0 or lag[i] != lag[i - 1]:
                run = i
            if own[i] >= 0:
                key_s.append(run << 44 | (own[i] & 0xFFFFFFFF) << 12 | i)
            if prev[i] >= 0:
                key_w.append(run << 44 | (prev[i] & 0xFFFFFFFF) << 12 | i)
    key_s.sort()
    key_w.sort()
    src_of, placed = [None] * p, [False] * p
    for x, kw in enumerate(key_w):
        group = kw & ~0xFFF
        k = x - bisect.bisect_left(key_w, group)
        s0, s1 = bisect.bisect_left(key_s, group), bisect.bisect_left(key_s, group + 0x1000)
        if k < s1 - s0:
            src_of[key_s[s0 + k] & 0xFFF] = kw & 0xFFF
            placed[kw & 0xFFF] = True
    loose = [i for i in range(p) if not placed[i]]                  # rank of a loose partition = its index here
    holes = [i for i in range(p) if src_of[i] is None]
    assert len(loose) == len(holes)
    for r, d in enumerate(holes):
        src_of[d] = loose[r]
    sticky = [out[s] for s in src_of]
    return sticky, sum(1 for d in range(p) if prev[src_of[d]] >= 0 and prev[src_of[d]] == own[d])


# ---- the shapes of the GPU tests, the smallest that reach each edge -----------------------------------------------------------
def shape_case(p, seed=11):
    """Topics of P partitions: mixed lags with 0, 1, 3 and 32 consumers, one run over the whole topic, all lags distinct."""
    rng = np.random.default_rng(seed + p)
    topics = [(mixed_lags(p, rng), c) for c in (0, 1, 3, 32)]
    topics += [(np.full(p, 77, np.int64), 5), (rng.permutation(p).astype(np.int64) + 1, 4)]
    return workload(topics, seed + p)


def straddle_case(seed=12):
    """Runs across positions 63 / 64 and 255 / 256 (the wavefront's and the small form's edges), runs of two throughout, and
    topics that are one run."""
    rng = np.random.default_rng(seed)
    topics = [(lags_of_runs([60, 8, 180, 20, 32], rng), 7),         # runs [60, 68) and [248, 268)
              (lags_of_runs([62, 4, 190, 2, 42], rng), 32),         # [62, 66), [256, 258): the run STARTS at 256
              (lags_of_runs([2] * 150, rng), 5),                    # many runs of two
              (lags_of_runs([2] * 32, rng), 3),
              (lags_of_runs([1, 2] * 40 + [1], rng), 6),            # runs of one between them
              (lags_of_runs([256], rng), 32)]
    return workload(topics, seed)


def uneven_case():
    """One topic, two runs of 12 positions, 3 consumers (4 positions each per run).  Member A = the lowest rank is the previous
    owner of 7 partitions of the first run (|S_A| = 4 < |W_A| = 7) and of 1 of the second (|S_A| = 4 > |W_A| = 1)."""
    w = workload([(lags_of_runs([12, 12]), 3)], 13)
    res = target(w)
    a, b, c = (int(x) for x in w.cons_rank)
    prev = np.array([a] * 7 + [b] * 2 + [-1] * 3 + [a] + [c] * 9 + [b] * 2, np.int32)
    s_first, s_second = int((res[1][:12] == a).sum()), int((res[1][12:] == a).sum())
    assert (s_first, s_second) == (4, 4)
    return w, res, prev


def mixed_300(seed=14):
    """300 topics of 0 .. 200 partitions: persistent workgroups walk several topics each."""
    rng = np.random.default_rng(seed)
    topics = []
    for t in range(300):
        p = int(rng.integers(0, 201)) if t % 7 else (0, 1, 2, 64, 65, 200)[(t // 7) % 6]
        kind = t % 4
        lag = (mixed_lags(p, rng) if kind == 0 else caught_up_lags(p, 0.05, rng) if kind == 1 else
               np.full(p, 5, np.int64) if kind == 2 else rng.permutation(p).astype(np.int64))
        topics.append((lag, int(rng.integers(0, 9)) if t % 11 else 0))
    return workload(topics, seed)


def caught_up(topics, partitions, consumers, rate, seed):
    """Two consecutive rebalances of the same topics and consumers, the lagging partitions redrawn at `rate` ->
    (workload of the second, its target, prev_owner from the first, the first's target)."""
    rng = np.random.default_rng(seed)
    first = workload([(caught_up_lags(partitions, rate, rng), consumers) for _ in range(topics)], seed)
    lag2 = np.concatenate([caught_up_lags(partitions, rate, rng) for _ in range(topics)])
    second = synth.Workload("sticky", first.n_topics, first.part_off, first.partition_id, first.begin, lag2.copy(), first.committed,
                            lag2, first.cons_off, first.cons_rank, first.max_partitions, first.max_consumers)
    res1, res2 = target(first), target(second)
    return second, res2, prev_owner_from(second, res2, res1), res1


def offsets_case(latest, seed=15):
    """Topics whose lags come from begin / end / committed with some committed < 0: end - committed from four values (ties),
    w.lag = the oracle's computePartitionLag of them under the reset mode."""
    rng = np.random.default_rng(seed)
    ps, cs = [70, 256, 1, 130], [5, 32, 2, 0]
    n = sum(ps)
    committed = rng.integers(0, 1 << 30, n).astype(np.int64)
    end = committed + rng.integers(0, 4, n) * 10
    begin = end - rng.integers(0, 3, n) * 10
    committed[rng.random(n) < 0.3] = -1
    lag = oracle.compute_lags(begin, end, committed, latest)
    cuts = np.cumsum(ps)[:-1]
    w = workload(list(zip(np.split(lag, cuts), cs)), seed)
    return synth.Workload("sticky", w.n_topics, w.part_off, w.partition_id, begin, end, committed, w.lag, w.cons_off, w.cons_rank,
                          w.max_partitions, w.max_consumers)
