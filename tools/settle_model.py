#!/usr/bin/env python3
"""Replay of the wave-tile kernel's greedy rounds (csrc/la_wave_tile_impl.h, greedy_rounds_tile) in numpy: what the consumer
bins look like when a round's sort starts, what settle_lanes_p64 (csrc/la_sort64.h) does with them, and what that costs in a
simple VALU count.  Exact integer arithmetic, no GPU.

    python tools/settle_model.py --partitions 256 --consumers 32 --dist zipf [--topics 64] [--d 4] [--k 4]

One group of L lanes holds one topic's bins, one per lane: bin = (total << 6) | index, lanes beyond the consumers an all-ones
sentinel.  Round q adds the lags at sorted positions q*C .. q*C+C-1 to the bins in lane order, and the next round sorts first.
From the third round on (q >= 2) the sort is the settle:

    descents   lanes whose bin is below their left neighbour's; none -> "in_order", nothing runs
    tried      the wavefront's largest per-group count is <= D (and the network spans >= 32 lanes)
    passes     even pass (pairs 2k, 2k+1), odd pass (2k+1, 2k+2), even, odd ... at most K pairs; the settle stops after the
               first odd pass that exchanges nothing, or an even pass (from the second pair on) that exchanges nothing: the
               pass before left the other pairs in order, so the bins are sorted -> "settled"
    gave_up    K pairs and the last odd pass still exchanged something: the bitonic network sorts what is there
    not_tried  more than D descents (or fewer than 32 lanes): the network, as before

All decisions are taken per WAVEFRONT (64 / L groups): settle_wave takes the rows of one wavefront.
"""
import argparse
import os
import sys

import numpy as np

# kSettleMaxDescents / kSettleMaxPairs of csrc/la_sort64.h
D_DEFAULT = 4
K_DEFAULT = 4
SENTINEL = np.uint64(0xFFFFFFFFFFFFFFFF)

# VALU instructions per piece (profiles/tile_settle_rounds.txt lists the generated code)
VALU_CHECK_BEFORE = 6        # lanes-in-order test as the compiler wrote it: 2 moves, a 64-bit compare, the lane condition
VALU_CHECK = 2               # lane_descents_p64
VALU_EVEN = 4
VALU_ODD = 6
VALU_STAGE = 4               # one compare-exchange stage of the network


def network_valu(lc):
    n = int(lc).bit_length() - 1
    return VALU_STAGE * n * (n + 1) // 2


def descents(row):
    """Number of positions whose element is below its left neighbour."""
    row = np.asarray(row, np.uint64)
    return int(np.count_nonzero(row[1:] < row[:-1]))


def even_pass(row):
    """Pairs (2k, 2k+1) of a row of even length.  Returns (row, exchanged anything)."""
    r = np.array(row, np.uint64)
    a, b = r[0::2].copy(), r[1::2].copy()
    sw = b < a
    r[0::2], r[1::2] = np.where(sw, b, a), np.where(sw, a, b)
    return r, bool(sw.any())


def odd_pass(row):
    """Pairs (2k+1, 2k+2); the first and the last element of the row have no partner."""
    r = np.array(row, np.uint64)
    a, b = r[1:-1:2].copy(), r[2::2].copy()
    sw = b < a
    r[1:-1:2], r[2::2] = np.where(sw, b, a), np.where(sw, a, b)
    return r, bool(sw.any())


def settle_wave(rows, lc, d=D_DEFAULT, k=K_DEFAULT):
    """The settle of one wavefront: `rows` = the bins of its groups (equal lengths L, a power of two), `lc` the lanes the
    network spans.  Returns (sorted rows, info): info = {descents (largest of a group), outcome, passes, pairs, valu,
    valu_before, stopped_unsorted}.  stopped_unsorted is True if the stop rule fired while some row was not sorted (never)."""
    rows = [np.array(r, np.uint64) for r in rows]
    most = max(descents(r) for r in rows)
    before = VALU_CHECK_BEFORE + (network_valu(lc) if most else 0)
    info = dict(descents=most, outcome="in_order", passes=0, pairs=0, valu=VALU_CHECK, valu_before=before, stopped_unsorted=False)
    if most == 0:
        return rows, info
    if lc < 32 or most > d:
        info.update(outcome="not_tried", valu=VALU_CHECK + network_valu(lc))
        return [np.sort(r) for r in rows], info
    passes = 0
    valu = VALU_CHECK
    stopped = False
    for p in range(k):
        done = [even_pass(r) for r in rows]
        rows, any_even = [x[0] for x in done], any(x[1] for x in done)
        passes += 1
        valu += VALU_EVEN
        if p > 0 and not any_even:
            stopped = True
            break
        done = [odd_pass(r) for r in rows]
        rows, any_odd = [x[0] for x in done], any(x[1] for x in done)
        passes += 1
        valu += VALU_ODD
        if not any_odd:
            stopped = True
            break
    info.update(passes=passes, pairs=(passes + 1) // 2)
    if stopped:
        info.update(outcome="settled", valu=valu, stopped_unsorted=any(descents(r) for r in rows))
        return rows, info
    info.update(outcome="gave_up", valu=valu + network_valu(lc))
    return [np.sort(r) for r in rows], info


def sorted_lags(lag, pid):
    """A topic's lags in assignment order: lag descending, partition id ascending."""
    lag, pid = np.asarray(lag, np.int64), np.asarray(pid, np.int64)
    return lag[np.lexsort((pid, -lag))]


def replay_wave(topics, l, d=D_DEFAULT, k=K_DEFAULT):
    """Rounds of one wavefront.  topics: list of (sorted lags, consumers) for its groups, consumers <= l.  Yields per round
    q >= 2 the rows as the sort finds them and the info of settle_wave.  Rounds 0 and 1 (no sort; mirror or network) are
    replayed with np.sort."""
    lc = l
    cmax = max(c for _, c in topics)
    for w in (4, 8, 16, 32):
        if w < l and cmax <= w:
            lc = w
            break
    rows = []
    for _, c in topics:
        r = np.full(l, SENTINEL, np.uint64)
        r[:c] = np.arange(c, dtype=np.uint64)
        rows.append(r)
    rounds = max((len(s) + c - 1) // c if c else 0 for s, c in topics)
    for q in range(rounds):
        info = None
        if q == 1:
            rows = [np.sort(r) for r in rows]
        elif q > 1:
            found = [r.copy() for r in rows]
            rows, info = settle_wave(rows, lc, d, k)
            yield q, found, info
        for r, (s, c) in zip(rows, topics):
            take = np.asarray(s[q * c:(q + 1) * c], np.int64)
            r[:take.size] += take.astype(np.uint64) << np.uint64(6)


def classify(topics, l, d=D_DEFAULT, k=K_DEFAULT):
    """Set of classes the rounds of one wavefront fall in: "in_order", "settled_<pairs>", "gave_up", "not_tried", and
    "only_<i>|<i+1>" for a round whose single descent sits between bins i and i+1."""
    out = set()
    for _, found, info in replay_wave(topics, l, d, k):
        o = info["outcome"]
        out.add("settled_%d" % info["pairs"] if o == "settled" else o)
        for r in found:
            bad = np.flatnonzero(r[1:] < r[:-1])
            if bad.size == 1:
                out.add("only_%d|%d" % (bad[0], bad[0] + 1))
    return out


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from kafka_lag_based_assignor_amd import synth
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--partitions", type=int, default=256)
    ap.add_argument("--consumers", type=int, default=32)
    ap.add_argument("--dist", default="zipf", choices=["zipf", "pareto", "uniform40", "uniform63", "zero"])
    ap.add_argument("--topics", type=int, default=64)
    ap.add_argument("--d", type=int, default=D_DEFAULT)
    ap.add_argument("--k", type=int, default=K_DEFAULT)
    ap.add_argument("--per-round", action="store_true", help="one line per round of the first wavefront")
    a = ap.parse_args()
    l = max(8, 1 << (a.consumers - 1).bit_length())
    g = 64 // l
    w = synth.make_uniform("model", 6, a.topics, a.partitions, a.consumers, a.dist, offsets=False)
    lag = w.lag.reshape(a.topics, a.partitions)
    pid = w.partition_id.reshape(a.topics, a.partitions)
    tot = dict(rounds=0, in_order=0, settled=0, gave_up=0, not_tried=0, passes=0, valu=0, valu_before=0)
    print("%s %d x %d, L = %d, %d topics, D = %d, K = %d" % (a.dist, a.partitions, a.consumers, l, a.topics, a.d, a.k))
    for t0 in range(0, a.topics - g + 1, g):
        topics = [(sorted_lags(lag[t], pid[t]), a.consumers) for t in range(t0, t0 + g)]
        for q, found, info in replay_wave(topics, l, a.d, a.k):
            if a.per_round and t0 == 0:
                print("  round %2d: descents %2d  %-9s passes %d (pairs %d)  VALU %3d -> %3d"
                      % (q, info["descents"], info["outcome"], info["passes"], info["pairs"], info["valu_before"], info["valu"]))
            tot["rounds"] += 1
            tot[info["outcome"]] += 1
            for key in ("passes", "valu", "valu_before"):
                tot[key] += info[key]
            assert not info["stopped_unsorted"]
    n = max(tot["rounds"], 1)
    waves = max(a.topics // g, 1)
    print("  rounds >= 2: %d; in order %.1f %%, settled %.1f %%, gave up %.1f %%, not tried %.1f %%; passes per settled or given-up round %.2f"
          % (tot["rounds"], 100.0 * tot["in_order"] / n, 100.0 * tot["settled"] / n, 100.0 * tot["gave_up"] / n,
             100.0 * tot["not_tried"] / n, tot["passes"] / max(tot["settled"] + tot["gave_up"], 1)))
    print("  modelled VALU of those rounds' sorts per wavefront: %.0f -> %.0f" % (tot["valu_before"] / waves, tot["valu"] / waves))


if __name__ == "__main__":
    main()
