#!/usr/bin/env python3
"""Time a cooperative rebalance from host arrays, call by call, the ways a host can make it:

    python tools/assign_coop_probe.py [--sizes 100,1000,2048 --calls 3000] [--out profiles/assign_coop_probe.txt]
    LA_LIB_PATH=<another build's liblagassign.so> python tools/assign_coop_probe.py --grouped-only

  two calls  la_assign_batch_sparse with host result arrays, then la_cooperative_round on them: what a host had to do before
             la_assign_batch_cooperative existed (two waits, the target across the link twice)
  fused      la_assign_batch_cooperative (a zero-copy staged call whose last launch is the round's workgroup)
  general    the same with LA_COOP_FORCE_TABLE (the composition behind one entry point)
  grouped    la_assign_batch_grouped at 100 and 2 000 partitions: the eager call, which the layout and HostCall changes must
             leave where it was.  --grouped-only runs this leg alone, twice, so that the same file can record another build of
             the library (LA_LIB_PATH) beside this one.

A point is N partitions over topics of 25, 8 members all subscribed to everything, ~1 % of the partitions without a committed
offset, every partition owned by the member a previous random assignment gave it (n_owned = N), and the outputs the C++ host
asks for (lists, target, totals, the four per-member counts, withheld per topic, summary).  The forms are compared with each
other first.  After a warm-up the legs ALTERNATE in blocks of 100 calls inside this one process; every call is timed on the
wall clock (the calls wait for their results); printed are the median and min .. max of the per-call times in microseconds.  A
record: no threshold hangs on a time.  The last line of a point says whether the fused call is faster than the two calls.
Exit status 1 only when results differ.  Needs a GPU.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(n, m=8, p=25):
    rng = np.random.default_rng(n)
    sizes = [p] * (n // p) + ([n % p] if n % p else [])
    t = len(sizes)
    part_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pid = np.concatenate([rng.permutation(s) for s in sizes]).astype(np.int32)
    com = rng.integers(0, 1 << 20, n).astype(np.int64)
    com[rng.random(n) < 0.01] = -1
    begin = rng.integers(0, 1 << 19, n).astype(np.int64)
    end = np.maximum(com, begin) + rng.integers(0, 1 << 20, n)
    cons_off = (np.arange(t + 1) * m).astype(np.int64)
    cons_rank = np.tile(np.arange(m, dtype=np.int32), t)
    return t, part_off, pid, begin, end, com, cons_off, cons_rank


def timed(legs, calls, block=100):
    """Per-call wall-clock times of every leg, the legs alternating block by block."""
    times = {k: [] for k in legs}
    for f in legs.values():
        for _ in range(200):
            f()
    done = 0
    while done < calls:
        for k, f in legs.items():
            for _ in range(block):
                t0 = time.perf_counter_ns()
                f()
                times[k].append((time.perf_counter_ns() - t0) * 1e-3)
        done += block
    return times


def fmt(v):
    return "%.1f us (min %.1f .. max %.1f, %d calls)" % (float(np.median(v)), min(v), max(v), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,1000,2048")
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--grouped-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from kafka_lag_based_assignor_amd import _native as N
    from kafka_lag_based_assignor_amd import sharding
    if not torch.cuda.is_available():
        sys.exit("assign_coop_probe: no GPU")
    ctx = N.Context(0)
    lib = N.load()
    h = ctx._h
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("assign_coop_probe: %d timed calls per leg and point, legs alternating in blocks of 100, wall clock per call, device %s, "
        "library %s" % (args.calls, torch.cuda.get_device_name(0), os.path.relpath(N.LIB_PATH, ROOT)))
    addr = lambda a: a.ctypes.data if a is not None and a.size else None
    m = 8

    def grouped_leg(n):
        t, part_off, pid, begin, end, com, cons_off, cons_rank = workload(n)
        off, g_t, g_p, tot = np.zeros(m + 1, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(cons_rank.size, np.int64)
        a = [h, t] + [addr(x) for x in (part_off, pid, begin, end, com)] + [N.LA_RESET_EARLIEST, addr(cons_off), addr(cons_rank), m,
                                                                            addr(off), addr(g_t), addr(g_p), addr(tot)]
        keep = (part_off, pid, begin, end, com, cons_off, cons_rank, off, g_t, g_p, tot)
        return (lambda: lib.la_assign_batch_grouped(*a)), keep

    for run in (1, 2):
        legs, keep = {}, []
        for n in (100, 2000):
            f, k = grouped_leg(n)
            assert f() == 0, ctx._lib.la_last_error(h)
            legs["%d partitions" % n] = f
            keep.append(k)
        times = timed(legs, args.calls)
        say("la_assign_batch_grouped, run %d: " % run + "; ".join("%s %s" % (k, fmt(v)) for k, v in times.items()))
    ok = True
    for word in ([] if args.grouped_only else args.sizes.split(",")):
        n = int(word)
        t, part_off, pid, begin, end, com, cons_off, cons_rank = workload(n)
        none_index, none_begin = N.sparse_begin(begin, com)
        rng = np.random.default_rng(n + 1)
        owned = [np.ascontiguousarray(x) for x in sharding.group_by_member_numpy(part_off, pid, rng.integers(0, m, n).astype(np.int32), m)]
        k = cons_rank.size

        def outputs():
            return dict(member_off=np.zeros(m + 1, np.int64), grouped_topic=np.zeros(n, np.int32), grouped_partition=np.zeros(n, np.int32),
                        totals=np.zeros(k, np.int64), out_partition=np.zeros(n, np.int32), out_member_rank=np.zeros(n, np.int32),
                        kept=np.zeros(m, np.int64), fresh=np.zeros(m, np.int64), pending=np.zeros(m, np.int64),
                        release=np.zeros(m, np.int64), topic_withheld=np.zeros(t, np.int64), summary=np.zeros(6, np.int64))

        def coop_args(o, flags):
            g = N.AssignCoopArgs()
            g.struct_size, g.flags, g.n_topics, g.reset_mode = ctypes.sizeof(N.AssignCoopArgs), flags, t, N.LA_RESET_EARLIEST
            g.part_off, g.partition_id, g.end_off, g.committed_off = addr(part_off), addr(pid), addr(end), addr(com)
            g.n_none, g.none_index, g.none_begin = none_index.size, addr(none_index), addr(none_begin)
            g.cons_off, g.cons_rank, g.n_members, g.n_owned = addr(cons_off), addr(cons_rank), m, n
            g.owned_member_off, g.owned_topic, g.owned_partition = [addr(x) for x in owned]
            g.member_off, g.grouped_topic, g.grouped_partition = addr(o["member_off"]), addr(o["grouped_topic"]), addr(o["grouped_partition"])
            g.out_total_lag, g.out_partition, g.out_member_rank = addr(o["totals"]), addr(o["out_partition"]), addr(o["out_member_rank"])
            g.member_kept, g.member_fresh, g.member_pending, g.member_release = [addr(o[x]) for x in ("kept", "fresh", "pending", "release")]
            g.topic_withheld, g.summary = addr(o["topic_withheld"]), addr(o["summary"])
            return g

        o_fused, o_general, o_two = outputs(), outputs(), outputs()
        g_fused, g_general = coop_args(o_fused, 0), coop_args(o_general, N.LA_COOP_FORCE_TABLE)
        r = N.CoopRoundArgs()
        r.struct_size = ctypes.sizeof(N.CoopRoundArgs)
        a = r.adjust
        a.struct_size = ctypes.sizeof(N.CoopArgs)
        a.n_topics, a.n_partitions, a.n_members, a.n_owned = t, n, m, n
        a.d_part_off, a.d_out_partition, a.d_out_member_rank = addr(part_off), addr(o_two["out_partition"]), addr(o_two["out_member_rank"])
        a.d_owned_member_off, a.d_owned_topic, a.d_owned_partition = [addr(x) for x in owned]
        a.d_member_kept, a.d_member_fresh, a.d_member_pending, a.d_member_release = [addr(o_two[x]) for x in ("kept", "fresh", "pending", "release")]
        a.d_topic_withheld, a.d_summary = addr(o_two["topic_withheld"]), addr(o_two["summary"])
        r.member_off, r.grouped_topic, r.grouped_partition = addr(o_two["member_off"]), addr(o_two["grouped_topic"]), addr(o_two["grouped_partition"])
        sparse = [h, t, addr(part_off), addr(pid), addr(end), addr(com), N.LA_RESET_EARLIEST, none_index.size, addr(none_index),
                  addr(none_begin), addr(cons_off), addr(cons_rank), addr(o_two["out_partition"]), addr(o_two["out_member_rank"]),
                  addr(o_two["totals"])]

        def two_calls():
            return lib.la_assign_batch_sparse(*sparse) or lib.la_cooperative_round(h, ctypes.byref(r))

        legs = {"two calls": two_calls,
                "fused": lambda: lib.la_assign_batch_cooperative(h, ctypes.byref(g_fused)),
                "general": lambda: lib.la_assign_batch_cooperative(h, ctypes.byref(g_general))}
        launches = {}
        for name, f in legs.items():
            assert f() == 0, ctx._lib.la_last_error(h)
            launches[name] = ctx.last_launches()
            if name == "fused":
                assert ctx.last_pipeline() == N.LA_PIPELINE_ZERO_COPY
        same = all(np.array_equal(o_fused[x], o_two[x]) and np.array_equal(o_general[x], o_two[x]) for x in o_two)
        ok = ok and same
        times = timed(legs, args.calls)
        med = {name: float(np.median(v)) for name, v in times.items()}
        say("N = n_owned = %d, T = %d, M = %d: " % (n, t, m) + "; ".join(
            "%s %s%s" % (name, fmt(v), ", %d kernel launches%s" % (launches[name], " in the second call" if name == "two calls" else ""))
            for name, v in times.items()) + "; results %s" % ("agree" if same else "DIFFER"))
        say("    fused / two calls = %.2f: the fused call is %s at %d partitions" % (
            med["fused"] / med["two calls"], "faster" if med["fused"] < med["two calls"] else "NOT FASTER", n))
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
