#!/usr/bin/env python3
"""Time la_assignment_moves_device against a restatement in torch ops on the same device arrays.

    python tools/moves_probe.py [--topics 100000 --partitions 256 --consumers 32 --launches 20 --windows 5] [--layouts] [--out FILE]

The layout is T topics x P partitions x C consumers (the bench's target shape by default).  The library assigns it several
times with every lag redrawn; consecutive assignments are the (previous, current) pairs, in enough resident copies that a call
never finds its inputs in the 256 MiB Infinity Cache (768 MB between two touches of one copy).  After a warm-up, `windows` timed
windows per side, library and torch alternating, each ONE pair of HIP events around `launches` back-to-back calls on the stream
they run on.  The torch side is the yardstick that is not the code under test: sort each side by  topic << 32 | id, scatter the
previous ranks through the two orders, compare, torch.bincount for the three counts.

Prints the median and the spread (min .. max) of both sides in microseconds per call, the bytes the call must move (16 B read
per partition, 4 B written for prev_owner), its streaming floor at 8 TB/s and the fraction of it the library reaches, and whether
the library is not slower than torch.  Both sides' results are compared bit for bit first.  Exit status 1 when the results
differ or the library is slower.  Needs a GPU: there is nothing to fall back to.

--layouts adds a leg for the two-layout form (d_prev_part_off): 1 % of the topics are grown by 16 partitions and assigned again,
and that assignment is joined against a previous one over the ungrown layout.  It is timed in the same windows next to the
one-layout call on the same previous arrays and checked against sharding.assignment_moves_layouts_numpy; its time is a record,
no threshold hangs on it.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
CACHE_PROOF_BYTES = 768 << 20
MAX_COPIES = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--topics", type=int, default=100_000)
    ap.add_argument("--partitions", type=int, default=256)
    ap.add_argument("--consumers", type=int, default=32)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--layouts", action="store_true", help="also time the two-layout form with 1 %% of the topics grown by 16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from kafka_lag_based_assignor_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("moves_probe: no GPU")
    dev = torch.device("cuda", 0)
    ctx = N.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t, p, c = args.topics, args.partitions, args.consumers
    n, k, m = t * p, t * c, c
    set_bytes = 20 * n
    copies = int(max(1, min(MAX_COPIES, -(-CACHE_PROOF_BYTES // max(16 * n, 1)))))
    rng = np.random.default_rng(1)
    part_off = np.arange(t + 1, dtype=np.int64) * p
    cons_off = np.arange(t + 1, dtype=np.int64) * c
    d_part_off, d_cons_off = torch.from_numpy(part_off).to(dev), torch.from_numpy(cons_off).to(dev)
    d_pid = torch.from_numpy(np.tile(np.arange(p, dtype=np.int32), t)).to(dev)
    d_cons = torch.from_numpy(np.tile(np.arange(c, dtype=np.int32), t)).to(dev)
    d_topic = torch.arange(t, dtype=torch.int64, device=dev).repeat_interleave(p)
    h_po = part_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    h_co = cons_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))

    results = []                                                     # copies + 1 assignments, every lag redrawn each time
    for i in range(copies + 1):
        lag = torch.from_numpy(rng.integers(0, 1 << 40, n, dtype=np.int64)).to(dev)
        out_pid = torch.empty(n, dtype=torch.int32, device=dev)
        out_rank = torch.empty(n, dtype=torch.int32, device=dev)
        b = N.DeviceBatch()
        b.n_topics, b.reset_mode, b.algo, b.flags = t, N.LA_RESET_LATEST, N.LA_ALGO_AUTO, 0
        b.n_partitions, b.n_consumers = n, k
        b.max_partitions_per_topic, b.max_consumers_per_topic = p, c
        b.d_part_off, b.d_partition_id, b.d_lag = d_part_off.data_ptr(), d_pid.data_ptr(), lag.data_ptr()
        b.d_cons_off, b.d_cons_rank = d_cons_off.data_ptr(), d_cons.data_ptr()
        b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = out_pid.data_ptr(), out_rank.data_ptr(), None
        b.h_part_off, b.h_cons_off = h_po, h_co
        torch.cuda.synchronize()
        ctx.assign_batch_device(b, stream)
        ctx.sync(stream)
        results.append((out_pid, out_rank))
        del lag
    sets = [(results[i + 1], results[i]) for i in range(copies)]    # (current, previous)
    owner = torch.empty(n, dtype=torch.int32, device=dev)
    topic_moved = torch.empty(t, dtype=torch.int64, device=dev)
    gained = torch.empty(m, dtype=torch.int64, device=dev)
    lost = torch.empty(m, dtype=torch.int64, device=dev)
    moved = torch.empty(1, dtype=torch.int64, device=dev)
    say("moves_probe: %d topics x %d partitions x %d consumers, N = %d, %d bytes per call, %d resident copies, %d launches x %d "
        "windows per side, device %s" % (t, p, c, n, set_bytes, copies, args.launches, args.windows, torch.cuda.get_device_name(0)))

    a = N.MovesArgs()
    a.n_topics, a.n_partitions, a.max_partitions_per_topic = t, n, p
    a.d_part_off, a.h_part_off, a.n_members = d_part_off.data_ptr(), h_po, m
    a.d_prev_owner, a.d_topic_moved = owner.data_ptr(), topic_moved.data_ptr()
    a.d_member_gained, a.d_member_lost, a.d_moved = gained.data_ptr(), lost.data_ptr(), moved.data_ptr()

    def lib_call(i):
        (cp, cr), (pp, pr) = sets[i % copies]
        a.d_out_partition, a.d_out_member_rank = cp.data_ptr(), cr.data_ptr()
        a.d_prev_partition, a.d_prev_member_rank = pp.data_ptr(), pr.data_ptr()
        ctx.assignment_moves_device(a, stream)

    def torch_call(i):
        (cp, cr), (pp, pr) = sets[i % copies]
        by_cur = torch.argsort((d_topic << 32) | (cp.to(torch.int64) & 0xFFFFFFFF))
        by_prev = torch.argsort((d_topic << 32) | (pp.to(torch.int64) & 0xFFFFFFFF))
        own = torch.empty(n, dtype=torch.int32, device=dev)
        own[by_cur] = pr[by_prev]
        mv = own != cr
        tm = torch.bincount(d_topic[mv], minlength=t)
        g = torch.bincount(cr[mv & (cr >= 0)], minlength=m)
        lo = torch.bincount(own[mv & (own >= 0)], minlength=m)
        return own, tm, g, lo, mv.sum()

    grown = None
    if args.layouts:
        # today's layout: every 100th topic has 16 more partitions; assigned once, joined against each resident previous copy
        from kafka_lag_based_assignor_amd import sharding
        sizes = np.full(t, p, dtype=np.int64)
        sizes[::100] += 16
        g_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        g_n = int(g_off[-1])
        g_pid = (np.arange(g_n, dtype=np.int64) - np.repeat(g_off[:-1], sizes)).astype(np.int32)
        d_g_off, d_g_pid = torch.from_numpy(g_off).to(dev), torch.from_numpy(g_pid).to(dev)
        g_lag = torch.from_numpy(rng.integers(0, 1 << 40, g_n, dtype=np.int64)).to(dev)
        g_out = (torch.empty(g_n, dtype=torch.int32, device=dev), torch.empty(g_n, dtype=torch.int32, device=dev))
        b = N.DeviceBatch()
        b.n_topics, b.reset_mode, b.algo, b.flags = t, N.LA_RESET_LATEST, N.LA_ALGO_AUTO, 0
        b.n_partitions, b.n_consumers = g_n, k
        b.max_partitions_per_topic, b.max_consumers_per_topic = p + 16, c
        b.d_part_off, b.d_partition_id, b.d_lag = d_g_off.data_ptr(), d_g_pid.data_ptr(), g_lag.data_ptr()
        b.d_cons_off, b.d_cons_rank = d_cons_off.data_ptr(), d_cons.data_ptr()
        b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = g_out[0].data_ptr(), g_out[1].data_ptr(), None
        b.h_part_off, b.h_cons_off = g_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), h_co
        torch.cuda.synchronize()
        ctx.assign_batch_device(b, stream)
        ctx.sync(stream)
        del g_lag
        g_owner = torch.empty(g_n, dtype=torch.int32, device=dev)
        g_topic = [torch.empty(t, dtype=torch.int64, device=dev) for _ in range(3)]
        g_counts = torch.empty(3, dtype=torch.int64, device=dev)
        g_gl = (torch.empty(m, dtype=torch.int64, device=dev), torch.empty(m, dtype=torch.int64, device=dev))
        g = N.MovesArgs()
        g.n_topics, g.n_partitions, g.max_partitions_per_topic = t, g_n, p + 16
        g.d_part_off, g.n_members = d_g_off.data_ptr(), m
        g.d_out_partition, g.d_out_member_rank = g_out[0].data_ptr(), g_out[1].data_ptr()
        g.n_prev_topics, g.n_prev_partitions, g.d_prev_part_off = t, n, d_part_off.data_ptr()
        g.d_prev_owner, g.d_topic_moved, g.d_topic_added, g.d_topic_removed = [x.data_ptr() for x in [g_owner] + g_topic]
        g.d_member_gained, g.d_member_lost = g_gl[0].data_ptr(), g_gl[1].data_ptr()
        g.d_moved, g.d_added, g.d_removed = [g_counts.data_ptr() + 8 * i for i in range(3)]

        def grown(i):
            pp, pr = sets[i % copies][1]
            g.d_prev_partition, g.d_prev_member_rank = pp.data_ptr(), pr.data_ptr()
            ctx.assignment_moves_device(g, stream)

        grown(0)
        g_launches = ctx.last_launches()
        ctx.sync(stream)
        exp = sharding.assignment_moves_layouts_numpy(g_off, g_out[0].cpu().numpy(), g_out[1].cpu().numpy(), part_off,
                                                      sets[0][1][0].cpu().numpy(), sets[0][1][1].cpu().numpy(), m)
        got = [g_owner] + g_topic + list(g_gl)
        g_same = all(np.array_equal(a.cpu().numpy(), e) for a, e in zip(got, exp[:6])) and g_counts.cpu().tolist() == list(exp[6:])
        g_bytes = 8 * g_n + 8 * n + 4 * g_n
        del exp

    lib_call(0)
    launches = ctx.last_launches()
    ctx.sync(stream)
    ref = torch_call(0)
    same = (bool(torch.equal(ref[0], owner)) and bool(torch.equal(ref[1], topic_moved)) and bool(torch.equal(ref[2], gained)) and
            bool(torch.equal(ref[3], lost)) and int(ref[4]) == int(moved[0]))
    share = int(moved[0]) / max(n, 1)
    del ref

    def window(call, i0):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.launches):
            call(i0 + i)
        e1.record()
        torch.cuda.synchronize()
        return float(e0.elapsed_time(e1)) * 1e3 / args.launches

    for call in (lib_call, torch_call):                             # warm-up: every copy, both sides
        for i in range(2 * copies):
            call(i)
    torch.cuda.synchronize()
    t_lib, t_torch, t_grown = [], [], []
    if grown:
        for i in range(2 * copies):
            grown(i)
    for w in range(args.windows):
        t_lib.append(window(lib_call, w * args.launches))
        if grown:
            t_grown.append(window(grown, w * args.launches))
        t_torch.append(window(torch_call, w * args.launches))
    ctx.sync(stream)
    lib_med, torch_med = float(np.median(t_lib)), float(np.median(t_torch))
    spread = max(max(t_lib) - min(t_lib), max(t_torch) - min(t_torch))
    not_slower = lib_med <= torch_med + spread
    floor_us = set_bytes / HBM_BYTES_PER_S * 1e6
    say("library %.1f us per call (min %.1f .. max %.1f; %d kernel launch(es) behind the memsets), torch restatement %.1f us "
        "(min %.1f .. max %.1f); results %s; %.1f %% of the entries moved; streaming floor %.1f us, the library runs at %.2f of "
        "it (%.2f TB/s); library not slower than torch: %s"
        % (lib_med, min(t_lib), max(t_lib), launches, torch_med, min(t_torch), max(t_torch), "equal" if same else "DIFFER",
           100.0 * share, floor_us, floor_us / lib_med, set_bytes / lib_med * 1e6 / 1e12, "yes" if not_slower else "NO"))
    if grown:
        g_med = float(np.median(t_grown))
        say("two layouts (%d of %d topics grown by 16, N = %d against N_prev = %d): %.1f us per call (min %.1f .. max %.1f; %d "
            "kernel launch(es)), %.2f x the one-layout call in the same windows; %d added, %d removed, %d moved; results %s; %d "
            "bytes per call, %.2f TB/s"
            % (len(range(0, t, 100)), t, g_n, n, g_med, min(t_grown), max(t_grown), g_launches, g_med / lib_med,
               int(g_counts[1]), int(g_counts[2]), int(g_counts[0]), "equal the host restatement" if g_same else "DIFFER",
               g_bytes, g_bytes / g_med * 1e6 / 1e12))
        same = same and g_same
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if (same and not_slower) else 1)


if __name__ == "__main__":
    main()
