#!/usr/bin/env python3
"""Time la_verify_assignment_device beside the la_assign_batch_device call it certifies.

    python tools/verify_probe.py [--topics 100000 --partitions 256 --consumers 32 --launches 20 --windows 5] [--out FILE]
    python tools/verify_probe.py --large [--large-shapes 1x10000x128,1x1048576x8192] [--launches 5 --windows 5] [--out FILE]

The layout is T topics x P partitions x C consumers (the bench's target shape by default), lags from begin / end / committed
offsets (EARLIEST, 1 % of the partitions without a committed offset), in enough resident copies that a call never finds its
inputs in the 256 MiB Infinity Cache (768 MB between two touches of one copy).  Every copy is assigned once and verified once
first: the verdicts must all be zero.  Then `windows` timed windows per side, assign and verify alternating, each ONE pair of HIP
events around `launches` back-to-back calls on one stream, on the same batches in the same process.

Prints the median and the spread (min .. max) of both calls in microseconds, their ratio, the bytes the verify call must move
((36 + 8 + 8 K / N) B per partition: inputs, the two result arrays, the totals) and its streaming floor at 8 TB/s.  Exit status 1
when a result is not certified.  Needs a GPU: there is nothing to fall back to.

--large is the leg for topics over the 4 096 x 4 096 limit of the LDS form: per shape (T x P x C; cfg2b and cfg5 of BASELINE.md by
default) the same method on ONE resident batch with LA_FLAG_VERIFY_LARGE set, so the verify call goes through the global form
(tables in device memory); the assign call ignores the flag.  It prints the pair and its ratio per shape, and the launches.
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


def large_leg(args, say):
    """The flagged verify call beside the assign call it certifies, per shape: alternating windows, one pair of events each."""
    import torch
    from kafka_lag_based_assignor_amd import _native as N
    dev = torch.device("cuda", 0)
    ctx = N.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    i64p = ctypes.POINTER(ctypes.c_int64)
    all_certified = True
    for spec in args.large_shapes.split(","):
        t, p, c = (int(x) for x in spec.lower().split("x"))
        n, k = t * p, t * c
        rng = np.random.default_rng(2)
        part_off, cons_off = np.arange(t + 1, dtype=np.int64) * p, np.arange(t + 1, dtype=np.int64) * c
        lag = rng.integers(0, 1 << 40, n, dtype=np.int64)
        committed = rng.integers(0, 1 << 40, n, dtype=np.int64)
        begin = rng.integers(0, 1 << 20, n, dtype=np.int64)
        none = rng.random(n) < 0.01
        committed[none] = -1
        end = np.where(none, begin, committed) + lag
        pid = np.concatenate([rng.permutation(p).astype(np.int32) for _ in range(t)])
        host = [part_off, pid, begin, end, committed, cons_off, np.tile(np.arange(c, dtype=np.int32), t)]
        d = [torch.from_numpy(a).to(dev) for a in host]
        outs = [torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty(k, dtype=torch.int64, device=dev)]
        verdict = torch.empty(t, dtype=torch.int32, device=dev)
        summary = torch.empty(4, dtype=torch.int64, device=dev)
        b = N.DeviceBatch()
        b.n_topics, b.reset_mode, b.algo, b.flags = t, N.LA_RESET_EARLIEST, N.LA_ALGO_AUTO, N.LA_FLAG_VERIFY_LARGE
        b.n_partitions, b.n_consumers = n, k
        b.max_partitions_per_topic, b.max_consumers_per_topic = p, c
        b.d_part_off, b.d_partition_id, b.d_begin_off, b.d_end_off, b.d_committed_off, b.d_cons_off, b.d_cons_rank = (a.data_ptr() for a in d)
        b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = (a.data_ptr() for a in outs)
        b.h_part_off, b.h_cons_off = part_off.ctypes.data_as(i64p), cons_off.ctypes.data_as(i64p)

        def assign_call():
            ctx.assign_batch_device(b, stream)

        def verify_call():
            ctx.verify_assignment_device(b, verdict.data_ptr(), summary.data_ptr(), stream)

        torch.cuda.synchronize()
        assign_call()
        a_launches = ctx.last_launches()
        verify_call()                                                # behind it on the stream; the first call also grows the scratch
        v_launches = ctx.last_launches()
        ctx.sync(stream)
        s4 = summary.cpu().numpy()
        certified = list(s4) == [0, 0, -1, -1] and not bool(verdict.any())
        all_certified = all_certified and certified

        def window(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                call()
            e1.record()
            torch.cuda.synchronize()
            return float(e0.elapsed_time(e1)) * 1e3 / args.launches

        for call in (assign_call, verify_call):                      # warm-up
            call()
            call()
        torch.cuda.synchronize()
        t_a, t_v = [], []
        for _ in range(args.windows):
            t_a.append(window(assign_call))
            t_v.append(window(verify_call))
        ctx.sync(stream)
        a_med, v_med = float(np.median(t_a)), float(np.median(t_v))
        say("large leg %d x %d x %d (LA_FLAG_VERIFY_LARGE, %d launches x %d windows per side, alternating): assign %.1f us per call "
            "(min %.1f .. max %.1f; %d kernel launch(es)), verify %.1f us per call (min %.1f .. max %.1f; %d kernel launch(es) behind the "
            "memsets and the list copy); verify / assign = %.2f; results %s (summary %s)"
            % (t, p, c, args.launches, args.windows, a_med, min(t_a), max(t_a), a_launches, v_med, min(t_v), max(t_v), v_launches,
               v_med / a_med, "certified" if certified else "NOT CERTIFIED", list(s4)))
        del d, outs, verdict, summary
    ctx.close()
    return all_certified


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--topics", type=int, default=100_000)
    ap.add_argument("--partitions", type=int, default=256)
    ap.add_argument("--consumers", type=int, default=32)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--large", action="store_true", help="the leg for topics over the LDS form's limit (LA_FLAG_VERIFY_LARGE)")
    ap.add_argument("--large-shapes", default="1x10000x128,1x1048576x8192")
    args = ap.parse_args()

    import torch
    from kafka_lag_based_assignor_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("verify_probe: no GPU")
    dev = torch.device("cuda", 0)
    ctx = N.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.large:
        ctx.close()
        say("verify_probe --large: device %s" % torch.cuda.get_device_name(0))
        certified = large_leg(args, say)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
        sys.exit(0 if certified else 1)

    t, p, c = args.topics, args.partitions, args.consumers
    n, k = t * p, t * c
    call_bytes = 44 * n + 8 * k
    copies = int(max(1, min(MAX_COPIES, -(-CACHE_PROOF_BYTES // max(call_bytes, 1)))))
    rng = np.random.default_rng(1)
    part_off = np.arange(t + 1, dtype=np.int64) * p
    cons_off = np.arange(t + 1, dtype=np.int64) * c
    d_part_off, d_cons_off = torch.from_numpy(part_off).to(dev), torch.from_numpy(cons_off).to(dev)
    d_pid = torch.from_numpy(np.tile(np.arange(p, dtype=np.int32), t)).to(dev)
    d_cons = torch.from_numpy(np.tile(np.arange(c, dtype=np.int32), t)).to(dev)
    h_po = part_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    h_co = cons_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    verdict = torch.empty(max(t, 1), dtype=torch.int32, device=dev)
    summary = torch.empty(4, dtype=torch.int64, device=dev)

    batches, keep = [], []
    for i in range(copies):
        lag = rng.integers(0, 1 << 40, n, dtype=np.int64)
        committed = rng.integers(0, 1 << 40, n, dtype=np.int64)
        begin = rng.integers(0, 1 << 20, n, dtype=np.int64)
        none = rng.random(n) < 0.01
        committed[none] = -1
        end = np.where(none, begin, committed) + lag
        arrays = [torch.from_numpy(a).to(dev) for a in (begin, end, committed)]
        outs = [torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty(k, dtype=torch.int64, device=dev)]
        b = N.DeviceBatch()
        b.n_topics, b.reset_mode, b.algo, b.flags = t, N.LA_RESET_EARLIEST, N.LA_ALGO_AUTO, 0
        b.n_partitions, b.n_consumers = n, k
        b.max_partitions_per_topic, b.max_consumers_per_topic = p, c
        b.d_part_off, b.d_partition_id = d_part_off.data_ptr(), d_pid.data_ptr()
        b.d_begin_off, b.d_end_off, b.d_committed_off = (a.data_ptr() for a in arrays)
        b.d_cons_off, b.d_cons_rank = d_cons_off.data_ptr(), d_cons.data_ptr()
        b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = (a.data_ptr() for a in outs)
        b.h_part_off, b.h_cons_off = h_po, h_co
        batches.append(b)
        keep.append((arrays, outs))
    say("verify_probe: %d topics x %d partitions x %d consumers, N = %d, %d bytes per verify call, %d resident copies, %d launches x "
        "%d windows per side, device %s" % (t, p, c, n, call_bytes, copies, args.launches, args.windows, torch.cuda.get_device_name(0)))

    def assign_call(i):
        ctx.assign_batch_device(batches[i % copies], stream)

    def verify_call(i):
        ctx.verify_assignment_device(batches[i % copies], verdict.data_ptr(), summary.data_ptr(), stream)

    torch.cuda.synchronize()
    certified, launches = True, (0, 0)
    for i in range(copies):                                          # assign, then verify behind it on the stream: all zero
        assign_call(i)
        a_launches = ctx.last_launches()
        verify_call(i)
        launches = (a_launches, ctx.last_launches())
        ctx.sync(stream)
        s = summary.cpu().numpy()
        if list(s) != [0, 0, -1, -1] or bool(verdict[:t].any()):
            certified = False
            say("copy %d is NOT certified: summary %s" % (i, list(s)))

    def window(call, i0):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.launches):
            call(i0 + i)
        e1.record()
        torch.cuda.synchronize()
        return float(e0.elapsed_time(e1)) * 1e3 / args.launches

    for call in (assign_call, verify_call):                          # warm-up: every copy, both sides
        for i in range(2 * copies):
            call(i)
    torch.cuda.synchronize()
    t_assign, t_verify = [], []
    for w in range(args.windows):
        t_assign.append(window(assign_call, w * args.launches))
        t_verify.append(window(verify_call, w * args.launches))
    ctx.sync(stream)
    a_med, v_med = float(np.median(t_assign)), float(np.median(t_verify))
    floor_us = call_bytes / HBM_BYTES_PER_S * 1e6
    say("assign %.1f us per call (min %.1f .. max %.1f; %d kernel launch(es)), verify %.1f us per call (min %.1f .. max %.1f; %d "
        "kernel launch(es) behind the memsets); verify / assign = %.2f; results %s; streaming floor of the verify call %.1f us, it "
        "runs at %.2f of it (%.2f TB/s)"
        % (a_med, min(t_assign), max(t_assign), launches[0], v_med, min(t_verify), max(t_verify), launches[1], v_med / a_med,
           "certified" if certified else "NOT CERTIFIED", floor_us, floor_us / v_med, call_bytes / v_med * 1e6 / 1e12))
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if certified else 1)


if __name__ == "__main__":
    main()
