#!/usr/bin/env python3
"""Time la_sticky_ties_device beside la_verify_assignment_device on the same batches, and count what it keeps.

    python tools/sticky_probe.py [--topics 100000 --partitions 256 --consumers 32 --rate 0.01 --launches 10 --windows 5] [--out FILE]

The layout is T topics x P partitions x C consumers (the bench's target shape by default) of a group that has caught up: every
lag 0 but for a share `rate` of the partitions.  Per resident copy two draws of the lagging partitions are assigned on the
device, the first as the previous rebalance and the second as today's; la_assignment_moves_device between them writes
d_prev_owner.  One call reads and writes 28 B per partition, so a single copy already exceeds the 256 MiB Infinity Cache; the
copies are rotated all the same.  Verify is the yardstick because it does the same join, lag read and LDS residency.

Every copy is re-matched once first and its sticky order verified: each topic must read 0 or LA_VERDICT_ORDER.  Then `windows`
timed windows per side, sticky and verify alternating, each ONE pair of HIP events around `launches` back-to-back calls on one
stream.  Prints the median and the spread of both calls in microseconds, their ratio, and kept before / kept after of the
first copy as shares of its entries.  Exit status 1 when a sticky order does not verify.  Needs a GPU: there is nothing to fall
back to.

    python tools/sticky_probe.py --large [--launches 10 --windows 5] [--out profiles/sticky_large_probe.txt]

The LARGE cases (LA_FLAG_STICKY_LARGE): one topic of 100 000 x 64 and one of 1 000 000 x 600, 1 % lagging, and 64 topics of
8 192 x 32.  Per case: time per call flagged (the global form re-matches the large topics) and unflagged (they are passed
through), kept before / after of both, the launches of both, and the same batch through la_verify_assignment_device with
LA_FLAG_VERIFY_LARGE; the flagged sticky order must verify as 0 or LA_VERDICT_ORDER.  Last a batch WITHOUT a large topic,
flagged against unflagged."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_COPIES = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--topics", type=int, default=100_000)
    ap.add_argument("--partitions", type=int, default=256)
    ap.add_argument("--consumers", type=int, default=32)
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--copies", type=int, default=2)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--large", action="store_true", help="the large cases (LA_FLAG_STICKY_LARGE) instead of the T x P x C batch")
    args = ap.parse_args()
    if args.large:
        return large_main(args)

    import torch
    from kafka_lag_based_assignor_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("sticky_probe: no GPU")
    dev = torch.device("cuda", 0)
    ctx = N.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t, p, c = args.topics, args.partitions, args.consumers
    n, k = t * p, t * c
    copies = max(1, min(MAX_COPIES, args.copies))
    rng = np.random.default_rng(1)
    part_off = np.arange(t + 1, dtype=np.int64) * p
    cons_off = np.arange(t + 1, dtype=np.int64) * c
    d_part_off, d_cons_off = torch.from_numpy(part_off).to(dev), torch.from_numpy(cons_off).to(dev)
    d_pid = torch.from_numpy(np.tile(np.arange(p, dtype=np.int32), t)).to(dev)
    d_cons = torch.from_numpy(np.tile(np.arange(c, dtype=np.int32), t)).to(dev)
    verdict = torch.empty(max(t, 1), dtype=torch.int32, device=dev)
    v_summary = torch.empty(4, dtype=torch.int64, device=dev)
    kept = torch.empty(max(t, 1), dtype=torch.int64, device=dev)
    saved = torch.empty(max(t, 1), dtype=torch.int64, device=dev)
    s_summary = torch.empty(4, dtype=torch.int64, device=dev)

    def draw():
        return np.where(rng.random(n) < args.rate, rng.integers(1, 1 << 30, n, dtype=np.int64), np.int64(0))

    def batch_of(d_lag, outs):
        b = N.DeviceBatch()
        b.n_topics, b.reset_mode, b.algo, b.flags = t, N.LA_RESET_LATEST, N.LA_ALGO_AUTO, 0
        b.n_partitions, b.n_consumers = n, k
        b.max_partitions_per_topic, b.max_consumers_per_topic = p, c
        b.d_part_off, b.d_partition_id, b.d_lag = d_part_off.data_ptr(), d_pid.data_ptr(), d_lag.data_ptr()
        b.d_cons_off, b.d_cons_rank = d_cons_off.data_ptr(), d_cons.data_ptr()
        b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = (a.data_ptr() for a in outs)
        return b

    def results():
        return [torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty(max(k, 1), dtype=torch.int64, device=dev)]

    batches, stickies, keep = [], [], []
    for i in range(copies):
        lag_prev, prev_outs = torch.from_numpy(draw()).to(dev), results()
        lag_now, outs = torch.from_numpy(draw()).to(dev), results()
        prev_owner = torch.empty(n, dtype=torch.int32, device=dev)
        sticky = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        b = batch_of(lag_now, outs)
        ctx.assign_batch_device(batch_of(lag_prev, prev_outs), stream)
        ctx.assign_batch_device(b, stream)
        m = N.MovesArgs()
        m.n_topics, m.n_partitions, m.max_partitions_per_topic = t, n, p
        m.d_part_off = d_part_off.data_ptr()
        m.d_out_partition, m.d_out_member_rank = outs[0].data_ptr(), outs[1].data_ptr()
        m.d_prev_partition, m.d_prev_member_rank = prev_outs[0].data_ptr(), prev_outs[1].data_ptr()
        m.n_members, m.n_prev_members = c, c
        m.d_prev_owner = prev_owner.data_ptr()
        ctx.assignment_moves_device(m, stream)
        ctx.sync(stream)
        a = N.StickyArgs()
        a.d_prev_owner, a.d_sticky_partition = prev_owner.data_ptr(), sticky.data_ptr()
        a.d_topic_kept, a.d_topic_saved, a.d_summary = kept.data_ptr(), saved.data_ptr(), s_summary.data_ptr()
        batches.append(b)
        stickies.append(a)
        keep.append((lag_now, outs, prev_owner, sticky))
        del lag_prev, prev_outs
    call_bytes = 28 * n
    say("sticky_probe: %d topics x %d partitions x %d consumers, %.0f %% lagging, N = %d, %d bytes per sticky call, %d resident copies, "
        "%d launches x %d windows per side, device %s" % (t, p, c, 100 * args.rate, n, call_bytes, copies, args.launches, args.windows,
                                                         torch.cuda.get_device_name(0)))

    def sticky_call(i):
        ctx.sticky_ties_device(batches[i % copies], stickies[i % copies], stream)

    def verify_call(i):
        ctx.verify_assignment_device(batches[i % copies], verdict.data_ptr(), v_summary.data_ptr(), stream)

    sound, launches, first = True, (0, 0), None
    for i in range(copies):                                          # re-match, then verify the STICKY order behind it on the stream
        sticky_call(i)
        s_launches = ctx.last_launches()
        vb = N.DeviceBatch.from_buffer_copy(batches[i])
        vb.d_out_partition = keep[i][3].data_ptr()
        ctx.verify_assignment_device(vb, verdict.data_ptr(), v_summary.data_ptr(), stream)
        launches = (s_launches, ctx.last_launches())
        ctx.sync(stream)
        s4 = [int(x) for x in s_summary.cpu().numpy()]
        first = first or s4
        bits = torch.unique(verdict[:t]).cpu().numpy().tolist()
        if not set(bits) <= {0, N.LA_VERDICT_ORDER} or int(saved[:t].min()) < 0:
            sound = False
            say("copy %d: the sticky order does NOT verify: verdict bits %s" % (i, bits))

    def window(call, i0):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.launches):
            call(i0 + i)
        e1.record()
        torch.cuda.synchronize()
        return float(e0.elapsed_time(e1)) * 1e3 / args.launches

    for call in (sticky_call, verify_call):                          # warm-up: every copy, both sides
        for i in range(2 * copies):
            call(i)
    torch.cuda.synchronize()
    t_sticky, t_verify = [], []
    for w in range(args.windows):
        t_sticky.append(window(sticky_call, w * args.launches))
        t_verify.append(window(verify_call, w * args.launches))
    ctx.sync(stream)
    s_med, v_med = float(np.median(t_sticky)), float(np.median(t_verify))
    say("sticky %.1f us per call (min %.1f .. max %.1f; %d kernel launch(es) behind the memset), verify %.1f us per call (min %.1f .. "
        "max %.1f; %d kernel launch(es)); sticky / verify = %.2f; the sticky call moves %.2f TB/s; sticky orders %s"
        % (s_med, min(t_sticky), max(t_sticky), launches[0], v_med, min(t_verify), max(t_verify), launches[1], s_med / v_med,
           call_bytes / s_med * 1e6 / 1e12, "verify as 0 or LA_VERDICT_ORDER" if sound else "DO NOT VERIFY"))
    say("copy 0: kept before %d of %d entries (%.1f %%), kept after %d (%.1f %%), topics whose order changed %d of %d, passed through %d"
        % (first[0], n, 100.0 * first[0] / max(n, 1), first[1], 100.0 * first[1] / max(n, 1), first[2], t, first[3]))
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if sound else 1)


LARGE_CASES = ((1, 100_000, 64), (1, 1_000_000, 600), (64, 8192, 32), (1000, 256, 32))      # the last: no large topic


def large_main(args):
    import ctypes
    import torch
    from kafka_lag_based_assignor_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("sticky_probe: no GPU")
    dev = torch.device("cuda", 0)
    ctx = N.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    i64p = ctypes.POINTER(ctypes.c_int64)
    lines, sound = [], True

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("sticky_probe --large: %.0f %% lagging, %d launches x %d windows per side, device %s"
        % (100 * args.rate, args.launches, args.windows, torch.cuda.get_device_name(0)))
    for t, p, c in LARGE_CASES:
        n, k = t * p, t * c
        rng = np.random.default_rng(1)
        part_off, cons_off = np.arange(t + 1, dtype=np.int64) * p, np.arange(t + 1, dtype=np.int64) * c
        d_part_off, d_cons_off = torch.from_numpy(part_off).to(dev), torch.from_numpy(cons_off).to(dev)
        d_pid = torch.from_numpy(np.tile(np.arange(p, dtype=np.int32), t)).to(dev)
        d_cons = torch.from_numpy(np.tile(np.arange(c, dtype=np.int32), t)).to(dev)
        i32 = lambda size: torch.empty(max(size, 1), dtype=torch.int32, device=dev)
        i64 = lambda size: torch.empty(max(size, 1), dtype=torch.int64, device=dev)
        verdict, v_summary, kept, saved, s_summary = i32(t), i64(4), i64(t), i64(t), i64(4)
        draw = lambda: np.where(rng.random(n) < args.rate, rng.integers(1, 1 << 30, n, dtype=np.int64), np.int64(0))

        def batch_of(d_lag, outs, flags=0):
            b = N.DeviceBatch()
            b.n_topics, b.reset_mode, b.algo, b.flags = t, N.LA_RESET_LATEST, N.LA_ALGO_AUTO, flags
            b.n_partitions, b.n_consumers, b.max_partitions_per_topic, b.max_consumers_per_topic = n, k, p, c
            b.d_part_off, b.d_partition_id, b.d_lag = d_part_off.data_ptr(), d_pid.data_ptr(), d_lag.data_ptr()
            b.d_cons_off, b.d_cons_rank = d_cons_off.data_ptr(), d_cons.data_ptr()
            b.h_part_off, b.h_cons_off = part_off.ctypes.data_as(i64p), cons_off.ctypes.data_as(i64p)
            b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = (a.data_ptr() for a in outs)
            return b

        lag_prev, prev_outs = torch.from_numpy(draw()).to(dev), [i32(n), i32(n), i64(k)]
        lag_now, outs = torch.from_numpy(draw()).to(dev), [i32(n), i32(n), i64(k)]
        prev_owner, sticky = i32(n), i32(n)
        torch.cuda.synchronize()
        ctx.assign_batch_device(batch_of(lag_prev, prev_outs), stream)
        ctx.assign_batch_device(batch_of(lag_now, outs), stream)
        m = N.MovesArgs()
        m.n_topics, m.n_partitions, m.max_partitions_per_topic = t, n, p
        m.d_part_off, m.h_part_off = d_part_off.data_ptr(), part_off.ctypes.data_as(i64p)
        m.d_out_partition, m.d_out_member_rank = outs[0].data_ptr(), outs[1].data_ptr()
        m.d_prev_partition, m.d_prev_member_rank = prev_outs[0].data_ptr(), prev_outs[1].data_ptr()
        m.n_members, m.n_prev_members = c, c
        m.d_prev_owner = prev_owner.data_ptr()
        ctx.assignment_moves_device(m, stream)
        ctx.sync(stream)
        a = N.StickyArgs()
        a.d_prev_owner, a.d_sticky_partition = prev_owner.data_ptr(), sticky.data_ptr()
        a.d_topic_kept, a.d_topic_saved, a.d_summary = kept.data_ptr(), saved.data_ptr(), s_summary.data_ptr()
        flagged, plain = batch_of(lag_now, outs, N.LA_FLAG_STICKY_LARGE), batch_of(lag_now, outs)
        vb = batch_of(lag_now, outs, N.LA_FLAG_VERIFY_LARGE)
        calls = {"flagged": lambda: ctx.sticky_ties_device(flagged, a, stream), "unflagged": lambda: ctx.sticky_ties_device(plain, a, stream),
                 "verify": lambda: ctx.verify_assignment_device(vb, verdict.data_ptr(), v_summary.data_ptr(), stream)}
        summaries, launches = {}, {}
        for name in ("unflagged", "flagged"):                        # (flagged last: its sticky order is the one verified below)
            calls[name]()
            launches[name] = ctx.last_launches()
            ctx.sync(stream)
            summaries[name] = [int(x) for x in s_summary.cpu().numpy()]
        vs = N.DeviceBatch.from_buffer_copy(vb)
        vs.d_out_partition = sticky.data_ptr()
        ctx.verify_assignment_device(vs, verdict.data_ptr(), v_summary.data_ptr(), stream)
        ctx.sync(stream)
        bits = torch.unique(verdict[:t]).cpu().numpy().tolist()
        ok = set(bits) <= {0, N.LA_VERDICT_ORDER} and int(saved[:t].min()) >= 0
        sound = sound and ok
        calls["verify"]()
        launches["verify"] = ctx.last_launches()
        ctx.sync(stream)

        def window(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                call()
            e1.record()
            torch.cuda.synchronize()
            return float(e0.elapsed_time(e1)) * 1e3 / args.launches

        times = {name: [] for name in calls}
        for _ in range(args.windows):
            for name, call in calls.items():
                times[name].append(window(call))
        ctx.sync(stream)
        med = {name: float(np.median(x)) for name, x in times.items()}
        say("%d topic(s) x %d partitions x %d consumers, N = %d: flagged %.1f us per call (min %.1f .. max %.1f; %d launches), unflagged "
            "%.1f us (min %.1f .. max %.1f; %d launch(es)), verify with LA_FLAG_VERIFY_LARGE %.1f us (min %.1f .. max %.1f; %d launches); "
            "flagged / verify = %.2f; the flagged sticky order %s"
            % (t, p, c, n, med["flagged"], min(times["flagged"]), max(times["flagged"]), launches["flagged"], med["unflagged"],
               min(times["unflagged"]), max(times["unflagged"]), launches["unflagged"], med["verify"], min(times["verify"]),
               max(times["verify"]), launches["verify"], med["flagged"] / med["verify"],
               "verifies as 0 or LA_VERDICT_ORDER" if ok else "DOES NOT VERIFY: verdict bits %s" % bits))
        f, u = summaries["flagged"], summaries["unflagged"]
        say("    kept before %d of %d (%.1f %%); kept after: flagged %d (%.1f %%, moved %d, %d topic(s) passed through), unflagged %d "
            "(%.1f %%, moved %d, %d passed through)" % (f[0], n, 100.0 * f[0] / n, f[1], 100.0 * f[1] / n, n - f[1], f[3], u[1],
                                                       100.0 * u[1] / n, n - u[1], u[3]))
        del lag_prev, prev_outs, lag_now, outs, prev_owner, sticky
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if sound else 1)


if __name__ == "__main__":
    main()
