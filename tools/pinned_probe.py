#!/usr/bin/env python3
"""Time the pinned assignment against the assign call on the same batch, and the host call with and without LA_COOP_PINNED:

    python tools/pinned_probe.py [--launches 10 --windows 5] [--out profiles/pinned_probe.txt]

  device  la_assign_pinned_device against la_assign_batch_device (the baseline: the code every rebalance runs today) on the same
          device-resident batch, 1 000 topics x 256 partitions x 32 consumers and 200 x 4 096 x 128, lags uniform in
          [0, 100 000), with 5 %, 50 % and 100 % of the partitions free.  The owned lists are the assign call's own result with
          the free share taken out at random, grouped by member; 5 % is the shape of a follow-up.  With everything free the two
          results are compared bit for bit; otherwise the first 16 topics are compared with sharding.assign_pinned_numpy.
  host    la_assign_batch_cooperative with and without LA_COOP_PINNED on pageable numpy arrays, 100, 1 000 and 2 048 partitions
          (topics of 25, at 2 048 of 32; 8 consumers), 5 % free, wall clock around calls that wait for their result.

Both sides of a comparison alternate in one process: after a warm-up, `windows` windows per side of `launches` back-to-back calls,
a window between one pair of HIP events (device) or on the wall clock (host).  Prints the median window and the range, per call
in microseconds.  A record: no threshold hangs on a time.  Exit status 1 only when results differ.  Needs a GPU."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch_of(seed, t, p, c):
    rng = np.random.default_rng(seed)
    part_off = np.arange(t + 1, dtype=np.int64) * p
    cons_off = np.arange(t + 1, dtype=np.int64) * c
    pid = np.concatenate([rng.permutation(p) for _ in range(t)]).astype(np.int32)
    lag = rng.integers(0, 100000, t * p).astype(np.int64)
    return part_off, pid, lag, cons_off, np.tile(np.arange(c, dtype=np.int32), t)


def owned_of(rng, sharding, part_off, out_pid, out_rank, m, free):
    """The result grouped by member with a share `free` of the partitions owned by nobody."""
    rank = np.where(rng.random(out_rank.size) < free, -1, out_rank) if free < 1.0 else np.full(out_rank.size, -1, np.int32)
    return sharding.group_by_member_numpy(part_off, out_pid, rank, m)


def large(args):
    """--large: la_assign_pinned_device with LA_FLAG_PINNED_LARGE against la_assign_batch_device on the same resident batch."""
    import torch
    from kafka_lag_based_assignor_amd import _native as N
    from kafka_lag_based_assignor_amd import sharding
    if not torch.cuda.is_available():
        sys.exit("pinned_probe: no GPU")
    dev = torch.device("cuda", 0)
    ctx = N.Context(0)
    lib, h = N.load(), ctx._h
    stream = torch.cuda.current_stream().cuda_stream
    sp = ctypes.c_void_p(stream)
    lines, ok = [], True

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def window(f, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            assert f() == 0, lib.la_last_error(h)
        e1.record()
        ctx.sync(stream)
        return float(e0.elapsed_time(e1)) * 1e3 / launches

    fmt = lambda v: "%.1f us per call (min %.1f .. max %.1f)" % (float(np.median(v)), min(v), max(v))
    say("pinned_probe --large: %d windows per side of %d calls (HIP events), sides alternating in one process, device %s; "
        "LA_FLAG_PINNED_LARGE, at most %d + %d launches" % (args.windows, args.launches, torch.cuda.get_device_name(0),
                                                            N.PINNED_MAX_LAUNCHES, N.PINNED_LARGE_LAUNCHES))
    for t, p, c, frees in ((1, 100000, 64, (0.05, 1.0)), (1, 1000000, 600, (0.05, 1.0, "joiner")), (64, 8192, 32, (0.05, 1.0)),
                           (1000, 256, 32, (0.05, 1.0))):
        part_off, pid, lag, cons_off, cons_rank = batch_of(t + p, t, p, c)
        n, k = pid.size, cons_rank.size
        d = [torch.from_numpy(x).to(dev) for x in (part_off, pid, lag, cons_off, cons_rank)]

        def batch(out, flags=0):
            b = N.DeviceBatch()
            b.n_topics, b.reset_mode, b.algo, b.flags = t, N.LA_RESET_LATEST, N.LA_ALGO_AUTO, flags
            b.n_partitions, b.n_consumers, b.max_partitions_per_topic, b.max_consumers_per_topic = n, k, p, c
            b.d_part_off, b.d_partition_id, b.d_lag, b.d_cons_off, b.d_cons_rank = [x.data_ptr() for x in d]
            b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = [x.data_ptr() for x in out]
            b.h_part_off = part_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
            b.h_cons_off = cons_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
            return b

        outs = lambda: [torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev),
                        torch.full((k,), -7, dtype=torch.int64, device=dev)]
        base_out, pin_out, plain_out = outs(), outs(), outs()
        b_base, b_pin, b_plain = batch(base_out), batch(pin_out, N.LA_FLAG_PINNED_LARGE), batch(plain_out)
        torch.cuda.synchronize()
        assert lib.la_assign_batch_device(h, ctypes.byref(b_base), sp) == 0, lib.la_last_error(h)
        base_launches = ctx.last_launches()
        ctx.sync(stream)
        base = [x.cpu().numpy() for x in base_out]
        rng = np.random.default_rng(p)
        for free in frees:
            if free == "joiner":                                          # one member joined: it holds nothing, everyone else keeps theirs
                owned = sharding.group_by_member_numpy(part_off, base[0], np.where(base[1] == 7, -1, base[1]), c)
            else:
                owned = owned_of(rng, sharding, part_off, base[0], base[1], c, free)
            d_owned = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in owned]
            free_t, summary = torch.zeros(t, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
            a = N.PinnedArgs()
            a.struct_size, a.n_members, a.n_owned = ctypes.sizeof(N.PinnedArgs), c, n
            a.d_owned_member_off, a.d_owned_topic, a.d_owned_partition = [x.data_ptr() for x in d_owned]
            a.d_topic_free, a.d_summary = free_t.data_ptr(), summary.data_ptr()
            pinned_call = lambda: lib.la_assign_pinned_device(h, ctypes.byref(b_pin), ctypes.byref(a), sp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert pinned_call() == 0, lib.la_last_error(h)
            pin_launches = ctx.last_launches()
            ctx.sync(stream)
            first_call = time.perf_counter() - t0
            got = [x.cpu().numpy() for x in pin_out]
            if free == 1.0:
                same = all(np.array_equal(g, e) for g, e in zip(got, base))
            else:
                t4 = min(t, 4)
                n4, k4 = t4 * p, t4 * c
                exp = sharding.assign_pinned_numpy(part_off[:t4 + 1], pid[:n4], lag[:n4], cons_off[:t4 + 1], cons_rank[:k4], c, owned[0],
                                                   np.where(owned[1] < t4, owned[1], -1), owned[2], max_partitions=sharding.PINNED_ANY_SIZE)
                same = all(np.array_equal(g[:s], e) for g, e, s in zip(got, exp[:3], (n4, n4, k4)))
            ok = ok and same
            s = summary.cpu().numpy()
            launches = args.launches if first_call < 0.25 else max(1, args.launches // 5)      # (a call of seconds: shorter windows, said below)
            sides = {"assign": lambda: lib.la_assign_batch_device(h, ctypes.byref(b_base), sp), "pinned": pinned_call}
            if p <= N.PINNED_MAX_PARTITIONS:                             # no large topic: the unflagged call is the third side
                sides["unflagged"] = lambda: lib.la_assign_pinned_device(h, ctypes.byref(b_plain), ctypes.byref(a), sp)
            for f in sides.values():
                window(f, 1)
            times = {k_: [] for k_ in sides}
            for _ in range(args.windows):
                for k_, f in sides.items():
                    times[k_].append(window(f, launches))
            what = "joining member" if free == "joiner" else "%3.0f %% free" % (100 * free)
            say("device, %d x %d x %d, %s (pinned %d, free %d), windows of %d calls: la_assign_batch_device %s, %d launches; flagged "
                "la_assign_pinned_device %s, %d launches; pinned / assign = %.2f%s; results %s" % (
                    t, p, c, what, int(s[0]), int(s[1]), launches, fmt(times["assign"]), base_launches, fmt(times["pinned"]), pin_launches,
                    float(np.median(times["pinned"])) / float(np.median(times["assign"])),
                    "; unflagged la_assign_pinned_device %s" % fmt(times["unflagged"]) if "unflagged" in times else "",
                    "agree" if same else "DIFFER"))
    ctx.close()
    out = args.out or os.path.join(ROOT, "profiles", "pinned_large_probe.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--large", action="store_true", help="LA_FLAG_PINNED_LARGE: topics over the LDS limit; writes profiles/pinned_large_probe.txt")
    args = ap.parse_args()
    if args.large:
        return large(args)

    import torch
    from kafka_lag_based_assignor_amd import _native as N
    from kafka_lag_based_assignor_amd import sharding
    if not torch.cuda.is_available():
        sys.exit("pinned_probe: no GPU")
    dev = torch.device("cuda", 0)
    ctx = N.Context(0)
    lib, h = N.load(), ctx._h
    stream = torch.cuda.current_stream().cuda_stream
    sp = ctypes.c_void_p(stream)
    lines, ok = [], True

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def windows(sides, timer):
        for f in sides.values():                                         # warm-up
            timer(f)
        times = {k: [] for k in sides}
        for _ in range(args.windows):
            for k, f in sides.items():
                times[k].append(timer(f))
        return times

    def device_window(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            assert f() == 0, lib.la_last_error(h)
        e1.record()
        ctx.sync(stream)
        return float(e0.elapsed_time(e1)) * 1e3 / args.launches

    def host_window(f):
        t0 = time.perf_counter()
        for _ in range(args.launches):
            assert f() == 0, lib.la_last_error(h)
        return (time.perf_counter() - t0) * 1e6 / args.launches

    fmt = lambda v: "%.1f us per call (min %.1f .. max %.1f)" % (float(np.median(v)), min(v), max(v))
    say("pinned_probe: %d windows per side of %d calls, sides alternating in one process, device %s; limits %d partitions x %d consumers"
        % (args.windows, args.launches, torch.cuda.get_device_name(0), N.PINNED_MAX_PARTITIONS, N.PINNED_MAX_CONSUMERS))

    # ---- the device call ----------------------------------------------------------------------------------------------------------
    for t, p, c in ((1000, 256, 32), (200, 4096, 128)):
        part_off, pid, lag, cons_off, cons_rank = batch_of(t + p, t, p, c)
        n, k = pid.size, cons_rank.size
        d = [torch.from_numpy(x).to(dev) for x in (part_off, pid, lag, cons_off, cons_rank)]

        def batch(out):
            b = N.DeviceBatch()
            b.n_topics, b.reset_mode, b.algo = t, N.LA_RESET_LATEST, N.LA_ALGO_AUTO
            b.n_partitions, b.n_consumers, b.max_partitions_per_topic, b.max_consumers_per_topic = n, k, p, c
            b.d_part_off, b.d_partition_id, b.d_lag, b.d_cons_off, b.d_cons_rank = [x.data_ptr() for x in d]
            b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = [x.data_ptr() for x in out]
            b.h_part_off = part_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
            b.h_cons_off = cons_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
            return b

        outs = lambda: [torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev),
                        torch.full((k,), -7, dtype=torch.int64, device=dev)]
        base_out, pin_out = outs(), outs()
        b_base, b_pin = batch(base_out), batch(pin_out)
        torch.cuda.synchronize()
        assert lib.la_assign_batch_device(h, ctypes.byref(b_base), sp) == 0, lib.la_last_error(h)
        base_launches = ctx.last_launches()
        ctx.sync(stream)
        base = [x.cpu().numpy() for x in base_out]
        rng = np.random.default_rng(p)
        for free in (0.05, 0.5, 1.0):
            owned = owned_of(rng, sharding, part_off, base[0], base[1], c, free)
            d_owned = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in owned]
            free_t, summary = torch.zeros(t, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
            a = N.PinnedArgs()
            a.struct_size, a.n_members, a.n_owned = ctypes.sizeof(N.PinnedArgs), c, n
            a.d_owned_member_off, a.d_owned_topic, a.d_owned_partition = [x.data_ptr() for x in d_owned]
            a.d_topic_free, a.d_summary = free_t.data_ptr(), summary.data_ptr()
            pinned_call = lambda: lib.la_assign_pinned_device(h, ctypes.byref(b_pin), ctypes.byref(a), sp)
            torch.cuda.synchronize()
            assert pinned_call() == 0, lib.la_last_error(h)
            pin_launches = ctx.last_launches()
            ctx.sync(stream)
            got = [x.cpu().numpy() for x in pin_out]
            if free == 1.0:
                same = all(np.array_equal(g, e) for g, e in zip(got, base))
            else:
                t16, n16, k16 = 16, 16 * p, 16 * c
                exp = sharding.assign_pinned_numpy(part_off[:t16 + 1], pid[:n16], lag[:n16], cons_off[:t16 + 1], cons_rank[:k16], c,
                                                   owned[0], np.where(owned[1] < t16, owned[1], -1), owned[2])
                same = all(np.array_equal(g[:s], e) for g, e, s in zip(got, exp[:3], (n16, n16, k16)))
            ok = ok and same
            s = summary.cpu().numpy()
            times = windows({"assign": lambda: lib.la_assign_batch_device(h, ctypes.byref(b_base), sp), "pinned": pinned_call}, device_window)
            say("device, %d x %d x %d, %3.0f %% free (pinned %d, free %d): la_assign_batch_device %s, %d launches; la_assign_pinned_device %s, "
                "%d launches; pinned / assign = %.2f; results %s" % (
                    t, p, c, 100 * free, int(s[0]), int(s[1]), fmt(times["assign"]), base_launches, fmt(times["pinned"]), pin_launches,
                    float(np.median(times["pinned"])) / float(np.median(times["assign"])), "agree" if same else "DIFFER"))

    # ---- the host call ------------------------------------------------------------------------------------------------------------
    for n_want in (100, 1000, 2048):
        p = 25 if n_want % 25 == 0 else 32
        t, c = n_want // p, 8
        part_off, pid, lag, cons_off, cons_rank = batch_of(n_want, t, p, c)
        target = ctx.assign_batch_lags(part_off, pid, lag, cons_off, cons_rank)
        owned = owned_of(np.random.default_rng(n_want), sharding, part_off, target[0], target[1], c, 0.05)
        keep = [np.ascontiguousarray(x) for x in (part_off, pid, cons_off, cons_rank, lag) + tuple(owned)]
        g_full, g_pin = N.AssignCoopArgs(), N.AssignCoopArgs()
        fill = lambda g: ctx._fill_assign_coop(g, keep[0], keep[1], keep[2], keep[3], c, keep[5], keep[6], keep[7], keep[4], None, None,
                                               None, 0, None, None, False, None)
        out_full, out_pin = fill(g_full), fill(g_pin)
        g_pin.flags |= N.LA_COOP_PINNED
        sides = {"full": lambda: lib.la_assign_batch_cooperative(h, ctypes.byref(g_full)),
                 "pinned": lambda: lib.la_assign_batch_cooperative(h, ctypes.byref(g_pin))}
        launches = {}
        for name, f in sides.items():
            assert f() == 0, lib.la_last_error(h)
            launches[name] = ctx.last_launches()
        pin3 = sharding.assign_pinned_numpy(part_off, pid, lag, cons_off, cons_rank, c, *owned)[:3]
        exp = sharding.assign_cooperative_numpy(part_off, pid, lag, cons_off, cons_rank, c, *owned, assign=lambda *x: pin3)
        same = all(np.array_equal(g, e) for g, e in zip(out_pin, exp))
        ok = ok and same
        times = windows(sides, host_window)
        say("host, N = %d (T = %d, 8 consumers), 5 %% free, wall clock: full form %s, %d launches, withheld %d; LA_COOP_PINNED %s, "
            "%d launches, withheld %d; pinned / full = %.2f; results %s" % (
                part_off[-1], t, fmt(times["full"]), launches["full"], int(out_full.summary[2]), fmt(times["pinned"]), launches["pinned"],
                int(out_pin.summary[2]), float(np.median(times["pinned"])) / float(np.median(times["full"])), "agree" if same else "DIFFER"))
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
