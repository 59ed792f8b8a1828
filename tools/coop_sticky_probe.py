#!/usr/bin/env python3
"""Time the cooperative round with sticky ties of a small rebalance three ways, on the same device-resident arrays:

    python tools/coop_sticky_probe.py [--sizes 100,1000,LIMIT --batch 100 --seconds 1.0] [--out profiles/coop_sticky_probe.txt]
                                      [--host-out profiles/assign_coop_sticky_probe.txt]

  chain   la_cooperative_adjust_device (for d_prev_owner), la_sticky_ties_device, la_cooperative_round_device on the sticky
          order: the three calls a caller chained by hand before la_cooperative_round_sticky_device existed
  sticky  la_cooperative_round_sticky_device (within the limits of csrc/la_coop.h: one launch of one workgroup)
  forced  the same with LA_COOP_FORCE_TABLE (the general form: the chain behind one entry point)
  host    la_assign_batch_cooperative_sticky on pageable numpy arrays, wall clock per call, three forms alternating: as it comes
          (FUSED: the sticky round is the last launch of the zero-copy call), with LA_NO_FUSED_STICKY=1 in the environment (the
          GENERAL form: a second packing, two copies, a second wait) and la_assign_batch_cooperative (fused) on the same arrays.
          Medians and interquartile spreads in microseconds; the fused form counts as faster where the general form's median
          exceeds its own by more than the larger of the two spreads.  Both forms are compared with the model on every output.

A point is a group that has caught up, from tests/sticky_cases.py (caught_up): N entries over topics of 25 partitions (32 at the limit), 8 consumers
per topic, 1 % of the partitions lagging, two consecutive rebalances with the lagging partitions redrawn; the owned lists are the
first rebalance grouped by member, the target is the second.  The forms are compared bit for bit first, with each other and with
sharding.cooperative_round_sticky_numpy.  After a warm-up the forms ALTERNATE batch by batch inside this one process until every
form has at least `seconds` of timed batches; a batch is ONE pair of HIP events around `batch` back-to-back calls, followed by a
sync.  Prints median (min .. max) microseconds per call, the spread of each form's batches (interquartile range over the median)
and the ratio chain / sticky.  A record: no threshold hangs on a time.  Exit status 1 only when results differ.  Needs a GPU.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,1000,LIMIT")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-out", default=None, help="the host call's section alone (profiles/assign_coop_sticky_probe.txt)")
    args = ap.parse_args()

    import torch
    from kafka_lag_based_assignor_amd import _native as N
    from kafka_lag_based_assignor_amd import sharding
    import sticky_cases as S
    if not torch.cuda.is_available():
        sys.exit("coop_sticky_probe: no GPU")
    dev = torch.device("cuda", 0)
    ctx = N.Context(0)
    lib = N.load()
    stream = torch.cuda.current_stream().cuda_stream
    sp = ctypes.c_void_p(stream)
    h = ctx._h
    lines = []

    host_lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def hsay(s):                                                         # the host call's section: also a record of its own
        say(s)
        host_lines.append(s)

    say("coop_sticky_probe: batches of %d calls, at least %.1f s of timed batches per form and point, forms alternating, device %s; "
        "limits N %d, n_owned %d, M %d, T %d" % (args.batch, args.seconds, torch.cuda.get_device_name(0), N.COOP_STICKY_ENTRIES,
                                                  N.COOP_STICKY_OWNED, N.COOP_STICKY_MEMBERS, N.COOP_STICKY_TOPICS))
    host_lines.append("coop_sticky_probe, host call: batches of %d calls on the wall clock, at least %.1f s of timed batches per form and point, "
                      "the three forms alternating in one process, device %s" % (args.batch, args.seconds, torch.cuda.get_device_name(0)))
    ok = True
    consumers = 8
    for word in args.sizes.split(","):
        n_want = N.COOP_STICKY_ENTRIES if word == "LIMIT" else int(word)
        p = 25 if n_want % 25 == 0 else 32                               # (the limit is a power of two)
        t = n_want // p
        w, res, _, res_before = S.caught_up(t, p, consumers, 0.01, 1000 + n_want)
        n, m = int(w.n_partitions), int(w.cons_rank.max()) + 1
        owned = sharding.group_by_member_numpy(w.part_off, res_before[0], res_before[1], m)
        exp = sharding.cooperative_round_sticky_numpy(w.part_off, w.partition_id, w.lag, res[0], res[1], m, *owned, max_partitions=p)
        plain = sharding.cooperative_round_numpy(w.part_off, res[0], res[1], m, *owned)
        d_in = [torch.from_numpy(np.array(x)).to(dev) for x in
                (w.part_off, w.partition_id, w.lag, res[0], res[1], owned[0], owned[1], owned[2])]
        ptr = lambda x: x.data_ptr()
        i32 = lambda s: torch.full((s,), -7, dtype=torch.int32, device=dev)
        i64 = lambda s: torch.full((s,), -7, dtype=torch.int64, device=dev)

        def outputs():
            return [i32(n), i64(t), i64(t), i64(4), i32(n), i32(n), i64(m), i64(m), i64(m), i64(m), i64(t), i64(6), i64(m + 1), i32(n), i32(n)]

        batch_desc = N.DeviceBatch()
        batch_desc.n_topics, batch_desc.reset_mode, batch_desc.algo, batch_desc.flags = t, N.LA_RESET_LATEST, N.LA_ALGO_AUTO, 0
        batch_desc.n_partitions, batch_desc.max_partitions_per_topic = n, p
        batch_desc.d_part_off, batch_desc.d_partition_id, batch_desc.d_lag = ptr(d_in[0]), ptr(d_in[1]), ptr(d_in[2])
        batch_desc.d_out_partition, batch_desc.d_out_member_rank = ptr(d_in[3]), ptr(d_in[4])

        def fill_adjust(a, out, target):
            a.struct_size = ctypes.sizeof(N.CoopArgs)
            a.n_topics, a.n_partitions, a.n_members, a.n_owned = t, n, m, n
            a.d_part_off, a.d_out_partition, a.d_out_member_rank = ptr(d_in[0]), target, ptr(d_in[4])
            a.d_owned_member_off, a.d_owned_topic, a.d_owned_partition = ptr(d_in[5]), ptr(d_in[6]), ptr(d_in[7])
            (a.d_prev_owner, a.d_coop_member_rank, a.d_member_kept, a.d_member_fresh, a.d_member_pending, a.d_member_release,
             a.d_topic_withheld, a.d_summary) = [ptr(x) for x in out[4:12]]

        def sticky_args(out, flags):
            a = N.CoopStickyArgs()
            a.struct_size, a.flags = ctypes.sizeof(N.CoopStickyArgs), flags
            fill_adjust(a.round.adjust, out, 0)
            a.round.member_off, a.round.grouped_topic, a.round.grouped_partition = [ptr(x) for x in out[12:]]
            a.d_sticky_partition, a.d_topic_kept, a.d_topic_saved, a.d_sticky_summary = [ptr(x) for x in out[:4]]
            return a

        outs = {k: outputs() for k in ("chain", "sticky", "forced")}
        a_sticky, a_forced = sticky_args(outs["sticky"], 0), sticky_args(outs["forced"], N.LA_COOP_FORCE_TABLE)
        g = outs["chain"]
        tmp_prev = i32(n)
        first = N.CoopArgs()
        first.struct_size = ctypes.sizeof(N.CoopArgs)
        first.n_topics, first.n_partitions, first.n_members, first.n_owned = t, n, m, n
        first.d_part_off, first.d_out_partition, first.d_out_member_rank = ptr(d_in[0]), ptr(d_in[3]), ptr(d_in[4])
        first.d_owned_member_off, first.d_owned_topic, first.d_owned_partition = ptr(d_in[5]), ptr(d_in[6]), ptr(d_in[7])
        first.d_prev_owner = ptr(tmp_prev)
        second = N.StickyArgs()
        second.struct_size = ctypes.sizeof(N.StickyArgs)
        second.d_prev_owner, second.d_sticky_partition = ptr(tmp_prev), ptr(g[0])
        second.d_topic_kept, second.d_topic_saved, second.d_summary = ptr(g[1]), ptr(g[2]), ptr(g[3])
        third = N.CoopRoundArgs()
        third.struct_size = ctypes.sizeof(N.CoopRoundArgs)
        fill_adjust(third.adjust, g, ptr(g[0]))
        third.member_off, third.grouped_topic, third.grouped_partition = [ptr(x) for x in g[12:]]
        chain_launches = [0]

        def chain(count=False):
            total = 0
            for call in (lambda: lib.la_cooperative_adjust_device(h, ctypes.byref(first), sp),
                         lambda: lib.la_sticky_ties_device(h, ctypes.byref(batch_desc), ctypes.byref(second), sp),
                         lambda: lib.la_cooperative_round_device(h, ctypes.byref(third), sp)):
                rc = call()
                if rc:
                    return rc
                if count:
                    total += ctx.last_launches()
            if count:
                chain_launches[0] = total
            return 0

        forms = {"chain": chain,
                 "sticky": lambda: lib.la_cooperative_round_sticky_device(h, ctypes.byref(batch_desc), ctypes.byref(a_sticky), sp),
                 "forced": lambda: lib.la_cooperative_round_sticky_device(h, ctypes.byref(batch_desc), ctypes.byref(a_forced), sp)}
        launches = {}
        torch.cuda.synchronize()
        assert chain(True) == 0, ctx._lib.la_last_error(h)
        launches["chain"] = chain_launches[0]
        for k in ("sticky", "forced"):
            assert forms[k]() == 0, ctx._lib.la_last_error(h)
            launches[k] = ctx.last_launches()
        ctx.sync(stream)
        same = all(np.array_equal(x.cpu().numpy(), e) for k in forms for x, e in zip(outs[k], exp))
        ok = ok and same

        def batch(f):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.batch):
                f()
            e1.record()
            ctx.sync(stream)
            return float(e0.elapsed_time(e1)) * 1e3 / args.batch

        for f in forms.values():                                         # warm-up
            batch(f)
        times = {k: [] for k in forms}
        spent = {k: 0.0 for k in times}
        while min(spent.values()) < args.seconds:
            for k, f in forms.items():
                times[k].append(batch(f))
                spent[k] += times[k][-1] * args.batch * 1e-6
        med = {k: float(np.median(v)) for k, v in times.items()}
        iqr = {k: float(np.percentile(v, 75) - np.percentile(v, 25)) / med[k] for k, v in times.items()}
        say("N = n_owned = %d, T = %d, M = %d, 1 %% lagging: " % (n, t, m) + "; ".join(
            "%s %.1f us per call (min %.1f .. max %.1f, spread %.1f %%, %d batches, %d kernel launches)" % (
                k, med[k], min(times[k]), max(times[k]), 100 * iqr[k], len(times[k]), launches[k]) for k in times) +
            "; results %s" % ("agree" if same else "DIFFER"))
        say("    withheld %d of %d with sticky ties, %d without; kept %d -> %d" % (
            int(exp[11][2]), n, int(plain[7][2]), int(exp[3][0]), int(exp[3][1])))
        say("    chain / one workgroup = %.2f: the one-workgroup form is %s at %d entries (spread of the two forms %.1f %% and %.1f %%)" % (
            med["chain"] / med["sticky"], "faster" if med["sticky"] < med["chain"] else "NOT FASTER", n, 100 * iqr["chain"],
            100 * iqr["sticky"]))
        # the host calls, on the same rebalance (lags form), alternating, wall clock
        keep = [np.ascontiguousarray(x) for x in (w.part_off, w.partition_id, w.cons_off, w.cons_rank, w.lag, owned[0], owned[1], owned[2])]
        g_plain, a_host = N.AssignCoopArgs(), N.AssignStickyArgs()
        fill = lambda g: ctx._fill_assign_coop(g, keep[0], keep[1], keep[2], keep[3], m, keep[5], keep[6], keep[7], keep[4], None, None,
                                               None, 0, None, None, False, None)
        out_plain, out_host = fill(g_plain), fill(a_host.coop)
        a_host.struct_size = ctypes.sizeof(N.AssignStickyArgs)
        h_sticky, h_kept, h_saved, h_sum = np.empty(n, np.int32), np.empty(t, np.int64), np.empty(t, np.int64), np.empty(4, np.int64)
        a_host.sticky_partition, a_host.topic_kept, a_host.topic_saved = h_sticky.ctypes.data, h_kept.ctypes.data, h_saved.ctypes.data
        a_host.sticky_summary = h_sum.ctypes.data
        sticky_call = lambda: lib.la_assign_batch_cooperative_sticky(h, ctypes.byref(a_host))

        def general_batch(f):                                            # the hook is read at every call: set around the batch alone
            os.environ["LA_NO_FUSED_STICKY"] = "1"
            try:
                return f()
            finally:
                del os.environ["LA_NO_FUSED_STICKY"]

        FUSED, GENERAL, PLAIN = "fused", "LA_NO_FUSED_STICKY", "la_assign_batch_cooperative (fused)"
        hosts = {FUSED: sticky_call, GENERAL: sticky_call, PLAIN: lambda: lib.la_assign_batch_cooperative(h, ctypes.byref(g_plain))}
        host_same, hlaunches = True, {}
        for k, f in hosts.items():
            for x in (h_sticky, h_kept, h_saved, h_sum) + tuple(out_host[3:]):
                x[...] = -7
            rc = general_batch(f) if k == GENERAL else f()
            assert rc == 0, ctx._lib.la_last_error(h)
            hlaunches[k] = ctx.last_launches()
            if k != PLAIN:                                               # both forms of the sticky call: all fifteen outputs and the target
                got = (h_sticky, h_kept, h_saved, h_sum) + tuple(out_host[3:])
                host_same = host_same and all(np.array_equal(x, e) for x, e in zip(got, exp)) and np.array_equal(out_host.out_partition, res[0])
        host_same = host_same and np.array_equal(out_host.out_partition, out_plain.out_partition)
        ok = ok and host_same

        def host_batch(f):
            t0 = time.perf_counter()
            for _ in range(args.batch):
                f()
            return (time.perf_counter() - t0) * 1e6 / args.batch

        run = {k: ((lambda f=f: general_batch(lambda: host_batch(f))) if k == GENERAL else (lambda f=f: host_batch(f))) for k, f in hosts.items()}
        for r in run.values():
            r()
        htimes = {k: [] for k in hosts}
        hspent = {k: 0.0 for k in hosts}
        while min(hspent.values()) < args.seconds:
            for k, r in run.items():
                htimes[k].append(r())
                hspent[k] += htimes[k][-1] * args.batch * 1e-6
        hmed = {k: float(np.median(v)) for k, v in htimes.items()}
        hiqr = {k: float(np.percentile(v, 75) - np.percentile(v, 25)) for k, v in htimes.items()}
        margin, noise = hmed[GENERAL] - hmed[FUSED], max(hiqr[FUSED], hiqr[GENERAL])
        hsay("la_assign_batch_cooperative_sticky, host arrays, N = n_owned = %d, T = %d, M = %d, 1 %% lagging, wall clock: " % (n, t, m) +
             "; ".join("%s %.1f us per call (min %.1f .. max %.1f, interquartile %.1f us, %d batches, %d kernel launches)" % (
                 k, hmed[k], min(v), max(v), hiqr[k], len(v), hlaunches[k]) for k, v in htimes.items()) +
             "; results %s" % ("agree" if host_same else "DIFFER"))
        hsay("    LA_NO_FUSED_STICKY - fused = %.1f us against %.1f us of noise (the larger interquartile spread): the fused form is %s at "
             "%d partitions; LA_NO_FUSED_STICKY / fused = %.2f, fused / la_assign_batch_cooperative = %.2f" % (
                 margin, noise, "FASTER" if margin > noise else "NOT FASTER", n, hmed[GENERAL] / hmed[FUSED], hmed[FUSED] / hmed[PLAIN]))
    ctx.close()
    for path, text in ((args.out, lines), (args.host_out, host_lines)):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write("\n".join(text) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
