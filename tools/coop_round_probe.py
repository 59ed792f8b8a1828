#!/usr/bin/env python3
"""Time the cooperative round of a small rebalance three ways, on the same device-resident arrays:

    python tools/coop_round_probe.py [--sizes 100,1000,LIMIT --batch 100 --seconds 1.0] [--out profiles/coop_round_probe.txt]

  sequence  la_cooperative_adjust_device followed by la_group_by_member_device on its adjusted ranks: the round as it was before
            la_cooperative_round_device existed
  round     la_cooperative_round_device (within the limits of csrc/la_coop.h: one launch of one workgroup)
  forced    the same with LA_COOP_FORCE_TABLE (the general form: the sequence behind one entry point)
  host      la_cooperative_round on pageable numpy arrays (one copy each way, waited for), wall clock per call

A point is N entries over topics of 25 partitions, 8 members, every entry owned by the member a previous random assignment gave it
(n_owned = N), every output wanted.  The device forms are compared bit for bit first.  After a warm-up the forms ALTERNATE batch by
batch inside this one process until every form has at least `seconds` of timed batches; a batch is ONE pair of HIP events around
`batch` back-to-back calls, followed by a sync.  Prints median (min .. max) microseconds per call.  A record: no threshold hangs on
a time.  The last line of a point says whether the one-workgroup form is at least as fast as the sequence there -- the rule by
which the limits of la_coop.h stand.  Exit status 1 only when results differ.  Needs a GPU.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,1000,LIMIT")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from kafka_lag_based_assignor_amd import _native as N
    from kafka_lag_based_assignor_amd import sharding
    if not torch.cuda.is_available():
        sys.exit("coop_round_probe: no GPU")
    dev = torch.device("cuda", 0)
    ctx = N.Context(0)
    lib = N.load()
    stream = torch.cuda.current_stream().cuda_stream
    sp = ctypes.c_void_p(stream)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("coop_round_probe: batches of %d calls, at least %.1f s of timed batches per form and point, forms alternating, device %s; "
        "limits N %d, n_owned %d, M %d, T %d" % (args.batch, args.seconds, torch.cuda.get_device_name(0), N.COOP_SMALL_ENTRIES,
                                                  N.COOP_SMALL_OWNED, N.COOP_SMALL_MEMBERS, N.COOP_SMALL_TOPICS))
    ok = True
    m = 8
    for word in args.sizes.split(","):
        n = N.COOP_SMALL_ENTRIES if word == "LIMIT" else int(word)
        rng = np.random.default_rng(n)
        p = 25
        sizes = [p] * (n // p) + ([n % p] if n % p else [])
        t = len(sizes)
        part_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        pid = np.concatenate([rng.permutation(s) for s in sizes]).astype(np.int32)
        prev_rank = rng.integers(0, m, n).astype(np.int32)
        rank = np.where(rng.random(n) < 0.7, prev_rank, rng.integers(-1, m, n)).astype(np.int32)     # most partitions stay
        owned = sharding.group_by_member_numpy(part_off, pid, prev_rank, m)
        exp = sharding.cooperative_round_numpy(part_off, pid, rank, m, *owned)
        host_in = [part_off, pid, rank] + [np.ascontiguousarray(x) for x in owned]
        d_in = [torch.from_numpy(x).to(dev) for x in host_in]

        def outputs(make32, make64):
            return [make32(n), make32(n), make64(m), make64(m), make64(m), make64(m), make64(t), make64(6), make64(m + 1), make32(n),
                    make32(n)]

        def round_args(inp, out, flags, addr):
            r = N.CoopRoundArgs()
            r.struct_size, r.flags = ctypes.sizeof(N.CoopRoundArgs), flags
            a = r.adjust
            a.struct_size = ctypes.sizeof(N.CoopArgs)
            a.n_topics, a.n_partitions, a.n_members, a.n_owned = t, n, m, n
            a.d_part_off, a.d_out_partition, a.d_out_member_rank = addr(inp[0]), addr(inp[1]), addr(inp[2])
            a.d_owned_member_off, a.d_owned_topic, a.d_owned_partition = addr(inp[3]), addr(inp[4]), addr(inp[5])
            (a.d_prev_owner, a.d_coop_member_rank, a.d_member_kept, a.d_member_fresh, a.d_member_pending, a.d_member_release,
             a.d_topic_withheld, a.d_summary) = [addr(x) for x in out[:8]]
            r.member_off, r.grouped_topic, r.grouped_partition = [addr(x) for x in out[8:]]
            return r

        dptr = lambda x: x.data_ptr()
        outs = {k: outputs(lambda s: torch.full((s,), -7, dtype=torch.int32, device=dev),
                           lambda s: torch.full((s,), -7, dtype=torch.int64, device=dev)) for k in ("sequence", "round", "forced")}
        r_round = round_args(d_in, outs["round"], 0, dptr)
        r_forced = round_args(d_in, outs["forced"], N.LA_COOP_FORCE_TABLE, dptr)
        r_seq = round_args(d_in, outs["sequence"], 0, dptr)
        seq_adjust = r_seq.adjust
        h_out = outputs(lambda s: np.full(s, -7, np.int32), lambda s: np.full(s, -7, np.int64))
        r_host = round_args(host_in, h_out, 0, lambda x: x.ctypes.data)
        h = ctx._h
        g = outs["sequence"]

        def sequence():
            rc = lib.la_cooperative_adjust_device(h, ctypes.byref(seq_adjust), sp)
            return rc or lib.la_group_by_member_device(h, t, n, dptr(d_in[0]), dptr(d_in[1]), dptr(g[1]), m, dptr(g[8]), dptr(g[9]),
                                                       dptr(g[10]), sp)

        forms = {"sequence": sequence,
                 "round": lambda: lib.la_cooperative_round_device(h, ctypes.byref(r_round), sp),
                 "forced": lambda: lib.la_cooperative_round_device(h, ctypes.byref(r_forced), sp)}
        launches = {}
        torch.cuda.synchronize()
        for k, f in forms.items():
            assert f() == 0, ctx._lib.la_last_error(h)
            launches[k] = ctx.last_launches() + (1 if k == "sequence" else 0)      # (the group call does not report its one launch)
        ctx.sync(stream)
        assert lib.la_cooperative_round(h, ctypes.byref(r_host)) == 0, ctx._lib.la_last_error(h)
        same = all(np.array_equal(x, e) for x, e in zip(h_out, exp))
        for k in forms:
            same = same and all(np.array_equal(x.cpu().numpy(), e) for x, e in zip(outs[k], exp))
        ok = ok and same

        def batch(f):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.batch):
                f()
            e1.record()
            ctx.sync(stream)
            return float(e0.elapsed_time(e1)) * 1e3 / args.batch

        def host_batch():
            t0 = time.perf_counter()
            for _ in range(args.batch):
                lib.la_cooperative_round(h, ctypes.byref(r_host))
            return (time.perf_counter() - t0) * 1e6 / args.batch

        for f in forms.values():                                         # warm-up
            batch(f)
        host_batch()
        times = {k: [] for k in list(forms) + ["host"]}
        spent = {k: 0.0 for k in times}
        while min(spent.values()) < args.seconds:
            for k, f in forms.items():
                times[k].append(batch(f))
                spent[k] += times[k][-1] * args.batch * 1e-6
            times["host"].append(host_batch())
            spent["host"] += times["host"][-1] * args.batch * 1e-6
        med = {k: float(np.median(v)) for k, v in times.items()}
        say("N = n_owned = %d, T = %d, M = %d: " % (n, t, m) + "; ".join(
            "%s %.1f us per call (min %.1f .. max %.1f, %d batches%s)" % (
                k, med[k], min(times[k]), max(times[k]), len(times[k]),
                ", %d kernel launches" % launches[k] if k in launches else ", wall clock")
            for k in times) + "; results %s" % ("agree" if same else "DIFFER"))
        say("    one workgroup / sequence = %.2f: the one-workgroup form is %s at %d entries" % (
            med["round"] / med["sequence"], "not slower" if med["round"] <= med["sequence"] else "SLOWER", n))
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
