#!/usr/bin/env python3
"""Time la_member_loads_device against torch's own reductions on the same device arrays.

    python tools/loads_probe.py [--n 25600000 --k 3200000 --members 32 1000000 --launches 200 --windows 7] [--out FILE]

Per member count M: N member ranks (1 % of them -1) and K (consumer rank, total) pairs, uniformly random, in enough resident
copies that a call never finds its inputs in the 256 MiB Infinity Cache (768 MB between two touches of one copy, as bench.py's
rotation_for).  After a warm-up, `windows` timed windows per side, library and torch alternating, each ONE pair of HIP events
around `launches` back-to-back calls on the stream they run on.  The torch side is the yardstick that is not the code under
test:  torch.bincount(rank + 1, minlength=M + 1)  plus  torch.zeros(M, int64).index_add_(0, cons_rank, totals).

Prints per M the median and the spread (min .. max) of both sides in microseconds per call, the library's streaming floor
(4 N + 12 K) bytes / 8 TB/s and its fraction of it, and whether the library is not slower than torch (its median at most
torch's plus the larger of the two spreads).  Both sides' results are compared bit for bit first.  Exit status 1 when the
results differ or the library is slower.  Needs a GPU: there is nothing to fall back to.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
CACHE_PROOF_BYTES = 768 << 20
MAX_COPIES = 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=25_600_000)
    ap.add_argument("--k", type=int, default=3_200_000)
    ap.add_argument("--members", type=int, nargs="+", default=[32, 1_000_000])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from kafka_lag_based_assignor_amd import _native as N
    if not torch.cuda.is_available():
        sys.exit("loads_probe: no GPU")
    dev = torch.device("cuda", 0)
    ctx = N.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n, k = args.n, args.k
    set_bytes = 4 * n + 12 * k
    copies = int(max(1, min(MAX_COPIES, -(-CACHE_PROOF_BYTES // max(set_bytes, 1)))))
    floor_us = set_bytes / HBM_BYTES_PER_S * 1e6
    say("loads_probe: N = %d, K = %d, %d bytes per call, %d resident copies, %d launches x %d windows per side, device %s"
        % (n, k, set_bytes, copies, args.launches, args.windows, torch.cuda.get_device_name(0)))
    ok = True
    for m in args.members:
        rng = np.random.default_rng(m)
        sets = []
        for c in range(copies):
            rank = rng.integers(0, m, n, dtype=np.int32)
            rank[rng.random(n) < 0.01] = -1
            cons = rng.integers(0, m, k, dtype=np.int32)
            tot = rng.integers(-(1 << 63), (1 << 63) - 1, k, dtype=np.int64)
            sets.append(tuple(torch.from_numpy(a).to(dev) for a in (rank, cons, tot)))
        parts = torch.empty(m, dtype=torch.int64, device=dev)
        lag = torch.empty(m, dtype=torch.int64, device=dev)
        un = torch.empty(1, dtype=torch.int64, device=dev)

        def lib_call(i):
            r, c, t = sets[i % copies]
            ctx.member_loads_device(n, r.data_ptr(), k, c.data_ptr(), t.data_ptr(), m, parts.data_ptr(), lag.data_ptr(),
                                    un.data_ptr(), stream=stream)

        def torch_call(i):
            r, c, t = sets[i % copies]
            counts = torch.bincount(r + 1, minlength=m + 1)
            sums = torch.zeros(m, dtype=torch.int64, device=dev).index_add_(0, c, t)
            return counts, sums

        # same bits first
        lib_call(0)
        ctx.sync(stream)
        counts, sums = torch_call(0)
        same = bool(torch.equal(counts[1:], parts)) and bool(torch.equal(sums, lag)) and int(counts[0]) == int(un[0])
        ok = ok and same

        def window(call, i0):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.launches):
                call(i0 + i)
            e1.record()
            torch.cuda.synchronize()
            return float(e0.elapsed_time(e1)) * 1e3 / args.launches

        for call in (lib_call, torch_call):                           # warm-up: every copy, both sides
            for i in range(2 * copies):
                call(i)
        torch.cuda.synchronize()
        t_lib, t_torch = [], []
        for w in range(args.windows):
            t_lib.append(window(lib_call, w * args.launches))
            t_torch.append(window(torch_call, w * args.launches))
        ctx.sync(stream)
        lib_med, torch_med = float(np.median(t_lib)), float(np.median(t_torch))
        spread = max(max(t_lib) - min(t_lib), max(t_torch) - min(t_torch))
        not_slower = lib_med <= torch_med + spread
        ok = ok and not_slower
        say("M = %d: library %.1f us per call (min %.1f .. max %.1f), torch pair %.1f us (min %.1f .. max %.1f); results %s; "
            "streaming floor %.1f us, the library runs at %.2f of it (%.2f TB/s); library not slower than torch: %s"
            % (m, lib_med, min(t_lib), max(t_lib), torch_med, min(t_torch), max(t_torch), "equal" if same else "DIFFER",
               floor_us, floor_us / lib_med, set_bytes / lib_med * 1e6 / 1e12, "yes" if not_slower else "NO"))
        del sets
        torch.cuda.empty_cache()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
