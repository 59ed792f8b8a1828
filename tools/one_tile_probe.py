#!/usr/bin/env python3
"""One unloaded wavefront of the tile kernel: a 2-topic batch of 256 x 32, back-to-back calls between HIP events.

    python tools/one_tile_probe.py                       # the in-tree build
    LA_LIB_PATH=other/liblagassign.so python tools/one_tile_probe.py     # another build, for a same-box A/B

Two forms: the resident single-launch kernel (wide code inline; a batch this small is widened to one 64-lane group per topic)
and the lean kernel of the bounded form (LA_FLAG_DEFER_WIDE | LA_FLAG_BOUNDS: one launch, nothing deferred).  ONE_TILE_CALLS
calls per window (default 2 000), ONE_TILE_REPS windows (default 5); prints the median, minimum and maximum microseconds per
call.  Back-to-back calls of a kernel this short are bounded below by the launch rate: read the kernel's own duration from a
`rocprofv3 --kernel-trace` of this script (ONE_TILE_CALLS=200 ONE_TILE_REPS=1)."""
import os, sys, json
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import synth

dev = torch.device("cuda", 0)
ctx = N.Context(0)
w = synth.make_uniform("custom", 11, 2, 256, 32, "zipf")
d = {k: torch.from_numpy(np.ascontiguousarray(getattr(w, k))).to(dev) for k in
     ("part_off", "partition_id", "begin", "end", "committed", "cons_off", "cons_rank")}
out_pid = torch.empty(w.n_partitions, device=dev, dtype=torch.int32)
out_rank = torch.empty(w.n_partitions, device=dev, dtype=torch.int32)
out_total = torch.empty(w.cons_rank.size, device=dev, dtype=torch.int64)
lag_max = int(np.maximum(w.end - np.where(w.committed >= 0, w.committed, 0), 0).max())


def batch(flags, bounds):
    b = N.DeviceBatch()
    b.n_topics, b.reset_mode, b.algo, b.flags = w.n_topics, N.LA_RESET_EARLIEST, N.LA_ALGO_AUTO, flags
    b.n_partitions, b.n_consumers = w.n_partitions, w.cons_rank.size
    b.max_partitions_per_topic, b.max_consumers_per_topic = w.max_partitions, w.max_consumers
    b.d_part_off, b.d_partition_id = d["part_off"].data_ptr(), d["partition_id"].data_ptr()
    b.d_begin_off, b.d_end_off, b.d_committed_off = d["begin"].data_ptr(), d["end"].data_ptr(), d["committed"].data_ptr()
    b.d_cons_off, b.d_cons_rank = d["cons_off"].data_ptr(), d["cons_rank"].data_ptr()
    b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = out_pid.data_ptr(), out_rank.data_ptr(), out_total.data_ptr()
    if bounds:
        b.flags |= N.LA_FLAG_BOUNDS
        b.max_lag_hint, b.max_partition_id_hint = lag_max, int(w.partition_id.max())
    return b


calls = int(os.environ.get("ONE_TILE_CALLS", "2000"))
reps = int(os.environ.get("ONE_TILE_REPS", "5"))
stream = torch.cuda.current_stream().cuda_stream
res = {}
for name, b in (("resident_single_launch", batch(0, False)), ("bounded_two_launch_form", batch(N.LA_FLAG_DEFER_WIDE, True))):
    for _ in range(300):
        ctx.assign_batch_device(b, stream)
    ctx.sync(stream)
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            ctx.assign_batch_device(b, stream)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1000.0 / calls)
    res[name] = {"us_per_call_median": round(float(np.median(us)), 3), "min": round(min(us), 3), "max": round(max(us), 3)}
ctx.close()
print(json.dumps(res))
