// la_host.hip -- everything that exists to serve the host-buffer calls of include/lagassign.h: the one builder of their device
// batches (device_batch), the three chunked pipelines (run_lane, run_shard_async, run_shard_mapped), the staged small-call forms
// (assign_small_zc, assign_small), the planner, assign_host and the grouping of the results it leaves on the device.
#include "la_ctx.h"

namespace {

// Validates the offsets on the host and measures the call.
int scan_shape(la_ctx* ctx, int32_t T, const int64_t* part_off, const int64_t* cons_off, Shape* s) {
    if (part_off[0] != 0 || cons_off[0] != 0) return fail(ctx, LA_EINVAL, "part_off[0] and cons_off[0] must be 0");
    for (int32_t t = 0; t < T; ++t) {
        const int64_t p = part_off[t + 1] - part_off[t], c = cons_off[t + 1] - cons_off[t];
        if (p < 0 || c < 0) return fail(ctx, LA_EINVAL, "offsets of topic %d decrease", t);
        if (p > s->max_p) s->max_p = p;
        if (c > s->max_c) s->max_c = c;
    }
    s->n = part_off[T];
    s->k = cons_off[T];
    return LA_OK;
}

constexpr int64_t kMinChunkPartitions = 1 << 19;   // a chunk's copies must be long enough to hide a kernel
constexpr int64_t kMidChunkPartitions = 100000;    // pageable arrays: from two such chunks on, a mid-size shard runs on two lanes
constexpr int kMaxChunks = 64;

// THE device batch of a host-buffer call: every pipeline and staged form builds its batches here.  `w` says where the arrays of
// the call -- or of the shard or chunk of it that the batch covers -- lie on the device, whatever brought them there (a pipeline's
// copies, a staging buffer, the caller's own mapped memory), and the sizes and host offsets that go with them.  It fills in
// every slot whether the call uses it or not (d_end_off: the lags, for la_assign_batch_lags); the rules are applied here, once:
// `begin` only where the call reads it, the lags in the slot of the end offsets, totals only where the caller wants them.  The
// caller's hints ride along: bounds that hold for the whole call hold for every chunk and shard of it.
la_device_batch device_batch(const HostCall& c, la_device_batch w) {
    w.reset_mode = c.reset_mode == LA_RESET_LATEST ? LA_RESET_LATEST : LA_RESET_EARLIEST;
    w.algo = LA_ALGO_AUTO;
    w.max_partitions_per_topic = c.shape.max_p;
    w.max_consumers_per_topic = c.shape.max_c;
    w.flags = LA_FLAG_RAGGED;        // the offsets are on the host anyway: let the dispatcher look at the shapes
    if (c.bounded) {
        w.flags |= LA_FLAG_BOUNDS;
        w.max_lag_hint = c.max_lag;
        w.max_partition_id_hint = c.max_id;
    }
    if (!c.use_begin) w.d_begin_off = nullptr;
    w.d_lag = c.lag ? w.d_end_off : nullptr;
    if (!c.out_total) w.d_out_total_lag = nullptr;
    return w;
}

// A batch with nothing to assign is not launched; its consumers -- the nk entries from k_first on -- still report a total of 0.
int assign_or_zero(la_ctx* ctx, Lane& ln, const la_device_batch& b, size_t np, int64_t k_first, size_t nk, hipStream_t st) {
    if (np) return enqueue_batch(ctx, ln, &b, st);
    if (b.d_out_total_lag && nk) LA_HIP(ctx, hipMemsetAsync(b.d_out_total_lag + k_first, 0, nk * 8, st));
    return LA_OK;
}

struct ShardPlan {
    int32_t t0 = 0, t1 = 0;                 // the shard's topics in the caller's numbering
    int64_t P0 = 0, K0 = 0, n = 0, k = 0;   // its partitions / consumer entries: first position, count
    const int64_t *lpo = nullptr, *lco = nullptr;   // offsets rebased to the shard (host)
    std::vector<int32_t> chunk;             // chunk boundaries, shard-local topic indices
    std::vector<int64_t> none_at;           // sparse begin: first list entry of every chunk (+ the end), caller's numbering
    std::atomic<int> next{0};
};

// Buffers + offsets of one shard, on the calling thread, before its lanes start.
int prepare_shard(la_ctx* ctx, const HostCall& c, Shard& sh, ShardPlan& sp) {
    LA_HIP(ctx, hipSetDevice(sh.device));
    const int32_t Ts = sp.t1 - sp.t0;
    if (sp.P0 == 0 && sp.K0 == 0) {
        sp.lpo = c.part_off + sp.t0;
        sp.lco = c.cons_off + sp.t0;
    } else {
        sh.local_part_off.resize((size_t)Ts + 1);
        sh.local_cons_off.resize((size_t)Ts + 1);
        for (int32_t t = 0; t <= Ts; ++t) {
            sh.local_part_off[t] = c.part_off[sp.t0 + t] - sp.P0;
            sh.local_cons_off[t] = c.cons_off[sp.t0 + t] - sp.K0;
        }
        sp.lpo = sh.local_part_off.data();
        sp.lco = sh.local_cons_off.data();
    }
    const size_t nb8 = (size_t)sp.n * 8, nb4 = (size_t)sp.n * 4, kb8 = (size_t)sp.k * 8, kb4 = (size_t)sp.k * 4;
    const size_t tb = (size_t)(Ts + 1) * 8;
    int rc;
    if ((rc = reserve(ctx, sh.part_off, tb)) || (rc = reserve(ctx, sh.cons_off, tb))) return rc;
    if (c.mapped) {
        // the kernels work on the caller's arrays in place: only what is NOT the caller's lives here -- the results of a call
        // that keeps them on the device, and the dense `begin` rebuilt from a sparse list (indexed by the caller's positions,
        // begin[0] included: the tile kernels park idle lanes there)
        if (!c.out_pid && ((rc = reserve(ctx, sh.out_pid, nb4 + 16)) || (rc = reserve(ctx, sh.out_rank, nb4 + 16)))) return rc;
        if (!c.out_total && (rc = reserve(ctx, sh.out_total, kb8 + 16))) return rc;
        if (c.sparse && (rc = reserve(ctx, sh.begin, (size_t)c.shape.n * 8 + 16))) return rc;
    } else if ((rc = reserve(ctx, sh.pid, nb4 + 16)) || (rc = reserve(ctx, sh.end, nb8 + 16)) ||
               (rc = reserve(ctx, sh.committed, c.lag ? 16 : nb8 + 16)) ||
               (rc = reserve(ctx, sh.begin, c.use_begin ? nb8 + 16 : 16)) ||
               (rc = reserve(ctx, sh.cons_rank, kb4 + 16)) || (rc = reserve(ctx, sh.out_pid, nb4 + 16)) ||
               (rc = reserve(ctx, sh.out_rank, nb4 + 16)) || (rc = reserve(ctx, sh.out_total, kb8 + 16))) {
        return rc;
    }
    hipStream_t st = sh.lanes[0].stream;
    LA_HIP(ctx, hipMemcpyAsync(sh.part_off.p, sp.lpo, tb, hipMemcpyHostToDevice, st));
    LA_HIP(ctx, hipMemcpyAsync(sh.cons_off.p, sp.lco, tb, hipMemcpyHostToDevice, st));
    LA_HIP(ctx, hipEventRecord(sh.ready, st));

    // chunks: enough of them that the copies of one overlap the kernels and the opposite copies of another
    int n_chunks = 1;
    if (c.mapped) {
        n_chunks = 1;                                    // the kernels pull the shard's bytes themselves: nothing to overlap
    } else if (ctx->split_always) {
        n_chunks = Ts < 3 ? (Ts > 0 ? Ts : 1) : 3;
    } else if ((int)sh.lanes.size() > 1 || ctx->last_pipeline == 2) {
        // (pinned arrays, one enqueueing thread: finer chunks -- the call ends one chunk's kernels + result copy after
        //  the last input byte has landed)
        int64_t target = ctx->chunk_partitions > 0 ? ctx->chunk_partitions : sp.n / 16;
        if (ctx->chunk_partitions <= 0 && target < kMinChunkPartitions) target = kMinChunkPartitions;
        // three-stream form: chunks of ~1 M partitions (28 MB of input) measured best on the 25.6 M-partition batch -- 13.6 ms
        // against 18-20 ms at 512 K, 14.4 at 2 M, 14.5 with few chunks that are small at both ends (profiles/archive/r03_host_probe.txt)
        // (by bytes: 1 M partitions of the dense offsets form = 28 MB of input; the sparse-begin and the lags forms move fewer
        //  bytes per partition and take proportionally more partitions per chunk -- a chunk's copies cost ~20 us each before their
        //  first byte moves, whatever they carry)
        if (ctx->chunk_partitions <= 0 && ctx->last_pipeline == 2)
            target = ((int64_t)28 << 20) / (c.lag ? 12 : (c.use_begin && !c.sparse ? 28 : 20));
        int64_t want = (sp.n + target - 1) / target;
        // pageable arrays, a mid-size shard (one chunk by the rule above): every copy of a pageable array costs its issuing thread
        // ~25 us before the first byte moves, whatever it carries, and a chunk is ten of them -- two lanes side by side still
        // halve the bytes behind each (256 000 partitions: 386 -> 326 us), more chunks than that lose (4: 421 us, 8: 501;
        // profiles/r05_b_latency_chunks.txt).  The lanes' threads are parked in the context, so the second one costs a wake-up.
        if (ctx->chunk_partitions <= 0 && ctx->last_pipeline == 1 && want == 1 && sp.n >= 2 * kMidChunkPartitions) want = 2;
        n_chunks = (int)(want < 1 ? 1 : (want > kMaxChunks ? kMaxChunks : want));
        if (n_chunks > Ts) n_chunks = Ts > 0 ? Ts : 1;
    }
    sp.chunk.resize((size_t)n_chunks + 1);
    plan_ranges(sp.lpo, 0, Ts, n_chunks, sp.chunk.data());
    sp.next.store(0);
    if (c.sparse) {
        // the list is ascending by contract, so a chunk's entries are one slice of it.  The first chunk of the call starts at
        // entry 0 and the last ends at n_none whatever the values say: every entry is then looked at by exactly one chunk, and
        // one that is not inside its chunk's positions (an unsorted or out-of-range list) is caught by the scatter kernel.
        sp.none_at.resize((size_t)n_chunks + 1);
        const int64_t* nb = c.none_index;
        const int64_t* ne = c.none_index + c.n_none;
        for (int ci = 0; ci <= n_chunks; ++ci) {
            const int64_t pos = sp.P0 + sp.lpo[sp.chunk[(size_t)ci]];
            sp.none_at[(size_t)ci] = std::lower_bound(nb, ne, pos) - nb;
        }
        if (sp.P0 == 0) sp.none_at[0] = 0;
        if (sp.P0 + sp.n == c.shape.n) sp.none_at[(size_t)n_chunks] = c.n_none;
        const size_t m = (size_t)(sp.none_at[(size_t)n_chunks] - sp.none_at[0]);
        if ((rc = reserve(ctx, sh.none_idx, m * 8 + 16)) || (rc = reserve(ctx, sh.none_val, m * 8 + 16))) return rc;
    }
    return LA_OK;
}

// Chunk ci of a shard: its topics [a, z) in the shard's numbering, its partitions [p0, p1) and consumer entries [k0, k1) in the
// shard's buffers, where they start in the caller's arrays (gp, gk), and how many there are (np, nk).
struct Chunk {
    int32_t a, z;
    int64_t p0, p1, k0, k1, gp, gk;
    size_t np, nk;
};

Chunk chunk_of(const ShardPlan& sp, int ci) {
    Chunk ck{};
    ck.a = sp.chunk[(size_t)ci]; ck.z = sp.chunk[(size_t)ci + 1];
    ck.p0 = sp.lpo[ck.a]; ck.p1 = sp.lpo[ck.z]; ck.k0 = sp.lco[ck.a]; ck.k1 = sp.lco[ck.z];
    ck.gp = sp.P0 + ck.p0; ck.gk = sp.K0 + ck.k0;              // the chunk in the caller's arrays
    ck.np = (size_t)(ck.p1 - ck.p0); ck.nk = (size_t)(ck.k1 - ck.k0);
    return ck;
}

// Sparse begin offsets of chunk ci: `copy` (non-null) uploads the chunk's slice of the (position, begin) list, `kern`
// (non-null) zeroes the chunk's part of the dense array and scatters the slice into it.  One stream may play both roles.
int sparse_begin_chunk(la_ctx* ctx, const HostCall& c, Shard& sh, const ShardPlan& sp, int ci, const Chunk& ck, Lane& ln,
                       hipStream_t copy, hipStream_t kern) {
    const int64_t j0 = sp.none_at[(size_t)ci], j1 = sp.none_at[(size_t)ci + 1], at = j0 - sp.none_at[0], p0 = ck.p0, p1 = ck.p1;
    const size_t m = (size_t)(j1 - j0);
    int64_t* d_idx = (int64_t*)sh.none_idx.p + at;
    int64_t* d_val = (int64_t*)sh.none_val.p + at;
    if (copy && m) {
        LA_HIP(ctx, hipMemcpyAsync(d_idx, c.none_index + j0, m * 8, hipMemcpyHostToDevice, copy));
        LA_HIP(ctx, hipMemcpyAsync(d_val, c.none_begin + j0, m * 8, hipMemcpyHostToDevice, copy));
    }
    if (kern) {
        if (p1 > p0) LA_HIP(ctx, hipMemsetAsync((int64_t*)sh.begin.p + p0, 0, (size_t)(p1 - p0) * 8, kern));
        LA_HIP(ctx, la::sparse_begin_launch((int64_t)m, d_idx, d_val, sp.P0, sp.P0 + p0, sp.P0 + p1, (int64_t*)sh.begin.p,
                                            ln.d_status, kern));
    }
    return LA_OK;
}

// H2D of a chunk's per-partition slices (a sparse begin list and the consumer ranks travel their pipeline's own way).
int chunk_copy_in(la_ctx* ctx, const HostCall& c, Shard& sh, const Chunk& ck, hipStream_t st) {
    if (!ck.np) return LA_OK;
    const int64_t p0 = ck.p0, gp = ck.gp;
    const size_t np = ck.np;
    LA_HIP(ctx, hipMemcpyAsync((int32_t*)sh.pid.p + p0, c.pid + gp, np * 4, hipMemcpyHostToDevice, st));
    if (c.lag) {
        LA_HIP(ctx, hipMemcpyAsync((int64_t*)sh.end.p + p0, c.lag + gp, np * 8, hipMemcpyHostToDevice, st));
    } else {
        LA_HIP(ctx, hipMemcpyAsync((int64_t*)sh.end.p + p0, c.end + gp, np * 8, hipMemcpyHostToDevice, st));
        LA_HIP(ctx, hipMemcpyAsync((int64_t*)sh.committed.p + p0, c.committed + gp, np * 8, hipMemcpyHostToDevice, st));
        if (c.use_begin && !c.sparse)
            LA_HIP(ctx, hipMemcpyAsync((int64_t*)sh.begin.p + p0, c.begin + gp, np * 8, hipMemcpyHostToDevice, st));
    }
    return LA_OK;
}

// D2H of a chunk's results, as far as the caller wants them.
int chunk_copy_out(la_ctx* ctx, const HostCall& c, Shard& sh, const Chunk& ck, hipStream_t st) {
    const int64_t p0 = ck.p0, k0 = ck.k0, gp = ck.gp, gk = ck.gk;
    const size_t np = ck.np, nk = ck.nk;
    if (np && c.out_pid) {
        LA_HIP(ctx, hipMemcpyAsync(c.out_pid + gp, (const int32_t*)sh.out_pid.p + p0, np * 4, hipMemcpyDeviceToHost, st));
        LA_HIP(ctx, hipMemcpyAsync(c.out_rank + gp, (const int32_t*)sh.out_rank.p + p0, np * 4, hipMemcpyDeviceToHost, st));
    }
    if (c.out_total && nk)
        LA_HIP(ctx, hipMemcpyAsync(c.out_total + gk, (const int64_t*)sh.out_total.p + k0, nk * 8, hipMemcpyDeviceToHost, st));
    return LA_OK;
}

// What chunk ci of a shard does on the device between the copies of its per-partition slices in and of its results out, on
// lane ln: the sparse-begin scatter, the check of its consumers, and its batch -- all on stream `kern`.  `copy` is the stream
// that brings the chunk's own sparse list and consumer ranks up first, or null where the pipeline has already sent the shard's.
// The chunk is a topic sub-range of the shard's batch: same arrays, offsets advanced to its first topic.
// n_partitions / n_consumers stay the shard's totals -- they bound the kernels' clamped loads, which may
// touch (and ignore) elements of neighbouring chunks.
int chunk_device_work(la_ctx* ctx, const HostCall& c, Shard& sh, const ShardPlan& sp, int ci, const Chunk& ck, Lane& ln,
                      hipStream_t copy, hipStream_t kern) {
    // (list entries where there are no partitions: the kernel reports them)
    if (c.sparse && (ck.np || sp.none_at[(size_t)ci + 1] > sp.none_at[(size_t)ci]))
        if (int rc = sparse_begin_chunk(ctx, c, sh, sp, ci, ck, ln, copy, kern)) return rc;
    if (ck.nk) {
        if (copy)
            LA_HIP(ctx, hipMemcpyAsync((int32_t*)sh.cons_rank.p + ck.k0, c.cons_rank + ck.gk, ck.nk * 4, hipMemcpyHostToDevice, copy));
        // the ascending-rank contract of cons_rank is checked on the device (one pass over K entries there
        // instead of ~1 ns per entry of host time), reported by sync_status as LA_EINVAL
        LA_HIP(ctx, la::check_consumers_launch(ck.z - ck.a, (const int64_t*)sh.cons_off.p + ck.a,
                                               (const int32_t*)sh.cons_rank.p, ln.d_status, kern));
    }
    la_device_batch w{};
    w.n_topics = ck.z - ck.a; w.n_partitions = sp.n; w.n_consumers = sp.k;
    w.d_part_off = (const int64_t*)sh.part_off.p + ck.a;
    w.d_cons_off = (const int64_t*)sh.cons_off.p + ck.a;
    w.d_partition_id = (const int32_t*)sh.pid.p;
    w.d_begin_off = (const int64_t*)sh.begin.p;
    w.d_end_off = (const int64_t*)sh.end.p;
    w.d_committed_off = (const int64_t*)sh.committed.p;
    w.d_cons_rank = (const int32_t*)sh.cons_rank.p;
    w.d_out_partition = (int32_t*)sh.out_pid.p; w.d_out_member_rank = (int32_t*)sh.out_rank.p;
    w.d_out_total_lag = (int64_t*)sh.out_total.p;
    w.h_part_off = sp.lpo + ck.a; w.h_cons_off = sp.lco + ck.a;
    return assign_or_zero(ctx, ln, device_batch(c, w), ck.np, ck.k0, ck.nk, kern);
}

// One lane of one shard: takes the shard's chunks in order until none is left.  Per chunk: H2D of its slices,
// the kernels over its topics, D2H of its results -- all on the lane's stream; the lanes of a shard overlap
// each other (the copies of a pageable buffer block their host thread, which is why lanes are threads).
int run_lane(la_ctx* ctx, const HostCall& c, Shard& sh, ShardPlan& sp, int lane_idx, std::atomic<bool>& stop) {
    LA_HIP(ctx, hipSetDevice(sh.device));
    Lane& ln = sh.lanes[(size_t)lane_idx];
    hipStream_t st = ln.stream;
    if (lane_idx > 0) LA_HIP(ctx, hipStreamWaitEvent(st, sh.ready, 0));
    const int n_chunks = (int)sp.chunk.size() - 1;
    int rc = LA_OK;
    while (!stop.load(std::memory_order_relaxed)) {
        const int ci = sp.next.fetch_add(1);
        if (ci >= n_chunks) break;
        const Chunk ck = chunk_of(sp, ci);
        if ((rc = chunk_copy_in(ctx, c, sh, ck, st)) || (rc = chunk_device_work(ctx, c, sh, sp, ci, ck, ln, st, st)) ||
            (rc = chunk_copy_out(ctx, c, sh, ck, st)))
            break;
    }
    const int rs = sync_status(ctx, ln, st);     // also when stopping early: nothing of this lane stays in flight
    return rc ? rc : rs;
}

// true when [p, p + bytes) is pinned host memory the runtime knows (la_host_alloc, hipHostMalloc, hipHostRegister): copies
// to and from it are plain DMA and hipMemcpyAsync returns at once.  NULL / zero bytes count as pinned.
bool is_pinned(const void* p, size_t bytes) {
    if (!p || bytes == 0) return true;
    // first AND last byte: a buffer registered only in part (hipHostRegister of a sub-range), or one that runs past its
    // allocation into another, must not take the thread-less pipeline, which assumes plain DMA over the whole range
    hipPointerAttribute_t at{}, az{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess ||
        hipPointerGetAttributes(&az, (const char*)p + (bytes - 1)) != hipSuccess) {
        (void)hipGetLastError();                          // an ordinary malloc'ed pointer: not an error of ours
        return false;
    }
    if (at.type != hipMemoryTypeHost || az.type != hipMemoryTypeHost) return false;
    // the same registration: where the runtime reports the host / device views, they advance together from first to last byte
    const ptrdiff_t span = (ptrdiff_t)(bytes - 1);
    if (at.hostPointer && az.hostPointer && (const char*)az.hostPointer - (const char*)at.hostPointer != span) return false;
    if ((at.devicePointer == nullptr) != (az.devicePointer == nullptr)) return false;
    if (at.devicePointer && (const char*)az.devicePointer - (const char*)at.devicePointer != span) return false;
    return true;
}

// One shard of a call whose arrays are all pinned: no worker threads.  The calling thread enqueues, per chunk,
//   copy_in[]: H2D of the chunk's slices, chunks alternating over two streams -> event "in"
//   lane 0   : wait "in"; check_consumers; the kernels over its topics     -> event "out"
//   copy_out : wait "out"; D2H of the chunk's results straight into the caller's arrays
// so the link carries input bytes back to back from the first chunk to the last (the H2D leg IS the floor of the call:
// 717 MB at the 57 GB/s this link sustains = 12.5 ms for the 25.6 M-partition batch, profiles/archive/r03_pcie_probe.txt) while
// kernels and result copies of earlier chunks run beside it.  Returns after enqueueing; finish_shard_async waits.
int run_shard_async(la_ctx* ctx, const HostCall& c, Shard& sh, ShardPlan& sp) {
    LA_HIP(ctx, hipSetDevice(sh.device));
    for (hipStream_t& st : sh.copy_in)
        if (!st) LA_HIP(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (!sh.copy_out) LA_HIP(ctx, hipStreamCreateWithFlags(&sh.copy_out, hipStreamNonBlocking));
    const int n_chunks = (int)sp.chunk.size() - 1;
    while ((int)sh.chunk_ev.size() < 2 * n_chunks + 1) {
        hipEvent_t e = nullptr;
        LA_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        sh.chunk_ev.push_back(e);
    }
    Lane& ln = sh.lanes[0];
    hipStream_t sk = ln.stream, so = sh.copy_out;
    // the consumer ranks of the whole shard go up once (4 B per entry: too small to be worth a copy per chunk)
    // ... and so does the shard's slice of a sparse begin list (16 B per listed partition: one copy pair, not one per chunk --
    // every copy costs ~20 us of engine latency before its first byte moves)
    const size_t m_all = c.sparse ? (size_t)(sp.none_at[(size_t)n_chunks] - sp.none_at[0]) : 0;
    if (sp.k || m_all) {
        if (sp.k)
            LA_HIP(ctx, hipMemcpyAsync(sh.cons_rank.p, c.cons_rank + sp.K0, (size_t)sp.k * 4, hipMemcpyHostToDevice, sh.copy_in[1]));
        if (m_all) {
            LA_HIP(ctx, hipMemcpyAsync(sh.none_idx.p, c.none_index + sp.none_at[0], m_all * 8, hipMemcpyHostToDevice, sh.copy_in[1]));
            LA_HIP(ctx, hipMemcpyAsync(sh.none_val.p, c.none_begin + sp.none_at[0], m_all * 8, hipMemcpyHostToDevice, sh.copy_in[1]));
        }
        LA_HIP(ctx, hipEventRecord(sh.chunk_ev[(size_t)(2 * n_chunks)], sh.copy_in[1]));
        LA_HIP(ctx, hipStreamWaitEvent(sk, sh.chunk_ev[(size_t)(2 * n_chunks)], 0));
    }
    for (int ci = 0; ci < n_chunks; ++ci) {
        const Chunk ck = chunk_of(sp, ci);
        hipEvent_t ev_in = sh.chunk_ev[(size_t)(2 * ci)], ev_out = sh.chunk_ev[(size_t)(2 * ci + 1)];
        hipStream_t si = sh.copy_in[ci % Shard::kCopyIn];
        if (ck.np) {
            if (int rc = chunk_copy_in(ctx, c, sh, ck, si)) return rc;
            LA_HIP(ctx, hipEventRecord(ev_in, si));
            LA_HIP(ctx, hipStreamWaitEvent(sk, ev_in, 0));
        }
        if (int rc = chunk_device_work(ctx, c, sh, sp, ci, ck, ln, nullptr, sk)) return rc;
        LA_HIP(ctx, hipEventRecord(ev_out, sk));
        const bool any_out = (ck.np && c.out_pid) || (c.out_total && ck.nk);
        if (any_out) LA_HIP(ctx, hipStreamWaitEvent(so, ev_out, 0));
        if (int rc = chunk_copy_out(ctx, c, sh, ck, so)) return rc;
    }
    return LA_OK;
}

// ---- pinned AND mapped caller arrays: no copies at all ------------------------------------------------------------------
// la_host_alloc memory (hipHostMalloc: portable, mapped) has a device address.  The tile kernels issue all the loads of a tile
// back to back and touch every input byte exactly once, so letting THEM pull the batch across PCIe needs no staging, no
// chunks and no copy engine: measured on the 25.6 M-partition target, 10.1 ms per call against 13.6 ms for the three-stream
// copy pipeline (tools/mapped_probe.py: 52-55 GB/s of kernel loads over the link, whose one-copy floor is 57 GB/s) -- and
// `begin` crosses the link only where a partition has no committed offset, because that is all the kernels read of it.
// Results are written straight into the caller's arrays.  Every shard works on the SAME arrays (positions are the caller's:
// part_off stays absolute), on its own range of topics.
template <typename T>
T* mapped_ptr(T* host) {
    if (!host) return nullptr;
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, (void*)host, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return (T*)d;
}

// first AND last byte: an array registered only in part (hipHostRegister of a sub-range), or one that runs past
// its registration, must not be handed to kernels that read and write it in place -- its device view has to exist at both
// ends and advance with the host view in between; anything else takes a copying pipeline.  NULL / zero bytes count as mapped.
bool is_mapped(const void* p, size_t bytes) {
    if (p == nullptr || bytes == 0) return true;
    const char* d0 = mapped_ptr((const char*)p);
    const char* d1 = mapped_ptr((const char*)p + (bytes - 1));
    return d0 != nullptr && d1 != nullptr && (size_t)(d1 - d0) == bytes - 1;
}

// ok(pointer, bytes) over the arrays of a (normalised) call: all of them, or with `copied_only` those a copying pipeline moves
// between the caller and the device -- not the offsets, which go up from the shard plan's own copy, and not a `begin` the call
// never reads.  (A sparse call has no dense `begin` and every other call no list: assign_host has nulled them.)
bool call_arrays_all(const HostCall& c, bool copied_only, bool (*ok)(const void*, size_t)) {
    const size_t n = (size_t)c.shape.n, k = (size_t)c.shape.k, tb = ((size_t)c.T + 1) * 8, m = (size_t)c.n_none * 8;
    const struct { const void* p; size_t bytes; bool copied; } arrays[] = {
        {c.part_off, tb, false}, {c.cons_off, tb, false}, {c.pid, n * 4, true}, {c.end, n * 8, true}, {c.committed, n * 8, true},
        {c.lag, n * 8, true}, {c.begin, n * 8, c.use_begin}, {c.none_index, m, true}, {c.none_begin, m, true},
        {c.cons_rank, k * 4, true}, {c.out_pid, n * 4, true}, {c.out_rank, n * 4, true}, {c.out_total, k * 8, true}};
    for (const auto& x : arrays)
        if ((x.copied || !copied_only) && !ok(x.p, x.bytes)) return false;
    return true;
}

// every array that is copied is pinned: the call can take the thread-less three-stream pipeline
bool call_is_pinned(const HostCall& c) { return call_arrays_all(c, true, is_pinned); }
// every array is mapped, copied or not: the kernels would address all of them
bool call_is_mapped(const HostCall& c) { return call_arrays_all(c, false, is_mapped); }

int run_shard_mapped(la_ctx* ctx, const HostCall& c, Shard& sh, ShardPlan& sp) {
    LA_HIP(ctx, hipSetDevice(sh.device));
    Lane& ln = sh.lanes[0];
    hipStream_t st = ln.stream;
    la_device_batch w{};
    w.n_topics = sp.t1 - sp.t0;
    w.n_partitions = c.shape.n;                                                  // (positions are the caller's: the bound is too)
    w.n_consumers = c.shape.k;
    w.d_part_off = mapped_ptr(c.part_off) + sp.t0;
    w.d_cons_off = mapped_ptr(c.cons_off) + sp.t0;
    w.d_cons_rank = mapped_ptr(c.cons_rank);
    if (sp.k)
        LA_HIP(ctx, la::check_consumers_launch(w.n_topics, w.d_cons_off, w.d_cons_rank, ln.d_status, st));
    w.d_begin_off = mapped_ptr(c.begin);
    if (c.sparse) {
        int64_t* db = (int64_t*)sh.begin.p;
        const int64_t j0 = sp.none_at.front(), j1 = sp.none_at.back();
        LA_HIP(ctx, hipMemsetAsync(db, 0, 8, st));                               // begin[0]: where idle lanes park
        if (sp.n) LA_HIP(ctx, hipMemsetAsync(db + sp.P0, 0, (size_t)sp.n * 8, st));
        LA_HIP(ctx, la::sparse_begin_launch(j1 - j0, mapped_ptr(c.none_index) + j0, mapped_ptr(c.none_begin) + j0, 0, sp.P0,
                                            sp.P0 + sp.n, db, ln.d_status, st));
        w.d_begin_off = db;
    }
    w.d_partition_id = mapped_ptr(c.pid);
    w.d_end_off = mapped_ptr(c.lag ? c.lag : c.end);
    w.d_committed_off = mapped_ptr(c.committed);
    // results the caller asked for land in its arrays; those it leaves on the device go to the shard's own buffers, addressed
    // by the caller's positions (only positions of this shard's topics are ever stored)
    // (the shard's own buffers hold positions [P0, P0 + n) only; their "position 0" is an address computed in integers, never
    //  dereferenced below P0)
    auto rebased = [&](void* base) { return (int32_t*)((uintptr_t)base - (uintptr_t)sp.P0 * sizeof(int32_t)); };
    w.d_out_partition = c.out_pid ? mapped_ptr(c.out_pid) : rebased(sh.out_pid.p);
    w.d_out_member_rank = c.out_pid ? mapped_ptr(c.out_rank) : rebased(sh.out_rank.p);
    w.d_out_total_lag = mapped_ptr(c.out_total);
    w.h_part_off = c.part_off + sp.t0; w.h_cons_off = c.cons_off + sp.t0;
    return assign_or_zero(ctx, ln, device_batch(c, w), (size_t)sp.n, sp.K0, (size_t)sp.k, st);
}

// Waits for everything run_shard_async enqueued on this shard (also after an error elsewhere: nothing stays in flight).
int finish_shard_async(la_ctx* ctx, Shard& sh) {
    LA_HIP(ctx, hipSetDevice(sh.device));
    const int rs = sync_status(ctx, sh.lanes[0], sh.lanes[0].stream);
    hipError_t e1 = hipSuccess;
    for (hipStream_t st : sh.copy_in)
        if (st) { const hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess) e1 = e; }
    hipError_t e2 = sh.copy_out ? hipStreamSynchronize(sh.copy_out) : hipSuccess;
    if (rs) return rs;
    if (e1 != hipSuccess || e2 != hipSuccess)
        return fail(ctx, LA_EHIP, "copy stream: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    return LA_OK;
}

// ---- small batches: one H2D, the kernels, one D2H ----------------------------------------------------------------
// A real group leader's rebalance is ONE call over a few dozen topics.  The chunked pipeline above is built for bandwidth;
// at this size the call is API latency: 7 H2D copies of caller arrays, 3 D2H copies, the status word, ~8 us each -- 105 us
// for a three-partition batch.  Here the inputs are packed into one pinned staging buffer (a memcpy of kilobytes), go up
// in ONE copy together with a zeroed status word, and status + results come back in ONE copy.
constexpr size_t kSmallBytes = 12u << 20;                   // (~340 000 partitions)
constexpr size_t kGroupStageBytes = 2u << 20;               // la_group_last_by_member: CSRs up to this size cross in one copy
constexpr size_t kMappedSmallBytes = 1280u << 10;          // mapped caller arrays: layouts beyond this are read in place instead
constexpr size_t kMappedSmallGroupedBytes = 3u << 20;      // ... and beyond this when the call wants every member's list too
constexpr size_t kPinnedSmallBytes = 2u << 20;             // pinned, not mapped: beyond this the three-stream pipeline
constexpr size_t kSmallHostCheck = 16384;      // consumer entries up to which the small path validates the ranks on the host

// One output of a staged call: where the caller wants it (null: it does not), and where it lies in the staging layout.
struct StagedOut { void* to; size_t off, bytes; };
// In the order of the layout.  The member lists are those of a grouped call, or of the ADJUSTED assignment of a cooperative one,
// whose eight outputs follow them, then the four of the sticky order (la_assign_batch_cooperative_sticky: carved for such a call
// only); the ungrouped results come last, so that a download can stop short of them.
enum { kOutTotals, kOutMemberOff, kOutListTopic, kOutListPartition, kOutKept, kOutFresh, kOutPending, kOutRelease, kOutWithheld,
       kOutSummary, kOutPrevOwner, kOutCoopRank, kOutSticky, kOutTopicKept, kOutTopicSaved, kOutStickySummary, kOutPid, kOutRank,
       kStagedOuts };

struct SmallLayout {
    size_t po, co, pid, end, com, beg, cr, status, total;
    // la_assign_batch_cooperative, fused form (carved for such a call only: every other call's layout is what it was): the owned
    // arrays on the upload side of the status word
    size_t oo, otp, opp;
    StagedOut out[kStagedOuts];                               // the download side of the status word
    // output `slot` in the copy of the layout at `base`: at() wherever it lies, want() only where the caller wants it
    template <typename T> T* at(const char* base, int slot) const { return (T*)(base + out[slot].off); }
    template <typename T> T* want(const char* base, int slot) const { return out[slot].to ? at<T>(base, slot) : nullptr; }
};

SmallLayout small_layout(const HostCall& c) {
    const size_t T = (size_t)c.T, n = (size_t)c.shape.n, k = (size_t)c.shape.k;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 16 + 255) & ~(size_t)255; return o; };
    SmallLayout L{};
    // (`room`: the slot holds its bytes even where the caller does not want them -- the kernels write there all the same)
    auto out = [&](int slot, void* to, size_t bytes, bool room = false) { L.out[slot] = {to, carve(to || room ? bytes : 0), bytes}; };
    L.po = carve((T + 1) * 8);
    L.co = carve((T + 1) * 8);
    L.pid = carve(n * 4);
    L.end = carve(n * 8);                                     // the lags, for la_assign_batch_lags
    L.com = carve(c.lag ? 0 : n * 8);
    L.beg = carve(c.use_begin ? n * 8 : 0);
    L.cr = carve(k * 4);
    const la::CoopRoundCall* q = c.coop;
    if (q) {
        const size_t no = (size_t)q->c.n_owned;
        L.oo = carve(no ? ((size_t)q->c.n_members + 1) * 8 : 0);
        L.otp = carve(no * 4);
        L.opp = carve(no * 4);
    }
    L.status = carve(256);                                    // last word of the upload, first of the download
    out(kOutTotals, c.out_total, k * 8, true);
    const bool grouped = c.g_members >= 0;                    // la_assign_batch_grouped: the CSR rides in the same download
    if (q) {                                                  // the lists of the ADJUSTED assignment take the CSR's place
        const size_t M = (size_t)q->c.n_members;
        out(kOutMemberOff, q->member_off, (M + 1) * 8, true);
        out(kOutListTopic, q->grouped_topic, n * 4);
        out(kOutListPartition, q->grouped_partition, n * 4, true);
        out(kOutKept, q->c.member_kept, M * 8);
        out(kOutFresh, q->c.member_fresh, M * 8);
        out(kOutPending, q->c.member_pending, M * 8);
        out(kOutRelease, q->c.member_release, M * 8);
        out(kOutWithheld, q->c.topic_withheld, T * 8);
        out(kOutSummary, q->c.summary, 6 * 8);
        out(kOutPrevOwner, q->c.prev_owner, n * 4);
        out(kOutCoopRank, q->c.coop_rank, n * 4);
        if (const StickyOuts* s = c.sticky) {                 // (no slot at all for any other call: its layout is what it was)
            out(kOutSticky, s->sticky_partition, n * 4, true);
            out(kOutTopicKept, s->topic_kept, T * 8);
            out(kOutTopicSaved, s->topic_saved, T * 8);
            out(kOutStickySummary, s->sticky_summary, 4 * 8);
        }
    } else {
        // (a call whose lists take their own round trip keeps g_off and its kin but has g_members < 0: not wanted HERE)
        out(kOutMemberOff, grouped ? c.g_off : nullptr, ((size_t)c.g_members + 1) * 8);
        out(kOutListTopic, grouped ? c.g_topic : nullptr, n * 4);
        out(kOutListPartition, grouped ? c.g_part : nullptr, n * 4);
    }
    out(kOutPid, c.out_pid, n * 4, true);
    out(kOutRank, c.out_rank, n * 4, true);
    L.total = off;
    return L;
}

// ---- the smallest calls: zero copies ----------------------------------------------------------------------------------
// For a rebalance of a few dozen topics even the two DMA submissions of assign_small are most of the call (~8 us each of ~35).
// Here the staging buffer is coherent host memory mapped into the device: the kernels READ the inputs in place over PCIe (all
// loads of a tile go out back to back: a couple of ~1.5 us round trips), write what the caller wants back -- totals, results
// or every member's list -- straight into it, and the call's last launch stores `done | status` where this thread is spinning.
// The ungrouped result of a grouped call never leaves the device.  No hipMemcpy, no stream synchronize.
// Up to which staging layout: rounds 3-4 stopped at 128 KB, where the form's three dependent launches + PCIe reads at kernel
// rate lost to one DMA copy each way.  With the call's end (and the small lists) fused into the tile kernel (round 5) it wins
// at every size measured up to where packing the inputs loses to the lanes' overlapped copies
// (profiles/r05_n_latency_probe.txt, r05_o_, r05_q_: 5 000 partitions 49 -> 35 us, 10 000: 56 -> 38, 30 000: 84 -> 65, 100 000:
// 242 (lanes) -> 160; 256 000: 335 (lanes) vs 402 packed by one thread, 267-310 with the parked threads' help (copy_pieces);
// 512 000: 546 vs 552) -- so every staged call is zero-copy now, and the one-copy form
// (assign_small) is what LA_ZERO_COPY_BYTES=<smaller> still selects (A/B, tests).
constexpr size_t kZeroCopyBytes = 12u << 20;

// The staged forms pack the caller's arrays into one buffer and unpack the results: plain memcpy.  From a few megabytes on that
// is most of the call on ONE thread (~35 GB/s: 100 us for the inputs of 100 000 partitions), so the pieces are handed out to
// the context's parked threads as well -- the calling thread starts on the first piece at once and simply does all of them
// when nobody else turns up in time (a parked thread needs 30-50 us to be back).  Measured, serial / with help
// (profiles/r05_q_latency_probe.txt): 100 000 partitions 161 / 139-166 us, 256 000: 402 / 267-310 us (lanes: 335).
struct CopyPiece { void* dst; const void* src; size_t bytes; };
constexpr size_t kParallelCopyBytes = 3u << 20, kCopyPieceBytes = 256u << 10;

void copy_pieces(la_ctx* ctx, const CopyPiece* cp, int n) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += cp[i].bytes;
    if (total < kParallelCopyBytes) {
        for (int i = 0; i < n; ++i)
            if (cp[i].bytes) memcpy(cp[i].dst, cp[i].src, cp[i].bytes);
        return;
    }
    std::vector<CopyPiece> pieces;
    pieces.reserve(total / kCopyPieceBytes + (size_t)n);
    for (int i = 0; i < n; ++i)
        for (size_t o = 0; o < cp[i].bytes; o += kCopyPieceBytes)
            pieces.push_back({(char*)cp[i].dst + o, (const char*)cp[i].src + o,
                              cp[i].bytes - o < kCopyPieceBytes ? cp[i].bytes - o : kCopyPieceBytes});
    std::atomic<size_t> next{0};
    ctx->pool.run(total >= (4u << 20) ? 4 : 3, [&](int) {
        for (;;) {
            const size_t i = next.fetch_add(1, std::memory_order_relaxed);
            if (i >= pieces.size()) break;
            memcpy(pieces[i].dst, pieces[i].src, pieces[i].bytes);
        }
    });
}

// The inputs of a small call, packed into its staging buffer (and validated where that is cheaper here than on the device).
int small_fill_inputs(la_ctx* ctx, const HostCall& c, const SmallLayout& L, char* h) {
    const size_t T = (size_t)c.T, n = (size_t)c.shape.n, k = (size_t)c.shape.k;
    memcpy(h + L.po, c.part_off, (T + 1) * 8);
    memcpy(h + L.co, c.cons_off, (T + 1) * 8);
    if (n) {
        const CopyPiece in[4] = {{h + L.pid, c.pid, n * 4},
                                 {h + L.end, c.lag ? c.lag : c.end, n * 8},
                                 {h + L.com, c.committed, c.lag ? 0 : n * 8},
                                 {h + L.beg, c.begin, (c.use_begin && !c.sparse) ? n * 8 : 0}};
        copy_pieces(ctx, in, 4);
        if (c.sparse) {
            // a small call rebuilds the dense array right here in the staging buffer: unlisted partitions have begin 0
            int64_t* hb = (int64_t*)(h + L.beg);
            memset(hb, 0, n * 8);
            int64_t prev = -1;
            for (int64_t j = 0; j < c.n_none; ++j) {
                const int64_t g = c.none_index[j];
                if (g <= prev || g >= (int64_t)n)
                    return fail(ctx, LA_EINVAL, "none_index must hold ascending positions inside the batch");
                hb[g] = c.none_begin[j];
                prev = g;
            }
        }
    }
    if (k) memcpy(h + L.cr, c.cons_rank, k * 4);
    if (c.coop && c.coop->c.n_owned > 0) {
        const la::CoopCall& q = c.coop->c;
        memcpy(h + L.oo, q.owned_off, ((size_t)q.n_members + 1) * 8);
        memcpy(h + L.otp, q.owned_topic, (size_t)q.n_owned * 4);
        memcpy(h + L.opp, q.owned_partition, (size_t)q.n_owned * 4);
    }
    if (k && k <= kSmallHostCheck) {
        // a topic's member ranks must be strictly ascending (the kernels compare ranks, never strings).  A few thousand
        // entries are checked here in less time than the ~5 us a dependent launch of the check kernel puts in front of
        // the assignment kernels -- and a real rebalance is this size.
        for (size_t t = 0; t < T; ++t)
            for (int64_t j = c.cons_off[t] + 1; j < c.cons_off[t + 1]; ++j)
                if (c.cons_rank[j - 1] >= c.cons_rank[j])
                    return fail(ctx, LA_EINVAL, "a topic's cons_rank segment is not strictly ascending");
    }
    return LA_OK;
}

// The device batch of a staged call: inputs (and totals) at in_base, results at out_base, both laid out by L.
la_device_batch small_batch(const HostCall& c, const SmallLayout& L, char* in_base, char* out_base) {
    la_device_batch w{};
    w.n_topics = c.T; w.n_partitions = c.shape.n; w.n_consumers = c.shape.k;
    w.d_part_off = (const int64_t*)(in_base + L.po);
    w.d_cons_off = (const int64_t*)(in_base + L.co);
    w.d_partition_id = (const int32_t*)(in_base + L.pid);
    w.d_begin_off = (const int64_t*)(in_base + L.beg);
    w.d_end_off = (const int64_t*)(in_base + L.end);
    w.d_committed_off = (const int64_t*)(in_base + L.com);
    w.d_cons_rank = (const int32_t*)(in_base + L.cr);
    w.d_out_partition = L.at<int32_t>(out_base, kOutPid); w.d_out_member_rank = L.at<int32_t>(out_base, kOutRank);
    w.d_out_total_lag = L.at<int64_t>(in_base, kOutTotals);
    w.h_part_off = c.part_off; w.h_cons_off = c.cons_off;
    return device_batch(c, w);
}

// The end both staged forms share, only ever after a status of zero.  Every output the caller wants, from the host side `h` of
// the staging buffer into its arrays (`pieces`: through copy_pieces; `n_slots`: kOutPid where the ungrouped results do not come
// from h); the lists of a grouped or cooperative call are then done; and what la_group_last_by_member would read: the offsets at
// po_base and the results at res_base, both device addresses.
void small_unpack(la_ctx* ctx, const HostCall& c, Shard& sh, const SmallLayout& L, const char* h, bool pieces, int n_slots,
                  const char* po_base, const char* res_base) {
    CopyPiece cp[kStagedOuts];
    int n = 0;
    for (int s = 0; s < n_slots; ++s)
        if (L.out[s].to && L.out[s].bytes) cp[n++] = {L.out[s].to, h + L.out[s].off, L.out[s].bytes};
    if (pieces) copy_pieces(ctx, cp, n);
    else for (int i = 0; i < n; ++i) memcpy(cp[i].dst, cp[i].src, cp[i].bytes);
    if (c.g_members >= 0 && c.grouped_done) *c.grouped_done = true;
    if (c.coop) *c.coop_done = true;
    sh.last_part_off = (const int64_t*)(po_base + L.po);
    sh.last_out_pid = L.at<const int32_t>(res_base, kOutPid);
    sh.last_out_rank = L.at<const int32_t>(res_base, kOutRank);
}

// One group_by_member launch over the results of a staged call: offsets at po_base, results in the device buffer d, the lists to
// lists_base (fin_flag / finished: the launch may also finish a zero-copy call, see assign_small_zc).
hipError_t small_group_launch(const HostCall& c, Lane& ln, const SmallLayout& L, const char* po_base, const char* d,
                              char* lists_base, uint32_t* status, hipStream_t st, uint32_t* fin_flag = nullptr,
                              bool* finished = nullptr) {
    return la::group_by_member_launch(ln.large, c.shape.n, c.g_members, c.T, (const int64_t*)(po_base + L.po),
                                      L.at<const int32_t>(d, kOutPid), L.at<const int32_t>(d, kOutRank),
                                      L.at<int64_t>(lists_base, kOutMemberOff), L.want<int32_t>(lists_base, kOutListTopic),
                                      L.at<int32_t>(lists_base, kOutListPartition), nullptr, status, st, fin_flag, finished);
}

// The round of a fused cooperative call, both forms: the owned arrays at m (the device's view of the staging buffer) and every
// output to m.  The target is the caller's to add.
la::CoopRoundCall small_coop_round(const HostCall& c, const SmallLayout& L, char* m) {
    la::CoopRoundCall r = *c.coop;
    const bool owned = r.c.n_owned > 0;
    r.c.owned_off = owned ? (const int64_t*)(m + L.oo) : nullptr;
    r.c.owned_topic = owned ? (const int32_t*)(m + L.otp) : nullptr;
    r.c.owned_partition = owned ? (const int32_t*)(m + L.opp) : nullptr;
    r.c.member_kept = L.want<int64_t>(m, kOutKept);
    r.c.member_fresh = L.want<int64_t>(m, kOutFresh);
    r.c.member_pending = L.want<int64_t>(m, kOutPending);
    r.c.member_release = L.want<int64_t>(m, kOutRelease);
    r.c.topic_withheld = L.want<int64_t>(m, kOutWithheld);
    r.c.summary = L.want<int64_t>(m, kOutSummary);
    r.c.prev_owner = L.want<int32_t>(m, kOutPrevOwner);
    r.c.coop_rank = L.want<int32_t>(m, kOutCoopRank);
    r.member_off = L.at<int64_t>(m, kOutMemberOff);
    r.grouped_topic = L.want<int32_t>(m, kOutListTopic);
    r.grouped_partition = L.at<int32_t>(m, kOutListPartition);
    return r;
}

// la_assign_batch_cooperative, fused form: the round of a zero-copy call as its last launch.  The target at d (device memory),
// the part offsets at m, the completion word where the calling thread spins.
hipError_t small_coop_launch(const HostCall& c, Lane& ln, const SmallLayout& L, char* m, const char* d, hipStream_t st) {
    la::CoopRoundCall r = small_coop_round(c, L, m);
    r.c.n_topics = c.T;
    r.c.n_partitions = c.shape.n;
    r.c.part_off = (const int64_t*)(m + L.po);
    r.c.out_partition = L.at<const int32_t>(d, kOutPid);
    r.c.out_member_rank = L.at<const int32_t>(d, kOutRank);
    return la::cooperative_round_finish_launch(r, L.want<int32_t>(m, kOutPid), L.want<int32_t>(m, kOutRank), ln.d_status,
                                               (uint32_t*)(m + L.status), st);
}

// la_assign_batch_cooperative_sticky, fused form: the STICKY round of a zero-copy call as its last launch.  The batch is the staged
// one -- the target at d (device memory); offsets, input ids and the lag source at m as small_fill_inputs staged them (the lags in
// the slot of the end offsets, the sparse list scattered into a dense array, no begin at all under LA_RESET_LATEST); the hint is
// the largest topic -- and goes through the checks of the device call; the owned arrays at m, every output to m, the completion
// word where the calling thread spins.
int small_coop_sticky_launch(la_ctx* ctx, const HostCall& c, Lane& ln, const SmallLayout& L, char* m, char* d, hipStream_t st) {
    const la_device_batch b = small_batch(c, L, m, d);
    la_coop_sticky_args a{};
    a.struct_size = (int32_t)sizeof a;
    a.round = coop_round_args_of(small_coop_round(c, L, m));
    a.d_sticky_partition = L.at<int32_t>(m, kOutSticky);
    a.d_topic_kept = L.want<int64_t>(m, kOutTopicKept);
    a.d_topic_saved = L.want<int64_t>(m, kOutTopicSaved);
    a.d_sticky_summary = L.want<int64_t>(m, kOutStickySummary);
    la::CoopStickyCall k{};
    if (int rc = coop_sticky_call_of(ctx, &b, &a, &k)) return rc;
    k.s.sticky = L.want<int32_t>(m, kOutSticky);               // (the finishing form alone: no trip over the link for ids nobody reads)
    const hipError_t e = la::cooperative_round_sticky_finish_launch(k, L.want<int32_t>(m, kOutPid), L.want<int32_t>(m, kOutRank),
                                                                    ln.d_status, (uint32_t*)(m + L.status), st);
    return e != hipSuccess ? hip_fail(ctx, e, "cooperative_round_sticky: %s") : LA_OK;
}

// The tail (lists + completion word) a zero-copy call asks the dispatcher to hang on its batch b's tile launch; false: none.
// ONE launch for the whole rebalance where the batch is one resident tile launch: its last workgroup builds the lists and
// stores the completion word -- otherwise the grouping / finishing launches of small_zc_enqueue.  Where that pays was measured at
// the C ABI (profiles/r05_ae_fused_tail.txt): with lists, 100 / 500 partitions 22-24 / 25 us fused against 25 / 26.5 us with the
// one-workgroup grouping as its own launch, but 2 000 partitions 37-38 against 34 -- the tail is 256 threads of the tile
// kernel, the grouping kernel 1 024, and every workgroup of a fused launch pays a system-scope fence -- so the lists are fused
// up to kTailMaxEntries entries; a call WITHOUT lists is faster with the plain finishing launch at every size (100
// partitions 16.6 against 18.6 us, 10 000: 31 against 38) and never takes the tail.  LA_FUSED_TAIL=all restores round
// 5's first form (every staged call that can), LA_NO_FUSED_TAIL=1 never fuses.
bool small_tail_request(const HostCall& c, const SmallLayout& L, Lane& ln, const char* m, const la_device_batch& b, la::TileTail* t) {
    static const bool no_tail = getenv("LA_NO_FUSED_TAIL") != nullptr;                 // (A/B hooks)
    static const bool tail_all = [] { const char* e = getenv("LA_FUSED_TAIL"); return e && !strcmp(e, "all"); }();
    const bool grouped = c.g_members >= 0;
    const bool one_wg_lists = grouped ? (c.shape.n <= (tail_all ? la::kSmallGroupN : la::kTailMaxEntries) &&
                                         (int64_t)c.g_members + 2 <= la::kTailGroupM)
                                      : tail_all;
    // (a cooperative call never: its round is its own 1 024-thread launch)
    if (!one_wg_lists || no_tail || (size_t)c.shape.k > kSmallHostCheck || c.coop) return false;
    *t = la::TileTail{};
    t->enabled = 1;
    t->n_members = grouped ? c.g_members : 0;
    t->n = (int32_t)c.shape.n; t->n_topics = c.T;
    t->part_off = (const int64_t*)(m + L.po);
    t->out_pid = b.d_out_partition; t->out_rank = b.d_out_member_rank;
    t->member_off = L.want<int64_t>(m, kOutMemberOff);
    t->grouped_topic = L.want<int32_t>(m, kOutListTopic);
    t->grouped_partition = L.want<int32_t>(m, kOutListPartition);
    t->counter = ln.d_status + 24;
    t->fin_flag = (uint32_t*)(m + L.status);
    return true;
}

// Puts the lane's status word, and with `tail_counter` the counter of the tile kernel's tail, back to zero behind whatever is
// on the stream: the next call must not inherit bits that kernels of a failed one OR-ed in, nor workgroups they counted done
// (ADVICE r4).
hipError_t lane_words_reset(Lane& ln, hipStream_t st, bool tail_counter) {
    const hipError_t e = hipMemsetAsync(ln.d_status, 0, sizeof(uint32_t), st);
    if (tail_counter) (void)hipMemsetAsync(ln.d_status + 24, 0, sizeof(uint32_t), st);
    return e;
}

// The kernels of a zero-copy call: the batch, and the launch that ends the call by storing `done | status` into the completion
// word -- the tile kernel's tail, the one-workgroup grouping, the cooperative round, or else a finishing launch of its own.
int small_zc_enqueue(la_ctx* ctx, const HostCall& c, Lane& ln, const SmallLayout& L, char* m, char* d, char* res, hipStream_t st) {
    uint32_t* const fin_flag = (uint32_t*)(m + L.status);
    // the totals: only when the caller wants them (device_batch)
    const la_device_batch b = small_batch(c, L, m, res);
    la::TileTail tail;
    StagedBatch staged;
    if (small_tail_request(c, L, ln, m, b, &tail)) staged.tail = &tail;
    if (int rc = enqueue_batch(ctx, ln, &b, st, &staged)) return rc;
    bool finished = staged.tail_done;                                    // (the one-workgroup grouping also finishes the call)
    if (c.g_members >= 0 && !finished)
        if (const hipError_t e = small_group_launch(c, ln, L, m, d, m, ln.d_status, st, fin_flag, &finished); e != hipSuccess)
            return hip_fail(ctx, e, "group_by_member: %s");
    if (c.coop && c.sticky) {
        if (int rc = small_coop_sticky_launch(ctx, c, ln, L, m, d, st)) return rc;
        finished = true;
    } else if (c.coop) {
        if (const hipError_t e = small_coop_launch(c, ln, L, m, d, st); e != hipSuccess) return hip_fail(ctx, e, "cooperative_round: %s");
        finished = true;
    }
    if (!finished)
        if (const hipError_t e = la::finish_status_launch(ln.d_status, fin_flag, st); e != hipSuccess)
            return fail(ctx, LA_EHIP, "finish launch: %s", hipGetErrorString(e));
    return LA_OK;
}

// The wait of a zero-copy call: a spin on the completion word; should it never come (a fault on the stream), the runtime will
// say why.  *status <- what the kernels flagged.
int small_zc_wait(la_ctx* ctx, Lane& ln, volatile uint32_t* flag, hipStream_t st, uint32_t* status) {
    uint32_t f = 0;
    for (uint64_t spins = 0;; ++spins) {
        f = *flag;
        if (f & 0x80000000u) break;
        if ((spins & 0xFFFu) == 0xFFFu) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) { f = *flag; if (f & 0x80000000u) break; LA_HIP(ctx, hipStreamSynchronize(st)); f = *flag | 0x80000000u; break; }
            if (q != hipErrorNotReady) {
                (void)lane_words_reset(ln, st, true);                                // (best effort after a stream error)
                return fail(ctx, LA_EHIP, "zero-copy call: %s", hipGetErrorString(q));
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    *status = f & 0x7FFFFFFFu;
    return LA_OK;
}

int assign_small_zc(la_ctx* ctx, const HostCall& c, Shard& sh, const SmallLayout& L) {
    LA_HIP(ctx, hipSetDevice(sh.device));
    Lane& ln = sh.lanes[0];
    hipStream_t st = ln.stream;
    if (int rc = reserve_host(ctx, sh.zc_h, L.total, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent)) return rc;
    if (int rc = reserve(ctx, sh.small_d, L.total)) return rc;           // the ungrouped result (same layout, device side)
    char* h = (char*)sh.zc_h.p;
    char* d = (char*)sh.small_d.p;
    void* hd = nullptr;                                                  // the device's view of the staging buffer
    LA_HIP(ctx, hipHostGetDevicePointer(&hd, h, 0));
    char* m = (char*)hd;
    if (int rc = small_fill_inputs(ctx, c, L, h)) return rc;
    volatile uint32_t* flag = (volatile uint32_t*)(h + L.status);
    *flag = 0;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    if ((size_t)c.shape.k > kSmallHostCheck)
        LA_HIP(ctx, la::check_consumers_launch(c.T, (const int64_t*)(m + L.co), (const int32_t*)(m + L.cr), ln.d_status, st));
    const bool grouped = c.g_members >= 0;
    // results the caller reads go to the host's memory; those only the grouping reads stay on the device
    // (a cooperative call: the round reads the target on the device and hands it on to the host itself where it is wanted)
    char* res = (c.out_pid && !grouped && !c.coop) ? m : d;
    if (int rc = small_zc_enqueue(ctx, c, ln, L, m, d, res, st)) {
        // nothing of this call stays in flight or behind: kernels already enqueued may have OR-ed bits into the lane's status word
        // (and counted themselves done on the tail's counter)
        (void)hipStreamSynchronize(st);
        (void)lane_words_reset(ln, st, true);
        (void)hipStreamSynchronize(st);
        return rc;
    }
    uint32_t status = 0;
    if (int rc = small_zc_wait(ctx, ln, flag, st, &status)) return rc;
    if (status) {
        // The completion word has arrived, so the tail's counter needs nothing: a launch that carried the tail has put it back to
        // zero itself before it stored the word (tile_tail: "the next call's count"), and no other launch of the call touches it.
        // The status word does: the tail and the grouping launch read it and leave it as it is.
        LA_HIP(ctx, lane_words_reset(ln, st, false));
        LA_HIP(ctx, hipStreamSynchronize(st));
        return status_error(ctx, status);
    }
    if (grouped && c.out_pid && c.shape.n) {
        // (no caller asks for both forms today: the ungrouped arrays would need their own trip)
        const size_t nb4 = (size_t)c.shape.n * 4;
        LA_HIP(ctx, hipMemcpyAsync(c.out_pid, L.at<int32_t>(d, kOutPid), nb4, hipMemcpyDeviceToHost, st));
        LA_HIP(ctx, hipMemcpyAsync(c.out_rank, L.at<int32_t>(d, kOutRank), nb4, hipMemcpyDeviceToHost, st));
        LA_HIP(ctx, hipStreamSynchronize(st));
    }
    // what la_group_last_by_member would read: valid only where the results stayed on the device
    small_unpack(ctx, c, sh, L, h, /*pieces=*/true, grouped ? kOutPid : kStagedOuts, m, res);
    return LA_OK;
}

int assign_small(la_ctx* ctx, const HostCall& c, Shard& sh, const SmallLayout& L) {
    LA_HIP(ctx, hipSetDevice(sh.device));
    Lane& ln = sh.lanes[0];
    hipStream_t st = ln.stream;
    if (int rc = reserve(ctx, sh.small_d, L.total)) return rc;
    if (int rc = reserve_host(ctx, sh.small_h, L.total)) return rc;
    char* h = (char*)sh.small_h.p;
    char* d = (char*)sh.small_d.p;
    if (int rc = small_fill_inputs(ctx, c, L, h)) return rc;
    memset(h + L.status, 0, 256);
    LA_HIP(ctx, hipMemcpyAsync(d, h, L.status + 256, hipMemcpyHostToDevice, st));
    // the status word of this call's kernels lives inside its device staging buffer: uploaded as zero with the inputs,
    // downloaded with the results
    StagedBatch staged;
    staged.status = (uint32_t*)(d + L.status);
    if ((size_t)c.shape.k > kSmallHostCheck)
        LA_HIP(ctx, la::check_consumers_launch(c.T, (const int64_t*)(d + L.co), (const int32_t*)(d + L.cr), staged.status, st));
    const la_device_batch b = small_batch(c, L, d, d);
    int rc = enqueue_batch(ctx, ln, &b, st, &staged);
    // every member's list, built where the results are: one more launch on the same stream, no second round trip
    if (rc == LA_OK && c.g_members >= 0)
        if (const hipError_t e = small_group_launch(c, ln, L, d, d, d, staged.status, st); e != hipSuccess)
            rc = hip_fail(ctx, e, "group_by_member: %s");
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    // status | totals | (member_off | grouped topic | grouped partition) | partition order | member ranks: as far as the caller wants them
    const size_t upto = c.out_pid ? L.total : L.out[kOutPid].off;
    LA_HIP(ctx, hipMemcpyAsync(h + L.status, d + L.status, upto - L.status, hipMemcpyDeviceToHost, st));
    LA_HIP(ctx, hipStreamSynchronize(st));
    const uint32_t status = *(const uint32_t*)(h + L.status);
    if (status) return status_error(ctx, status);
    small_unpack(ctx, c, sh, L, h, /*pieces=*/false, kStagedOuts, d, d);
    return LA_OK;
}

// grouping of one shard's last results, on its lane 0, into the given device arrays (null: the shard's own pid =
// grouped partition, cons_rank = grouped topic with shard-local indices, out_total = member_off -- their old contents
// are no longer needed)
int group_shard_device(la_ctx* ctx, Shard& sh, int32_t n_members, bool want_topic, int64_t* d_off = nullptr,
                       int32_t* d_topic = nullptr, int32_t* d_part = nullptr) {
    const int64_t n = sh.last_n;
    if (n > 0x7FFFFFFF) return fail(ctx, LA_ESHAPE, "at most 2^31-1 entries per shard are supported");
    if (!d_off) {
        const size_t nb4 = (size_t)n * 4, mb = ((size_t)n_members + 1) * 8;
        int rc;
        if ((rc = reserve(ctx, sh.pid, nb4 + 16)) || (rc = reserve(ctx, sh.cons_rank, nb4 + 16)) ||
            (rc = reserve(ctx, sh.out_total, mb + 16)))
            return rc;
        d_off = (int64_t*)sh.out_total.p;
        d_topic = (int32_t*)sh.cons_rank.p;
        d_part = (int32_t*)sh.pid.p;
    }
    hipError_t e = la::group_by_member_launch(sh.lanes[0].large, n, n_members, sh.last_topics, sh.last_part_off,
                                              sh.last_out_pid, sh.last_out_rank, d_off, want_topic ? d_topic : nullptr,
                                              d_part, nullptr, sh.lanes[0].d_status, sh.lanes[0].stream);
    if (e != hipSuccess)
        return hip_fail(ctx, e, "group_by_member: %s");
    return LA_OK;
}

// ... into the shard's own arrays, and that CSR back to the host: the offsets, the topics (null: not wanted) and the partitions.
// Waits, and reports what the grouping's sort flagged through the lane's status word.
int group_shard_to_host(la_ctx* ctx, Shard& sh, int32_t n_members, int64_t* off, int32_t* topic, int32_t* part) {
    if (int rc = group_shard_device(ctx, sh, n_members, topic != nullptr)) return rc;
    hipStream_t st = sh.lanes[0].stream;
    const size_t nb4 = (size_t)sh.last_n * 4;
    LA_HIP(ctx, hipMemcpyAsync(off, sh.out_total.p, ((size_t)n_members + 1) * 8, hipMemcpyDeviceToHost, st));
    if (sh.last_n) {
        LA_HIP(ctx, hipMemcpyAsync(part, sh.pid.p, nb4, hipMemcpyDeviceToHost, st));
        if (topic) LA_HIP(ctx, hipMemcpyAsync(topic, sh.cons_rank.p, nb4, hipMemcpyDeviceToHost, st));
    }
    return sync_status(ctx, sh.lanes[0], st);
}

// The caller's side of a call, checked and normalised: the hinted bounds, the shape, which arrays the call needs and reads.
int normalise_call(la_ctx* ctx, HostCall& c, bool hinted) {
    if (!c.part_off || !c.cons_off) return fail(ctx, LA_EINVAL, "null offsets");
    if (hinted && (ctx->hints.flags & LA_HINT_BOUNDS) && ctx->hints.max_lag >= 0 && ctx->hints.max_partition_id >= 0) {
        c.bounded = true;
        c.max_lag = ctx->hints.max_lag;
        c.max_id = ctx->hints.max_partition_id;
    }
    // offsets are checked here; cons_rank's order on the device (chunk_device_work)
    if (int rc = scan_shape(ctx, c.T, c.part_off, c.cons_off, &c.shape)) return rc;
    const Shape& s = c.shape;
    if (s.n > 0 && (!c.pid || (!c.lag && (!c.end || !c.committed)))) return fail(ctx, LA_EINVAL, "null per-partition buffer");
    if ((c.out_pid == nullptr) != (c.out_rank == nullptr))
        return fail(ctx, LA_EINVAL, "out_partition and out_member_rank must both be given or both be NULL");
    if (s.k > 0 && !c.cons_rank) return fail(ctx, LA_EINVAL, "null cons_rank");
    c.sparse = c.sparse && !c.lag && c.reset_mode != LA_RESET_LATEST;      // (`latest` never reads begin: the list is ignored)
    if (c.sparse && (c.n_none < 0 || (c.n_none > 0 && (!c.none_index || !c.none_begin))))
        return fail(ctx, LA_EINVAL, "n_none < 0 or a null sparse-begin array");
    if (!c.lag && c.reset_mode != LA_RESET_LATEST && !c.begin && !c.sparse && s.n > 0)
        return fail(ctx, LA_EINVAL, "begin_off is required unless reset_mode is LA_RESET_LATEST");
    c.use_begin = !c.lag && (c.begin || c.sparse) && c.reset_mode != LA_RESET_LATEST;
    if (c.sparse) {
        c.begin = nullptr;
    } else {
        c.n_none = 0; c.none_index = nullptr; c.none_begin = nullptr;
    }
    return LA_OK;
}

// How the arrays of the call can be reached: pageable, pinned, or pinned and device-mapped (`no_mapped`: the
// LA_NO_MAPPED_PIPELINE hook -- mapped arrays then count as pinned).  Probed when first asked for and kept in the call: the
// probes are two runtime queries per array, and the smallest calls never need them.
enum { kMemPageable, kMemPinned, kMemMapped };

int call_memory(HostCall& c, bool no_mapped) {
    if (c.memory < 0) c.memory = !call_is_pinned(c) ? kMemPageable : (!no_mapped && call_is_mapped(c) ? kMemMapped : kMemPinned);
    return c.memory;
}

// la_assign_batch_cooperative, the GENERAL form: this call becomes a plain assign call into buffers of the context's own
// (totals | ids | ranks), and the entry point runs the round on them -- the caller's arrays see nothing before both have
// succeeded.  (The outputs are other arrays now: their memory is probed anew.)
void coop_take_general(la_ctx* ctx, HostCall& c) {
    ctx->coop_target.resize((size_t)c.shape.k + (size_t)c.shape.n + 1);
    c.out_total = ctx->coop_target.data();
    c.out_pid = (int32_t*)(ctx->coop_target.data() + c.shape.k);
    c.out_rank = c.out_pid + c.shape.n;
    c.coop = nullptr;
    c.sticky = nullptr;
    c.memory = -1;
}

// Whether a one-shard call travels through ONE staging buffer, and with what aboard: *L <- its layout.
// How large a layout still does.  Pageable caller arrays: kSmallBytes (12 MB) -- beyond, packing the inputs costs as much as the
// lanes' overlapped copies.  Caller arrays that are pinned need no packing at all on the other side of the comparison:
// device-mapped ones (la_host_alloc: the Java host's direct buffers) are read in place by the kernels from 1.25 MB on (3 MB with
// the lists aboard, which the staged form brings back in the same round trip); pinned but not mapped ones keep round 4's 2 MB.
// profiles/r05_o_latency_probe.txt.
bool stage_decision(la_ctx* ctx, HostCall& c, bool no_mapped, SmallLayout* L) {
    auto fits = [&](bool with_lists) {
        size_t upto = kSmallBytes;
        if (L->total > kMappedSmallBytes && call_memory(c, no_mapped) != kMemPageable) {
            const size_t lim = c.memory == kMemMapped ? (with_lists ? kMappedSmallGroupedBytes : kMappedSmallBytes) : kPinnedSmallBytes;
            if (lim < upto) upto = lim;
        }
        return L->total <= upto;
    };
    *L = small_layout(c);
    // (a cooperative call is FUSED only as a zero-copy staged call)
    if (fits(c.g_members >= 0) && !(c.coop && L->total > ctx->zero_copy_bytes)) return true;
    // too large with everything aboard: the round of a cooperative call follows the call, the lists of a grouped one take their
    // own round trip (no call is both) -- and what is left is asked once more
    if (c.coop) coop_take_general(ctx, c);
    else if (c.g_members >= 0) c.g_members = -1;
    else return false;
    *L = small_layout(c);
    return fits(false);
}

// The chunked pipelines over the S shards of ctx->last_bounds: the caller's arrays read in place (mapped), sent over three
// streams by this thread (pinned), or by a host thread per lane (pageable).
int run_pipelines(la_ctx* ctx, HostCall& c, int S, bool no_mapped) {
    std::vector<ShardPlan> plans((size_t)S);
    struct Work { int shard, lane; };
    std::vector<Work> work;
    const bool pinned = call_memory(c, no_mapped) != kMemPageable;
    c.mapped = c.memory == kMemMapped;
    ctx->last_pipeline = c.mapped ? LA_PIPELINE_MAPPED : (pinned ? 2 : 1);
    for (int i = 0; i < S; ++i) {
        ShardPlan& sp = plans[(size_t)i];
        Shard& sh = ctx->shards[(size_t)i];
        sp.t0 = ctx->last_bounds[i];
        sp.t1 = ctx->last_bounds[i + 1];
        sp.P0 = c.part_off[sp.t0]; sp.n = c.part_off[sp.t1] - sp.P0;
        sp.K0 = c.cons_off[sp.t0]; sp.k = c.cons_off[sp.t1] - sp.K0;
        sh.last_t0 = sp.t0; sh.last_topics = sp.t1 - sp.t0; sh.last_p0 = sp.P0; sh.last_n = sp.n;
        if (sp.t1 == sp.t0) continue;
        const int rc_prepare = prepare_shard(ctx, c, sh, sp);
        sh.last_part_off = (const int64_t*)sh.part_off.p;       // (after the reserves of prepare_shard)
        sh.last_out_pid = (const int32_t*)sh.out_pid.p;
        sh.last_out_rank = (const int32_t*)sh.out_rank.p;
        if (int rc = rc_prepare) {
            for (int j = 0; j <= i; ++j)                         // nothing of this call stays in flight
                if (hipSetDevice(ctx->shards[(size_t)j].device) == hipSuccess)
                    (void)hipStreamSynchronize(ctx->shards[(size_t)j].lanes[0].stream);
            return rc;
        }
        if (c.mapped && c.out_pid) {
            // the kernels wrote the ungrouped results into the caller's own (mapped) arrays: that is where a following
            // la_group_last_by_member reads them, in place
            sh.last_out_pid = mapped_ptr(c.out_pid) + sp.P0;
            sh.last_out_rank = mapped_ptr(c.out_rank) + sp.P0;
        }
        const int n_chunks = (int)sp.chunk.size() - 1;
        const int lanes = n_chunks < (int)sh.lanes.size() ? n_chunks : (int)sh.lanes.size();
        if (!pinned)
            for (int l = 0; l < lanes; ++l) work.push_back({i, l});
    }
    if (pinned) {
        // pinned caller arrays: this thread enqueues every shard's chunks (nothing blocks), then waits shard by shard
        int rc = LA_OK;
        for (int i = 0; i < S && rc == LA_OK; ++i)
            if (plans[(size_t)i].t1 > plans[(size_t)i].t0)
                rc = c.mapped ? run_shard_mapped(ctx, c, ctx->shards[(size_t)i], plans[(size_t)i])
                              : run_shard_async(ctx, c, ctx->shards[(size_t)i], plans[(size_t)i]);
        for (int i = 0; i < S; ++i) {
            if (plans[(size_t)i].t1 == plans[(size_t)i].t0) continue;
            const int rf = finish_shard_async(ctx, ctx->shards[(size_t)i]);
            if (rc == LA_OK) rc = rf;
        }
        return rc;
    }
    std::atomic<bool> stop{false};
    return run_workers(ctx, (int)work.size(), [&](int w) {
        const Work& wk = work[(size_t)w];
        const int r = run_lane(ctx, c, ctx->shards[(size_t)wk.shard], plans[(size_t)wk.shard], wk.lane, stop);
        if (r != LA_OK) stop.store(true, std::memory_order_relaxed);
        return r;
    });
}

}  // namespace

// ---- planner: contiguous topic ranges balanced by partition count -----------------------------------------
// The shard axis is the per-topic loop of assign(Map,Map) (Main.java:177-184): assignTopic touches only its own
// topic's bins, so any split at topic boundaries is valid; the kernels' cost is per partition, so the split
// balances partitions.  bounds[r] = first topic boundary at or after r/parts of the partitions.  Every topic
// lands in exactly one range; ranges may be empty.  Used for shards (devices) and for the chunks of one shard.
void plan_ranges(const int64_t* po, int32_t t_begin, int32_t t_end, int parts, int32_t* bounds) {
    const int64_t base = po[t_begin], total = po[t_end] - base;
    bounds[0] = t_begin;
    for (int r = 1; r < parts; ++r) {
        const int64_t target = base + (total / parts) * r + (total % parts) * r / parts;
        const int64_t* lo = std::lower_bound(po + bounds[r - 1], po + t_end + 1, target);
        int64_t t = lo - po;
        if (t > t_end) t = t_end;
        bounds[r] = (int32_t)t;
    }
    bounds[parts] = t_end;
}

// The size up to which a staged call runs zero-copy: the default, and its lab override read once per context.
void host_defaults(la_ctx* ctx) {
    ctx->zero_copy_bytes = kZeroCopyBytes;
    if (const char* env = getenv("LA_ZERO_COPY_BYTES")) ctx->zero_copy_bytes = (size_t)atoll(env);
}

// One host-buffer assign call.  The entry point has filled in what it was given -- the arrays, the sparse trio behind `sparse`,
// the grouped quartet behind g_members >= 0 -- and everything else of `c` is worked out here.
int assign_host(la_ctx* ctx, HostCall& c) {
    if (!ctx) return LA_EINVAL;
    ctx->last_valid = false;
    const bool hinted = ctx->hints_set;                       // one-shot: whatever this call returns, the hints are spent
    ctx->hints_set = false;
    const int32_t T = c.T;
    if (T < 0) return fail(ctx, LA_EINVAL, "n_topics < 0");
    if (T == 0) return LA_OK;
    if (int rc = normalise_call(ctx, c, hinted)) return rc;
    const Shape& s = c.shape;
    // the one environment hook of a call, read at every call (tests and the benchmark flip it around live contexts)
    const bool no_mapped = getenv("LA_NO_MAPPED_PIPELINE") != nullptr;

    // shards: all devices for a batch worth splitting, fewer (down to one) for a small one
    int S = (int)ctx->shards.size();
    if (!ctx->split_always) {
        const int64_t by_size = s.n / kMinShardPartitions;
        if (by_size < S) S = by_size < 1 ? 1 : (int)by_size;
    }
    if (S > T) S = T;
    plan_ranges(c.part_off, 0, T, S, ctx->last_bounds);
    ctx->last_shards = S;
    const bool may_stage = S == 1 && !ctx->split_always && s.n > 0;
    // la_assign_batch_cooperative[_sticky].  FUSED: a zero-copy staged call within the (sticky) round kernel's limits.  Anything
    // else, and whatever the entry point asks for with coop_general (LA_COOP_FORCE_TABLE, the sticky call's LA_NO_FUSED_STICKY),
    // is the GENERAL form (coop_take_general).
    if (c.coop) {
        la::CoopCall probe = c.coop->c;
        probe.n_topics = T;
        probe.n_partitions = s.n;
        const bool small = c.sticky ? la::coop_sticky_is_small(probe) : la::coop_round_is_small(probe);
        if (!may_stage || c.coop_general || !small) coop_take_general(ctx, c);
    }
    SmallLayout L;
    int rc;
    if (may_stage && stage_decision(ctx, c, no_mapped, &L)) {
        Shard& sh = ctx->shards[0];
        sh.last_t0 = 0; sh.last_topics = T; sh.last_p0 = 0; sh.last_n = s.n;
        const bool zc = L.total <= ctx->zero_copy_bytes;
        ctx->last_pipeline = zc ? LA_PIPELINE_ZERO_COPY : LA_PIPELINE_ONE_COPY;
        rc = zc ? assign_small_zc(ctx, c, sh, L) : assign_small(ctx, c, sh, L);
    } else {
        rc = run_pipelines(ctx, c, S, no_mapped);
    }
    if (rc) return rc;
    ctx->last_valid = true;
    return LA_OK;
}

// Every member's list from the results the shards hold (Shard::last_*): one shard -> its CSR straight into the caller's
// arrays; several -> grouped per shard on its device, merged by offset on the host.
int group_last_impl(la_ctx* ctx, int32_t n_members, int64_t* member_off, int32_t* grouped_topic, int32_t* grouped_partition) {
    const int S = ctx->last_shards;
    int64_t n = 0;
    for (int i = 0; i < S; ++i) n += ctx->shards[(size_t)i].last_n;
    if (!member_off || (n > 0 && !grouped_partition)) return fail(ctx, LA_EINVAL, "null buffer");
    const size_t mb = ((size_t)n_members + 1) * 8;
    if (S == 1) {
        // one shard: its CSR is the answer, straight into the caller's arrays
        Shard& sh = ctx->shards[0];
        LA_HIP(ctx, hipSetDevice(sh.device));
        hipStream_t st = sh.lanes[0].stream;
        const size_t nb4 = (size_t)n * 4;
        const size_t o_topic = (mb + 16 + 255) & ~(size_t)255, o_part = (o_topic + nb4 + 16 + 255) & ~(size_t)255;
        const size_t g_total = o_part + nb4 + 16;
        if (g_total <= kGroupStageBytes) {
            // small batch: the CSR is built in one staging buffer and crosses in one copy (see assign_small)
            int rc;
            if ((rc = reserve(ctx, sh.small_g, g_total)) || (rc = reserve_host(ctx, sh.small_gh, g_total))) return rc;
            char* d = (char*)sh.small_g.p;
            char* h = (char*)sh.small_gh.p;
            if ((rc = group_shard_device(ctx, sh, n_members, grouped_topic != nullptr, (int64_t*)d,
                                         (int32_t*)(d + o_topic), (int32_t*)(d + o_part))))
                return rc;
            LA_HIP(ctx, hipMemcpyAsync(h, d, g_total, hipMemcpyDeviceToHost, st));
            if ((rc = sync_status(ctx, sh.lanes[0], st))) return rc;    // the grouping's sort reports through the lane's status word
            memcpy(member_off, h, mb);
            if (n) {
                memcpy(grouped_partition, h + o_part, nb4);
                if (grouped_topic) memcpy(grouped_topic, h + o_topic, nb4);
            }
            return LA_OK;
        }
        return group_shard_to_host(ctx, sh, n_members, member_off, grouped_topic, grouped_partition);
    }
    // Several shards.  A member's list is its per-topic appends in topic order (Main.java:177-184, :264), and the
    // shards are contiguous topic ranges: the list is the concatenation, in shard order, of the shards' lists.
    // Phase 1, per shard in parallel: group on the device, CSR into pinned staging.  Then the global offsets
    // (a scan over members x shards on the host), then phase 2, per shard in parallel: every member's slice to
    // its place in the caller's arrays, topic indices moved from shard-local to the caller's numbering.
    int rc = run_workers(ctx, S, [&](int i) -> int {
        Shard& sh = ctx->shards[(size_t)i];
        if (sh.last_topics == 0) return LA_OK;
        LA_HIP(ctx, hipSetDevice(sh.device));
        const size_t nb4 = (size_t)sh.last_n * 4;
        int r;
        if ((r = reserve_host(ctx, sh.g_off, mb)) || (r = reserve_host(ctx, sh.g_part, nb4 + 16)) ||
            (grouped_topic && (r = reserve_host(ctx, sh.g_topic, nb4 + 16))))
            return r;
        return group_shard_to_host(ctx, sh, n_members, (int64_t*)sh.g_off.p, grouped_topic ? (int32_t*)sh.g_topic.p : nullptr,
                                   (int32_t*)sh.g_part.p);
    });
    if (rc) return rc;
    // group g = 0 is "no consumer" (rank -1: the entries before member_off[0]), g = r + 1 is member r
    const size_t G = (size_t)n_members + 1;
    // shard sh's entries of group g: [lo, hi) of its CSR
    auto slice = [G](const Shard& sh, size_t g, int64_t& lo, int64_t& hi) {
        const int64_t* so = (const int64_t*)sh.g_off.p;
        lo = g == 0 ? 0 : so[g - 1];
        hi = g == G - 1 ? sh.last_n : so[g];
    };
    std::vector<int64_t> base((size_t)S * G);          // destination of shard i's slice of group g
    {
        int64_t run = 0;
        for (size_t g = 0; g < G; ++g) {
            if (g >= 1) member_off[g - 1] = run;
            for (int i = 0; i < S; ++i) {
                const Shard& sh = ctx->shards[(size_t)i];
                base[(size_t)i * G + g] = run;
                if (sh.last_topics == 0) continue;
                int64_t lo, hi;
                slice(sh, g, lo, hi);
                run += hi - lo;
            }
        }
        member_off[n_members] = run;
    }
    rc = run_workers(ctx, S, [&](int i) -> int {
        const Shard& sh = ctx->shards[(size_t)i];
        if (sh.last_topics == 0 || sh.last_n == 0) return LA_OK;
        const int32_t* sp = (const int32_t*)sh.g_part.p;
        const int32_t* stp = (const int32_t*)sh.g_topic.p;
        for (size_t g = 0; g < G; ++g) {
            int64_t lo, hi;
            slice(sh, g, lo, hi);
            if (hi <= lo) continue;
            const int64_t dst = base[(size_t)i * G + g];
            memcpy(grouped_partition + dst, sp + lo, (size_t)(hi - lo) * 4);
            if (grouped_topic) {
                int32_t* gt = grouped_topic + dst;
                const int32_t t0 = sh.last_t0;
                for (int64_t j = lo; j < hi; ++j) gt[j - lo] = stp[j] + t0;
            }
        }
        return LA_OK;
    });
    return rc;
}

// A grouped call: every member's list (c.g_members, c.g_off, c.g_topic, c.g_part) instead of the ungrouped arrays.
int assign_grouped(la_ctx* ctx, HostCall& c) {
    const int32_t n_topics = c.T, n_members = c.g_members;
    const int64_t* part_off = c.part_off;
    int64_t* member_off = c.g_off;
    int32_t *grouped_topic = c.g_topic, *grouped_partition = c.g_part;
    if (n_members < 0) return fail(ctx, LA_EINVAL, "negative size");
    if (!member_off) return fail(ctx, LA_EINVAL, "member_off is NULL");
    if (n_topics > 0 && part_off && part_off[n_topics] > 0 && !grouped_partition)
        return fail(ctx, LA_EINVAL, "grouped_partition is NULL");
    if (n_topics <= 0) {                                        // nothing assigned: every member's list is empty
        if (n_topics < 0) return fail(ctx, LA_EINVAL, "n_topics < 0");
        ctx->last_valid = false;
        for (int32_t r = 0; r <= n_members; ++r) member_off[r] = 0;
        return LA_OK;
    }
    bool done = false;
    c.grouped_done = &done;
    c.out_pid = nullptr; c.out_rank = nullptr;
    if (int rc = assign_host(ctx, c)) return rc;
    if (done) return LA_OK;                                      // a small call: the lists came back with the totals
    if (!ctx->last_valid) {                                      // (no partitions at all)
        for (int32_t r = 0; r <= n_members; ++r) member_off[r] = 0;
        return LA_OK;
    }
    return group_last_impl(ctx, n_members, member_off, grouped_topic, grouped_partition);
}
