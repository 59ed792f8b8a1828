// la_api.hip -- the C ABI of include/lagassign.h over the HIP kernels (the cooperative and sticky entry points: la_api_coop.hip).
//
// There is no CPU fallback here by design: if the device or a kernel is unavailable the
// call fails with a negative code and the caller decides what to do.
#include "la_ctx.h"

#include <dlfcn.h>

namespace {

constexpr int kMaxShards = 64;

// ---- RCCL, loaded at run time (la_allgather_results) ------------------------------------------------------------------
// Only the five entry points the all-gather needs; prototypes as in rccl.h (ncclResult_t is an int enum, 0 = success;
// ncclInt32 = 2).  A copy of the library that the process has already loaded wins: a process that carries its own ROCm
// runtime (PyTorch does) must not get a second one through /opt/rocm's librccl.
struct RcclApi {
    void* handle = nullptr;
    int (*CommInitAll)(void** comms, int ndev, const int* devlist) = nullptr;
    int (*CommDestroy)(void* comm) = nullptr;
    int (*AllGather)(const void* send, void* recv, size_t count, int datatype, void* comm, hipStream_t stream) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string why;
};

RcclApi& rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        const char* names[] = {"librccl.so", "librccl.so.1"};
        for (const char* n : names)
            if (!api.handle) api.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD);       // already in the process?
        for (const char* n : names)
            if (!api.handle) api.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (!api.handle) { api.why = std::string("librccl not found: ") + (dlerror() ? dlerror() : "?"); return; }
        auto sym = [&](const char* name) { return dlsym(api.handle, name); };
        api.CommInitAll = (decltype(api.CommInitAll))sym("ncclCommInitAll");
        api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
        api.AllGather = (decltype(api.AllGather))sym("ncclAllGather");
        api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
        api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
        api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
        if (!api.CommInitAll || !api.CommDestroy || !api.AllGather || !api.GroupStart || !api.GroupEnd) {
            api.why = "librccl lacks ncclCommInitAll / ncclAllGather / ncclGroupStart";
            api.handle = nullptr;
        }
    });
    return api;
}

int create_lane(Lane& ln) {
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipMalloc((void**)&ln.d_status, 256)) != hipSuccess ||
        // zeroed ON the lane's stream and waited for: the stream is non-blocking, so a null-stream hipMemset is not ordered
        // before the first kernel launched on it -- a context whose very first call came right behind la_create could find
        // the status word or the fused tail's workgroup counter stale (a small grouped call then came back with empty lists;
        // found by la_wake's test in round 6: hipMalloc hands back memory a destroyed context had used)
        (e = hipMemsetAsync(ln.d_status, 0, 256, ln.stream)) != hipSuccess ||
        (e = hipStreamSynchronize(ln.stream)) != hipSuccess ||
        (e = hipHostMalloc((void**)&ln.h_status, 64, hipHostMallocDefault)) != hipSuccess)
        return hip_fail(nullptr, e, "context setup: %s");
    *ln.h_status = 0;
    return LA_OK;
}

void destroy_lane(Lane& ln) {
    if (ln.stream) (void)hipStreamSynchronize(ln.stream);
    release(ln.defer);
    release(ln.block_list);
    for (Lane::Stage& sg : ln.stage) {
        if (sg.done) { (void)hipEventSynchronize(sg.done); (void)hipEventDestroy(sg.done); }
        if (sg.p) (void)hipHostFree(sg.p);
    }
    la::large_scratch_release(ln.large);
    if (ln.d_status) (void)hipFree(ln.d_status);
    if (ln.h_status) (void)hipHostFree(ln.h_status);
    if (ln.stream) (void)hipStreamDestroy(ln.stream);
}

// ---- dispatcher: which path every topic of a batch takes --------------------------------------------------
//   * tile-sized topics (<= 1 024 partitions, <= 64 consumers): one wave-tile launch over the whole batch that
//     skips the others -- or, when the shapes are ragged enough to pay for it, one launch per shape class over a
//     topic list, so that a few wide topics do not make every topic pay for the widest tile;
//   * up to 8 192 partitions x 2 048 consumers: the block path, one workgroup per topic, one launch per size
//     class over a topic list;
//   * beyond: the large path, topic by topic.
constexpr int kTileClasses = 3;
constexpr int64_t kTileClsP[kTileClasses] = {64, 256, la::kTileMaxPartitions};
constexpr int64_t kTileClsC[kTileClasses] = {8, 32, la::kTileMaxConsumers};
constexpr uint8_t kLargeCode = kTileClasses + la::kBlockClasses;      // codes: tile classes, block classes, large

struct BatchPlan {
    const uint8_t* code = nullptr;                                    // per topic
    struct { int64_t n = 0, mp = 0, mc = 0; } tile[kTileClasses];     // after merging: what each launch holds
    int merged[kTileClasses] = {0, 1, 2};                             // tile class -> the class it is launched with
    bool classed = false;                                             // tile topics go by shape class (lists)
    int64_t n_tile = 0, tile_mp = 0, tile_mc = 0;
    int64_t n_block[la::kBlockClasses] = {};
    int64_t n_block_all = 0, n_large = 0;
    // offsets of the lists in the staged array: block classes first, then tile classes
    int64_t block_at[la::kBlockClasses] = {}, tile_at[kTileClasses] = {};
    int64_t n_lists = 0;
};

// One pass over the host offsets: a class code per topic, counts and maxima; then the tile plan.
int plan_batch(la_ctx* ctx, Lane& ln, const la_device_batch* b, int tile_mode, bool use_block, BatchPlan* plan) {
    const int64_t T = b->n_topics;
    ln.topic_class.resize((size_t)T);
    uint8_t* code = ln.topic_class.data();
    int64_t cnt[kLargeCode + 1] = {};
    int64_t mp[kTileClasses] = {}, mc[kTileClasses] = {};
    bool decreasing = false;
    const int64_t* po = b->h_part_off;
    const int64_t* co = b->h_cons_off;
    for (int64_t t = 0; t < T; ++t) {
        const int64_t p = po[t + 1] - po[t], c = co[t + 1] - co[t];
        decreasing |= (p < 0) | (c < 0);
        uint8_t k;
        if (p <= kTileClsP[0] && c <= kTileClsC[0]) k = 0;
        else if (p <= kTileClsP[1] && c <= kTileClsC[1]) k = 1;
        else if (p <= kTileClsP[2] && c <= kTileClsC[2]) k = 2;
        else if (use_block && la::block_fits(p, c)) k = (uint8_t)(kTileClasses + la::block_class(p, c));
        else k = kLargeCode;
        code[t] = k;
        ++cnt[k];
        if (k < kTileClasses) {
            if (p > mp[k]) mp[k] = p;
            if (c > mc[k]) mc[k] = c;
        }
    }
    if (decreasing) return fail(ctx, LA_EINVAL, "part_off / cons_off decrease");
    plan->code = code;
    for (int k = 0; k < kTileClasses; ++k) {
        plan->tile[k].n = cnt[k]; plan->tile[k].mp = mp[k]; plan->tile[k].mc = mc[k];
        plan->n_tile += cnt[k];
        if (mp[k] > plan->tile_mp) plan->tile_mp = mp[k];
        if (mc[k] > plan->tile_mc) plan->tile_mc = mc[k];
    }
    for (int k = 0; k < la::kBlockClasses; ++k) {
        plan->n_block[k] = cnt[kTileClasses + k];
        plan->n_block_all += cnt[kTileClasses + k];
    }
    plan->n_large = cnt[kLargeCode];

    // tile plan: the sort slots a launch spends = topics x lanes x records per lane of its tile shape
    auto work = [](int64_t n, int64_t p, int64_t c) {
        int L = 0, E = 0;
        la::wave_tile_pick(p, c, &L, &E);
        return (double)n * L * E;
    };
    const bool force = (b->flags & LA_FLAG_SHAPE_CLASSES) != 0;
    if (tile_mode == 0 && (plan->n_tile >= 4096 || force)) {
        for (int k = 0; k + 1 < kTileClasses; ++k) {                    // a launch is not worth a handful of topics
            auto& lo = plan->tile[k];
            auto& hi = plan->tile[k + 1];
            if (lo.n > 0 && lo.n < 1024 && !force) {
                hi.n += lo.n;
                if (lo.mp > hi.mp) hi.mp = lo.mp;
                if (lo.mc > hi.mc) hi.mc = lo.mc;
                lo.n = 0;
                for (int q = 0; q <= k; ++q) if (plan->merged[q] == k) plan->merged[q] = k + 1;
            }
        }
        double split = 0;
        int launches = 0;
        for (const auto& k : plan->tile) if (k.n > 0) { split += work(k.n, k.mp, k.mc); ++launches; }
        // worth it when the sort slots saved (~12 ps each on the device) outweigh the second host pass over
        // the topics (~2 ns each) and the extra launches
        plan->classed = launches >= 2 &&
                        (force || work(plan->n_tile, plan->tile_mp, plan->tile_mc) - split > 170.0 * (double)T + 8e6);
    }
    for (int k = 1; k < la::kBlockClasses; ++k) plan->block_at[k] = plan->block_at[k - 1] + plan->n_block[k - 1];
    plan->tile_at[0] = plan->n_block_all;
    for (int k = 1; k < kTileClasses; ++k) plan->tile_at[k] = plan->tile_at[k - 1] + plan->tile[k - 1].n;
    plan->n_lists = plan->n_block_all + (plan->classed ? plan->n_tile : 0);
    return LA_OK;
}

// Second host pass: the topic lists, built in a pinned slot of the context's ring and copied to the device.
int stage_topic_lists(la_ctx* ctx, Lane& ln, const BatchPlan& plan, int64_t T, hipStream_t stream, const int32_t** d_lists) {
    *d_lists = nullptr;
    if (plan.n_lists == 0 || (!plan.classed && plan.n_block_all <= 8)) return LA_OK;   // few block topics go inline
    Lane::Stage& sg = ln.stage[ln.stage_next++ & 3u];
    if (sg.done) LA_HIP(ctx, hipEventSynchronize(sg.done));          // the copy that last read this slot
    else LA_HIP(ctx, hipEventCreateWithFlags(&sg.done, hipEventDisableTiming));
    if (sg.cap < (size_t)plan.n_lists) {
        if (sg.p) { LA_HIP(ctx, hipHostFree(sg.p)); sg.p = nullptr; sg.cap = 0; }
        const size_t want = (size_t)plan.n_lists + (size_t)plan.n_lists / 2 + 64;
        LA_HIP(ctx, hipHostMalloc((void**)&sg.p, want * sizeof(int32_t), hipHostMallocDefault));
        sg.cap = want;
    }
    int64_t block_fill[la::kBlockClasses], tile_fill[kTileClasses];
    for (int k = 0; k < la::kBlockClasses; ++k) block_fill[k] = plan.block_at[k];
    for (int k = 0; k < kTileClasses; ++k) tile_fill[k] = plan.tile_at[k];
    for (int64_t t = 0; t < T; ++t) {
        const uint8_t k = plan.code[t];
        if (k < kTileClasses) {
            if (plan.classed) sg.p[tile_fill[plan.merged[k]]++] = (int32_t)t;
        } else if (k < kLargeCode) {
            sg.p[block_fill[k - kTileClasses]++] = (int32_t)t;
        }
    }
    // calls of one context are stream-ordered (lagassign.h), so the device copy of the lists is free again by
    // the time this copy runs
    if (int rc = reserve(ctx, ln.block_list, (size_t)plan.n_lists * sizeof(int32_t))) return rc;
    LA_HIP(ctx, hipMemcpyAsync(ln.block_list.p, sg.p, (size_t)plan.n_lists * sizeof(int32_t), hipMemcpyHostToDevice,
                               stream));
    LA_HIP(ctx, hipEventRecord(sg.done, stream));
    *d_lists = (const int32_t*)ln.block_list.p;
    return LA_OK;
}

int launch_block_topics(la_ctx* ctx, const la_device_batch* b, const BatchPlan& plan, const int32_t* d_lists, uint32_t* status,
                        hipStream_t stream) {
    la::BlockArgs g{};
    g.part_off = b->d_part_off;
    g.cons_off = b->d_cons_off;
    g.pid = b->d_partition_id;
    g.begin = b->d_begin_off;
    g.end = b->d_end_off;
    g.committed = b->d_committed_off;
    g.lag = b->d_lag;
    g.cons_rank = b->d_cons_rank;
    g.out_pid = b->d_out_partition;
    g.out_rank = b->d_out_member_rank;
    g.out_total = b->d_out_total_lag;
    g.status = status;
    g.reset_latest = (b->reset_mode == LA_RESET_LATEST) ? 1 : 0;
    if (!d_lists) {
        // a handful of block topics: their indices travel in the kernel arguments (no copy, no event)
        for (int cls = 0; cls < la::kBlockClasses; ++cls) {
            if (plan.n_block[cls] == 0) continue;
            int n = 0;
            for (int64_t t = 0; t < b->n_topics && n < (int)plan.n_block[cls]; ++t)
                if (plan.code[t] == kTileClasses + cls) g.inline_list[n++] = (int32_t)t;
            g.list = nullptr;
            g.n_list = n;
            LA_HIP(ctx, la::block_launch(g, cls, stream));
        }
        return LA_OK;
    }
    for (int cls = 0; cls < la::kBlockClasses; ++cls) {
        g.list = d_lists + plan.block_at[cls];
        g.n_list = (int32_t)plan.n_block[cls];
        LA_HIP(ctx, la::block_launch(g, cls, stream));
    }
    return LA_OK;
}

int launch_large_topics(la_ctx* ctx, Lane& ln, const la_device_batch* b, const BatchPlan& plan, bool argmin, uint32_t* status,
                        hipStream_t stream) {
    // The per-topic loop of assign(Map,Map) (Main.java:177-184) is independent across topics: all large topics of the batch
    // run SIDE BY SIDE (la::large_topics_launch: every phase one launch over all of them, one greedy workgroup per topic),
    // in groups bounded by scratch memory.  Topics with more consumers than the one-workgroup greedy holds take the
    // bins-in-HBM form, one after another; the literal-argmin test hook stays serial.
    std::vector<la::LargeArgs> group;
    int64_t group_n = 0;
    auto flush = [&]() -> int {
        if (group.empty()) return LA_OK;
        const hipError_t e = la::large_topics_launch(ln.large, group.data(), (int)group.size(), stream);
        group.clear();
        group_n = 0;
        return e != hipSuccess ? hip_fail(ctx, e, "large topics: %s") : LA_OK;
    };
    constexpr int64_t kGroupPartitions = (int64_t)1 << 30;          // ~26 GB of sort buffers
    constexpr size_t kGroupTopics = 8192;
    for (int64_t t = 0; t < b->n_topics; ++t) {
        if (plan.code[t] != kLargeCode) continue;
        const int64_t p = b->h_part_off[t + 1] - b->h_part_off[t], c = b->h_cons_off[t + 1] - b->h_cons_off[t];
        if (p > 0x7FFFFFFF || c > 0x7FFFFFFF)
            return fail(ctx, LA_ESHAPE, "topic %lld has %lld partitions and %lld consumers; at most 2^31-1 of each are supported",
                        (long long)t, (long long)p, (long long)c);
        la::LargeArgs g{};
        g.p0 = b->h_part_off[t];
        g.n_part = p;
        g.c0 = b->h_cons_off[t];
        g.n_cons = c;
        g.pid = b->d_partition_id;
        g.begin = b->d_begin_off;
        g.end = b->d_end_off;
        g.committed = b->d_committed_off;
        g.lag = b->d_lag;
        g.cons_rank = b->d_cons_rank;
        g.out_pid = b->d_out_partition;
        g.out_rank = b->d_out_member_rank;
        g.out_total = b->d_out_total_lag;
        g.reset_latest = (b->reset_mode == LA_RESET_LATEST) ? 1 : 0;
        g.no_sample_sort = (b->flags & LA_FLAG_NO_SAMPLE_SORT) ? 1 : ((b->flags & LA_FLAG_SAMPLE_TIGHT) ? 2 : 0);
        g.sort_multi_kernel = (b->flags & LA_FLAG_SORT_MULTIKERNEL) ? 1 : 0;
        g.no_run_merge = (b->flags & LA_FLAG_NO_RUN_MERGE) ? 1 : 0;
        g.no_moved_sort = (b->flags & LA_FLAG_NO_MOVED_SORT) ? 1 : 0;
        const bool bounded_large = (b->flags & LA_FLAG_BOUNDS) && b->max_lag_hint >= 0 && b->max_partition_id_hint >= 0;
        g.max_lag_hint = bounded_large ? b->max_lag_hint : -1;
        g.max_id_hint = bounded_large ? b->max_partition_id_hint : -1;
        g.status = status;
        hipError_t e = hipSuccess;
        if (c > la::kLargeMaxConsumers) {
            if (int rc = flush()) return rc;
            if (argmin)
                return fail(ctx, LA_ESHAPE, "topic %lld has %lld consumers; LA_ALGO_ARGMIN (a test hook) holds at most %lld",
                            (long long)t, (long long)c, (long long)la::kLargeMaxConsumers);
            e = la::huge_topic_launch(ln.large, g, stream);
        } else if (argmin || p == 0 || (b->flags & LA_FLAG_SERIAL_LARGE)) {
            if (int rc = flush()) return rc;
            e = la::large_topic_launch(ln.large, g, argmin, stream);
        } else {
            if (group.size() >= kGroupTopics || (group_n > 0 && group_n + p > kGroupPartitions))
                if (int rc = flush()) return rc;
            group.push_back(g);
            group_n += p;
        }
        if (e != hipSuccess) return hip_fail(ctx, e, "large topic %lld: %s", (long long)t);
    }
    return flush();
}

}  // namespace

// The dispatcher shared by the host and device entry points (`staged`: what a staged host-buffer call adds, see la_ctx.h).
int enqueue_batch(la_ctx* ctx, Lane& ln, const la_device_batch* b, hipStream_t stream, StagedBatch* staged) {
    uint32_t* const status = staged && staged->status ? staged->status : ln.d_status;
    const la::TileTail* const tail = staged ? staged->tail : nullptr;
    bool* const tail_done = staged ? &staged->tail_done : nullptr;
    if (b->n_topics < 0 || b->n_partitions < 0 || b->n_consumers < 0)
        return fail(ctx, LA_EINVAL, "negative size");
    if (b->n_topics == 0) return LA_OK;
    if (!b->d_part_off || !b->d_cons_off) return fail(ctx, LA_EINVAL, "null offsets");
    // (a batch whose topics have no partitions at all has nothing to write: its [0]-sized outputs may be anything)
    const bool wire_out = (b->flags & LA_FLAG_WIRE_OUT) != 0;
    if (b->n_partitions > 0 && !wire_out && (!b->d_out_partition || !b->d_out_member_rank)) return fail(ctx, LA_EINVAL, "null outputs");
    if (wire_out) {
        // the results in the all-gather's wire format straight from the kernels: the tile path's one-launch form only
        if (!b->d_out_wire || (b->wire_elem_bytes != 2 && b->wire_elem_bytes != 4) ||
            !la::wire_format_valid(b->wire_elem_bytes, b->wire_id_bits))
            return fail(ctx, LA_EINVAL, "LA_FLAG_WIRE_OUT: d_out_wire and a 2- or 4-byte wire format are required");
        if (b->algo != LA_ALGO_AUTO || (b->flags & LA_FLAG_RAGGED) ||
            !la::wave_tile_fits(b->max_partitions_per_topic, b->max_consumers_per_topic) || b->n_partitions >= ((int64_t)1 << 29) ||
            b->n_consumers >= ((int64_t)1 << 30) || (b->flags & LA_FLAG_INDEX64) || !(b->flags & LA_FLAG_BOUNDS) ||
            !la::wave_tile_always_packs(b->max_partitions_per_topic, b->max_consumers_per_topic, b->max_lag_hint,
                                        b->max_partition_id_hint))
            return fail(ctx, LA_EINVAL, "LA_FLAG_WIRE_OUT needs a batch of tile-sized topics (shape hint within 1024 x 64, no LA_FLAG_RAGGED), "
                                        "LA_FLAG_BOUNDS that prove every tile packs, and fewer than 2^29 partitions: run this batch "
                                        "without the flag and pack the results with la_pack_results_on");
    }
    if (b->n_partitions > 0 && (!b->d_partition_id || (!b->d_lag && (!b->d_end_off || !b->d_committed_off))))
        return fail(ctx, LA_EINVAL, "null per-partition input");
    if (b->n_consumers > 0 && !b->d_cons_rank) return fail(ctx, LA_EINVAL, "null cons_rank");
    if (!b->d_lag && b->reset_mode != LA_RESET_LATEST && !b->d_begin_off && b->n_partitions > 0)
        return fail(ctx, LA_EINVAL, "begin_off is required unless reset_mode is LA_RESET_LATEST");
    if (b->algo != LA_ALGO_AUTO && b->algo != LA_ALGO_ROUNDS && b->algo != LA_ALGO_ARGMIN && b->algo != LA_ALGO_ROUNDS_WIDE)
        return fail(ctx, LA_EINVAL, "unknown algo %d", b->algo);

    la::TileArgs a{};
    a.n_topics = b->n_topics;
    a.part_off = b->d_part_off;
    a.pid = b->d_partition_id;
    a.begin = b->d_begin_off;
    a.end = b->d_end_off;
    a.committed = b->d_committed_off;
    a.lag = b->d_lag;
    a.cons_off = b->d_cons_off;
    a.cons_rank = b->d_cons_rank;
    a.out_pid = b->d_out_partition;
    a.out_rank = b->d_out_member_rank;
    a.out_total = b->d_out_total_lag;
    a.status = status;
    a.reset_latest = (b->reset_mode == LA_RESET_LATEST) ? 1 : 0;
    a.n_total = b->n_partitions;
    a.flags = b->flags & (LA_FLAG_INDEX64 | LA_FLAG_DEFER_WIDE);
    if (getenv("LA_TILE_ALWAYS_STAGE2")) a.flags |= la::kTileAlwaysStage2;       // (A/B hook, read at every call)
    a.begin_sparse_max = -1;                                                     // the launcher's choice (launch_one)
    if (const char* env = getenv("LA_TILE_BEGIN_SPARSE_MAX")) a.begin_sparse_max = atoi(env) < 0 ? 0 : atoi(env);   // (A/B hook, read at every call)
    if (wire_out) {
        a.flags |= la::kTileWireOut;
        a.out_wire = b->d_out_wire;
        a.wire_bytes = b->wire_elem_bytes;
        a.wire_id_bits = b->wire_id_bits;
    }
    a.topic_list = nullptr;
    a.k_total = b->n_consumers;
    if (int rc = reserve(ctx, ln.defer, la::wave_tile_defer_bytes(b->n_topics))) return rc;
    a.defer_list = (int32_t*)ln.defer.p;
    const bool argmin = (b->algo == LA_ALGO_ARGMIN);
    const int tile_mode = argmin ? 2 : (b->algo == LA_ALGO_ROUNDS_WIDE ? 1 : 0);

    // The counter pair alternates per LA_ALGO_AUTO launch: such a launch counts into one and its wide
    // kernel zeroes the other (idle by stream order), so no memset node sits between launches.
    // Under stream capture the arguments are frozen into the graph, so the alternation cannot work on replay: a
    // captured launch counts into a third word that a memset node clears first (its wide kernel "resets" a dummy).
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (tile_mode == 0) LA_HIP(ctx, hipStreamIsCapturing(stream, &capture));
    hipError_t counter_err = hipSuccess;
    // LA_FLAG_BOUNDS: when the caller's bounds prove that every tile of a launch packs, that launch defers nothing, needs no
    // wide kernel behind it and leaves the counter pair alone (it neither counts nor has a wide kernel to zero the idle one)
    const bool bounded = tile_mode == 0 && (b->flags & LA_FLAG_BOUNDS) && b->max_lag_hint >= 0 && b->max_partition_id_hint >= 0;
    auto proven = [&](int64_t mp, int64_t mc) {
        return bounded && la::wave_tile_always_packs(mp, mc, b->max_lag_hint, b->max_partition_id_hint);
    };
    auto next_counters = [&](la::TileArgs& t) {
        int32_t* pair = (int32_t*)(ln.d_status + 16);
        if (t.flags & la::kTileNoDefer) {
            t.defer_count = pair + (ln.launches & 1u);
            t.defer_count_next = pair + ((ln.launches + 1u) & 1u);
            return;
        }
        if (capture != hipStreamCaptureStatusNone) {
            t.defer_count = pair + 2;
            t.defer_count_next = pair + 3;
            const hipError_t e = hipMemsetAsync(pair + 2, 0, sizeof(int32_t), stream);
            if (e != hipSuccess) counter_err = e;
            return;
        }
        t.defer_count = pair + (ln.launches & 1u);
        t.defer_count_next = pair + ((ln.launches + 1u) & 1u);
        if (tile_mode == 0) ++ln.launches;
    };
    if (b->n_partitions == 0) {
        // nothing to assign; consumers of partition-less topics still report a total of 0
        if (b->d_out_total_lag && b->n_consumers > 0)
            LA_HIP(ctx, hipMemsetAsync(b->d_out_total_lag, 0, (size_t)b->n_consumers * sizeof(int64_t), stream));
        return LA_OK;
    }
    ln.large.prof.armed = (b->flags & LA_FLAG_PROFILE) != 0;
    if (ln.large.prof.armed) ln.large.prof.recorded = false;
    const bool have_host = b->h_part_off && b->h_cons_off;
    const bool fits_hint = la::wave_tile_fits(b->max_partitions_per_topic, b->max_consumers_per_topic);
    if (fits_hint && !(have_host && (b->flags & LA_FLAG_RAGGED) && tile_mode == 0)) {
        // the plain case: every topic fits a wave tile, one shape for all, nothing read on the host
        if (proven(b->max_partitions_per_topic, b->max_consumers_per_topic)) a.flags |= la::kTileNoDefer;
        next_counters(a);
        LA_HIP(ctx, counter_err);
        if (tail && tile_mode == 0) a.tail = *tail;                       // the batch is this one launch
        LA_HIP(ctx, la::wave_tile_launch(a, b->max_partitions_per_topic, b->max_consumers_per_topic, tile_mode, stream,
                                         tail_done));
        return LA_OK;
    }
    la_device_batch with_host;
    if (!have_host) {
        // The shape hint exceeds one wave tile and the caller kept no host copy of the offsets: fetch them (two
        // small copies and a wait on `stream` -- this call is then neither asynchronous nor capturable).
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        LA_HIP(ctx, hipStreamIsCapturing(stream, &cap));
        if (cap != hipStreamCaptureStatusNone)
            return fail(ctx, LA_EINVAL, "shape hint exceeds one wave tile: h_part_off and h_cons_off are required "
                                        "while the stream is being captured");
        const size_t words = (size_t)b->n_topics + 1;
        ln.host_offsets.resize(2 * words);
        LA_HIP(ctx, hipMemcpyAsync(ln.host_offsets.data(), b->d_part_off, words * 8, hipMemcpyDeviceToHost, stream));
        LA_HIP(ctx, hipMemcpyAsync(ln.host_offsets.data() + words, b->d_cons_off, words * 8, hipMemcpyDeviceToHost, stream));
        LA_HIP(ctx, hipStreamSynchronize(stream));
        with_host = *b;
        with_host.h_part_off = ln.host_offsets.data();
        with_host.h_cons_off = ln.host_offsets.data() + words;
        b = &with_host;
    }

    // mixed or ragged shapes (see the dispatcher notes above)
    const bool use_block = !argmin && b->algo != LA_ALGO_ROUNDS_WIDE;   // the test-hook algos keep to tile + large
    BatchPlan plan;
    if (int rc = plan_batch(ctx, ln, b, tile_mode, use_block, &plan)) return rc;
    const int32_t* d_lists = nullptr;
    if (int rc = stage_topic_lists(ctx, ln, plan, b->n_topics, stream, &d_lists)) return rc;
    if (plan.classed) {
        for (int k = 0; k < kTileClasses; ++k) {
            if (plan.tile[k].n == 0) continue;
            la::TileArgs run = a;
            run.n_topics = plan.tile[k].n;
            run.topic_list = d_lists + plan.tile_at[k];
            if (proven(plan.tile[k].mp, plan.tile[k].mc)) run.flags |= la::kTileNoDefer;
            next_counters(run);
            LA_HIP(ctx, counter_err);
            LA_HIP(ctx, la::wave_tile_launch(run, plan.tile[k].mp, plan.tile[k].mc, tile_mode, stream));
        }
    } else if (plan.n_tile > 0) {
        la::TileArgs run = a;
        run.flags |= la::kTileSkipOversize;
        if (proven(plan.tile_mp, plan.tile_mc)) run.flags |= la::kTileNoDefer;
        next_counters(run);
        LA_HIP(ctx, counter_err);
        // (a tail only when nothing else of the batch runs behind this launch)
        if (tail && tile_mode == 0 && plan.n_block_all == 0 && plan.n_large == 0) run.tail = *tail;
        LA_HIP(ctx, la::wave_tile_launch(run, plan.tile_mp, plan.tile_mc, tile_mode, stream, tail_done));
    }
    if (plan.n_block_all > 0)
        if (int rc = launch_block_topics(ctx, b, plan, d_lists, status, stream)) return rc;
    if (plan.n_large > 0)
        if (int rc = launch_large_topics(ctx, ln, b, plan, argmin, status, stream)) return rc;
    return LA_OK;
}

// ---- C ABI --------------------------------------------------------------------------------------
LA_API int la_version(void) { return LA_VERSION; }

LA_API const char* la_last_error(const la_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

LA_API int la_device_count(void) {
    int count = 0;
    const hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess) return fail(nullptr, LA_ENODEV, "no HIP device (%s)", hipGetErrorString(e));
    return count;
}

LA_API int la_create_multi(la_ctx** out, int n_devices, const int* device_ids, unsigned flags) {
    DeviceGuard restore_device;
    if (!out) return fail(nullptr, LA_EINVAL, "out is NULL");
    *out = nullptr;
    try {
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count <= 0)
            return fail(nullptr, LA_ENODEV, "no HIP device (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        std::vector<int> ids;
        if (n_devices < 0) return fail(nullptr, LA_EINVAL, "n_devices < 0");
        if (n_devices == 0 || !device_ids) {
            if (n_devices != 0) return fail(nullptr, LA_EINVAL, "device_ids is NULL");
            for (int d = 0; d < count; ++d) ids.push_back(d);          // every device of the node
        } else {
            ids.assign(device_ids, device_ids + n_devices);
        }
        if ((int)ids.size() > kMaxShards) return fail(nullptr, LA_EINVAL, "at most %d shards", kMaxShards);
        for (int d : ids) {
            if (d < 0 || d >= count) return fail(nullptr, LA_ENODEV, "device %d of %d", d, count);
            hipDeviceProp_t prop;
            if ((e = hipGetDeviceProperties(&prop, d)) != hipSuccess)
                return fail(nullptr, LA_EHIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
            if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
                return fail(nullptr, LA_ENODEV, "device %d is %s; this library is built for gfx950 only", d,
                            prop.gcnArchName);
        }
        int lanes = (int)(flags & LA_CREATE_LANES_MASK);
        if (const char* env = getenv("LA_LANES")) lanes = atoi(env);
        if (lanes <= 0) lanes = ids.size() <= 2 ? 3 : 2;
        if (lanes > 8) lanes = 8;
        la_ctx* ctx = new (std::nothrow) la_ctx();
        if (!ctx) return fail(nullptr, LA_ENOMEM, "out of host memory");
        ctx->split_always = (flags & LA_CREATE_SPLIT_ALWAYS) != 0;
        if (const char* env = getenv("LA_CHUNK_PARTITIONS")) ctx->chunk_partitions = atoll(env);
        host_defaults(ctx);
        ctx->shards.resize(ids.size());
        for (size_t i = 0; i < ids.size(); ++i) {
            Shard& sh = ctx->shards[i];
            sh.device = ids[i];
            sh.lanes.resize((size_t)lanes);
            int rc = LA_OK;
            if ((e = hipSetDevice(sh.device)) != hipSuccess ||
                (e = hipEventCreateWithFlags(&sh.ready, hipEventDisableTiming)) != hipSuccess)
                rc = fail(nullptr, LA_EHIP, "context setup: %s", hipGetErrorString(e));
            if (rc == LA_OK && (e = la::large_init_device()) != hipSuccess)
                rc = fail(nullptr, LA_EHIP, "context setup (device check): %s", hipGetErrorString(e));
            for (Lane& ln : sh.lanes)
                if (rc == LA_OK) rc = create_lane(ln);
            if (rc != LA_OK) {
                la_destroy(ctx);
                return rc;
            }
        }
        *out = ctx;
        return LA_OK;
    } catch (...) {
        return fail(nullptr, LA_ENOMEM, "exception in la_create_multi");
    }
}

LA_API int la_create(la_ctx** out, int device_id, unsigned flags) { return la_create_multi(out, 1, &device_id, flags); }

LA_API void la_destroy(la_ctx* ctx) {
    DeviceGuard restore_device;
    if (!ctx) return;
    if (!ctx->comms.empty()) {
        for (Shard& sh : ctx->shards) {                                   // nothing of an all-gather stays in flight
            (void)hipSetDevice(sh.device);
            if (!sh.lanes.empty() && sh.lanes[0].stream) (void)hipStreamSynchronize(sh.lanes[0].stream);
        }
        RcclApi& r = rccl_api();
        for (void* c : ctx->comms)
            if (c && r.CommDestroy) (void)r.CommDestroy(c);
        ctx->comms.clear();
    }
    for (Shard& sh : ctx->shards) {
        (void)hipSetDevice(sh.device);
        for (Lane& ln : sh.lanes) destroy_lane(ln);
        for (DevBuf* b : {&sh.part_off, &sh.pid, &sh.begin, &sh.end, &sh.committed, &sh.cons_off, &sh.cons_rank,
                          &sh.out_pid, &sh.out_rank, &sh.out_total, &sh.small_d, &sh.small_g, &sh.none_idx, &sh.none_val})
            release(*b);
        for (HostBuf* h : {&sh.g_off, &sh.g_topic, &sh.g_part, &sh.small_h, &sh.small_gh, &sh.zc_h})
            if (h->p) (void)hipHostFree(h->p);
        la::moves_scratch_release(sh.moves);
        la::verify_scratch_release(sh.verify);
        la::sticky_scratch_release(sh.sticky);
        la::coop_scratch_release(sh.coop);
        la::pinned_large_scratch_release(sh.pinned_large);
        if (sh.ready) (void)hipEventDestroy(sh.ready);
        for (hipEvent_t e : sh.chunk_ev) (void)hipEventDestroy(e);
        for (hipStream_t st : sh.copy_in)
            if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        if (sh.copy_out) { (void)hipStreamSynchronize(sh.copy_out); (void)hipStreamDestroy(sh.copy_out); }
    }
    delete ctx;
}

LA_API int la_shard_count(const la_ctx* ctx) { return ctx ? (int)ctx->shards.size() : LA_EINVAL; }

LA_API int la_shard_device(const la_ctx* ctx, int shard) {
    if (!ctx || shard < 0 || shard >= (int)ctx->shards.size()) return LA_EINVAL;
    return ctx->shards[(size_t)shard].device;
}

LA_API int la_device_features(const la_ctx* ctx, int shard) {
    DeviceGuard restore_device;
    if (!ctx || shard < 0 || shard >= (int)ctx->shards.size()) return LA_EINVAL;
    if (hipSetDevice(ctx->shards[(size_t)shard].device) != hipSuccess) return LA_EHIP;
    return la::large_atomic_rank_supported() ? LA_FEATURE_ATOMIC_RANK : 0;
}

LA_API int la_plan_shards(int32_t n_topics, const int64_t* part_off, int32_t n_shards, int32_t* bounds) {
    if (n_topics < 0 || n_shards < 1 || !part_off || !bounds) return LA_EINVAL;
    for (int32_t t = 0; t < n_topics; ++t)
        if (part_off[t + 1] < part_off[t]) return LA_EINVAL;
    try {
        std::vector<int32_t> tmp((size_t)n_shards + 1);
        plan_ranges(part_off, 0, n_topics, n_shards, tmp.data());
        memcpy(bounds, tmp.data(), tmp.size() * sizeof(int32_t));
        return LA_OK;
    } catch (...) {
        return LA_ENOMEM;
    }
}

LA_API int la_last_shard_bounds(const la_ctx* ctx, int32_t* bounds, int32_t capacity) {
    if (!ctx) return LA_EINVAL;
    const int S = ctx->last_shards;
    if (bounds)
        for (int i = 0; i <= S && i < capacity; ++i) bounds[i] = ctx->last_bounds[i];
    return S;
}

// One ncclAllGather per shard inside one group, `bytes` bytes each (ncclUint8: an all-gather does no arithmetic, the type only
// sizes the elements), on the shards' own streams.
static int allgather_bytes(la_ctx* ctx, size_t bytes, const void* const* d_send, void* const* d_recv) {
    const int S = (int)ctx->shards.size();
    if (!d_send || !d_recv) return fail(ctx, LA_EINVAL, "null buffer list");
    for (int i = 0; i < S; ++i)
        if (bytes > 0 && (!d_send[i] || !d_recv[i])) return fail(ctx, LA_EINVAL, "null buffer of shard %d", i);
    for (int i = 0; i < S; ++i)
        for (int j = 0; j < i; ++j)
            if (ctx->shards[(size_t)i].device == ctx->shards[(size_t)j].device)
                return fail(ctx, LA_EINVAL, "shards %d and %d share device %d: RCCL needs one distinct device per rank", j, i,
                            ctx->shards[(size_t)i].device);
    if (bytes == 0) return LA_OK;
    RcclApi& r = rccl_api();
    if (!r.handle) return fail(ctx, LA_ENODEV, "%s", r.why.c_str());
    auto text = [&](int rc) { return r.GetErrorString ? r.GetErrorString(rc) : "rccl error"; };
    if (ctx->comms.empty()) {
        std::vector<int> devs;
        for (const Shard& sh : ctx->shards) devs.push_back(sh.device);
        std::vector<void*> comms((size_t)S, nullptr);
        const int rc = r.CommInitAll(comms.data(), S, devs.data());
        if (rc != 0) return fail(ctx, LA_EHIP, "ncclCommInitAll over %d device(s): %s", S, text(rc));
        ctx->comms = comms;
    }
    int rc = r.GroupStart();
    if (rc != 0) return fail(ctx, LA_EHIP, "ncclGroupStart: %s", text(rc));
    int first_bad = 0;
    for (int i = 0; i < S; ++i) {
        Shard& sh = ctx->shards[(size_t)i];
        if (hipSetDevice(sh.device) != hipSuccess) { first_bad = -1; break; }
        rc = r.AllGather(d_send[i], d_recv[i], bytes, /* ncclUint8 */ 1, ctx->comms[(size_t)i], sh.lanes[0].stream);
        if (rc != 0 && first_bad == 0) first_bad = rc;
    }
    rc = r.GroupEnd();
    if (first_bad == -1) return fail(ctx, LA_EHIP, "hipSetDevice failed while enqueueing the all-gather");
    if (first_bad != 0) return fail(ctx, LA_EHIP, "ncclAllGather: %s", text(first_bad));
    if (rc != 0) return fail(ctx, LA_EHIP, "ncclGroupEnd: %s", text(rc));
    return LA_OK;
}

LA_API int la_allgather_results(la_ctx* ctx, int64_t count, const int32_t* const* d_send, int32_t* const* d_recv) {
    DeviceGuard restore_device;
    if (!ctx) return LA_EINVAL;
    try {
        if (count < 0) return fail(ctx, LA_EINVAL, "negative count");
        return allgather_bytes(ctx, (size_t)count * 4, (const void* const*)d_send, (void* const*)d_recv);
    } catch (...) {
        return fail(ctx, LA_ENOMEM, "exception in la_allgather_results");
    }
}

LA_API int la_allgather_packed(la_ctx* ctx, int64_t count, int32_t elem_bytes, const void* const* d_send, void* const* d_recv) {
    DeviceGuard restore_device;
    if (!ctx) return LA_EINVAL;
    try {
        if (count < 0) return fail(ctx, LA_EINVAL, "negative count");
        if (elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) return fail(ctx, LA_EINVAL, "elem_bytes must be 2, 4 or 8");
        return allgather_bytes(ctx, (size_t)count * (size_t)elem_bytes, d_send, d_recv);
    } catch (...) {
        return fail(ctx, LA_ENOMEM, "exception in la_allgather_packed");
    }
}

LA_API int la_wire_format_for(int64_t max_partition_id, int64_t n_members, la_wire_format* out) {
    if (!out) return LA_EINVAL;
    int eb = 8, ib = 32;
    la::wire_format_for(max_partition_id, n_members, &eb, &ib);
    out->elem_bytes = eb;
    out->id_bits = ib;
    return LA_OK;
}

LA_API int la_pack_results_on(la_ctx* ctx, int shard, int64_t n, const int32_t* d_out_partition, const int32_t* d_out_member_rank,
                              const la_wire_format* fmt, void* d_packed, void* stream) {
    return shard_entry<false>(ctx, shard, "exception in la_pack_results_on", [&](Shard& sh) -> int {
        if (n < 0) return fail(ctx, LA_EINVAL, "negative size");
        if (!fmt || !la::wire_format_valid(fmt->elem_bytes, fmt->id_bits)) return fail(ctx, LA_EINVAL, "bad wire format");
        if (n > 0 && (!d_out_partition || !d_out_member_rank || !d_packed)) return fail(ctx, LA_EINVAL, "null buffer");
        LA_HIP(ctx, la::wire_pack_launch(n, d_out_partition, d_out_member_rank, fmt->elem_bytes, fmt->id_bits, d_packed,
                                         sh.lanes[0].d_status, (hipStream_t)stream));
        return LA_OK;
    });
}

LA_API int la_unpack_results_on(la_ctx* ctx, int shard, int64_t n, const void* d_packed, const la_wire_format* fmt,
                                int32_t* d_out_partition, int32_t* d_out_member_rank, void* stream) {
    return shard_entry<false>(ctx, shard, "exception in la_unpack_results_on", [&](Shard& sh) -> int {
        if (n < 0) return fail(ctx, LA_EINVAL, "negative size");
        if (!fmt || !la::wire_format_valid(fmt->elem_bytes, fmt->id_bits)) return fail(ctx, LA_EINVAL, "bad wire format");
        if (n > 0 && (!d_out_partition || !d_out_member_rank || !d_packed)) return fail(ctx, LA_EINVAL, "null buffer");
        LA_HIP(ctx, la::wire_unpack_launch(n, d_packed, fmt->elem_bytes, fmt->id_bits, d_out_partition, d_out_member_rank,
                                           (hipStream_t)stream));
        return LA_OK;
    });
}

LA_API int la_last_pipeline(const la_ctx* ctx) { return ctx ? ctx->last_pipeline : LA_EINVAL; }

LA_API int64_t la_last_launches(const la_ctx* ctx) { return ctx ? ctx->last_launches : (int64_t)LA_EINVAL; }

LA_API int la_hint_next_call(la_ctx* ctx, const la_call_hints* hints) {
    if (!ctx) return LA_EINVAL;
    ctx->hints_set = false;
    if (!hints) return LA_OK;
    // the struct may grow: take what the caller's header knows of it (the four fields of ABI 0.4.0 at least)
    if (hints->struct_size < (int32_t)sizeof(la_call_hints))
        return fail(ctx, LA_EINVAL, "la_call_hints.struct_size %d is smaller than the %zu bytes of ABI 0.4.0", hints->struct_size,
                    sizeof(la_call_hints));
    if ((hints->flags & LA_HINT_BOUNDS) && (hints->max_lag < 0 || hints->max_partition_id < 0))
        return fail(ctx, LA_EINVAL, "LA_HINT_BOUNDS: max_lag and max_partition_id must be >= 0");
    ctx->hints = *hints;
    ctx->hints_set = true;
    return LA_OK;
}

LA_API void* la_host_alloc(la_ctx* ctx, size_t bytes) {
    DeviceGuard restore_device;
    if (!ctx || ctx->shards.empty()) return nullptr;
    void* p = nullptr;
    if (hipSetDevice(ctx->shards[0].device) != hipSuccess) return nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable);
    if (e != hipSuccess) {
        (void)fail(ctx, LA_ENOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
        return nullptr;
    }
    return p;
}

LA_API void la_host_free(la_ctx* ctx, void* p) {
    (void)ctx;
    if (p) (void)hipHostFree(p);
}

LA_API int la_compute_lag(la_ctx* ctx, int64_t n, const int64_t* begin_off, const int64_t* end_off,
                          const int64_t* committed_off, int32_t reset_mode, int64_t* out_lag) {
    DeviceGuard restore_device;
    LaunchSpan span(ctx);
    if (!ctx) return LA_EINVAL;
    try {
        if (n < 0) return fail(ctx, LA_EINVAL, "n < 0");
        if (n == 0) return LA_OK;
        if (!end_off || !committed_off || !out_lag) return fail(ctx, LA_EINVAL, "null buffer");
        const bool latest = reset_mode == LA_RESET_LATEST;
        if (!latest && !begin_off) return fail(ctx, LA_EINVAL, "begin_off is required unless reset_mode is LA_RESET_LATEST");
        ctx->last_valid = false;                       // reuses the scratch the last results live in
        // elementwise and PCIe-bound: contiguous element ranges over the shards (every device has its own link), each on
        // its shard's first lane
        int S = (int)ctx->shards.size();
        if (!ctx->split_always) {
            const int64_t by_size = n / (4 * kMinShardPartitions);
            if (by_size < S) S = by_size < 1 ? 1 : (int)by_size;
        }
        if ((int64_t)S > n) S = (int)n;
        auto run_range = [&](int i) -> int {
            Shard& sh = ctx->shards[(size_t)i];
            const int64_t e0 = n / S * i + (n % S) * i / S, e1 = n / S * (i + 1) + (n % S) * (i + 1) / S;
            const int64_t m = e1 - e0;
            if (m <= 0) return LA_OK;
            LA_HIP(ctx, hipSetDevice(sh.device));
            const size_t nb = (size_t)m * 8;
            int rc;
            if ((rc = reserve(ctx, sh.end, nb)) || (rc = reserve(ctx, sh.committed, nb)) ||
                (rc = reserve(ctx, sh.begin, latest ? 16 : nb)) || (rc = reserve(ctx, sh.out_total, nb)))
                return rc;
            hipStream_t st = sh.lanes[0].stream;
            LA_HIP(ctx, hipMemcpyAsync(sh.end.p, end_off + e0, nb, hipMemcpyHostToDevice, st));
            LA_HIP(ctx, hipMemcpyAsync(sh.committed.p, committed_off + e0, nb, hipMemcpyHostToDevice, st));
            if (!latest) LA_HIP(ctx, hipMemcpyAsync(sh.begin.p, begin_off + e0, nb, hipMemcpyHostToDevice, st));
            LA_HIP(ctx, la::lag_launch(m, latest ? nullptr : (const int64_t*)sh.begin.p, (const int64_t*)sh.end.p,
                                       (const int64_t*)sh.committed.p, latest, (int64_t*)sh.out_total.p, st));
            LA_HIP(ctx, hipMemcpyAsync(out_lag + e0, sh.out_total.p, nb, hipMemcpyDeviceToHost, st));
            LA_HIP(ctx, hipStreamSynchronize(st));
            return LA_OK;
        };
        if (S == 1) return run_range(0);
        return run_workers(ctx, S, run_range);
    } catch (...) {
        return fail(ctx, LA_ENOMEM, "exception in la_compute_lag");
    }
}

LA_API int la_assign_batch(la_ctx* ctx, int32_t n_topics, const int64_t* part_off, const int32_t* partition_id,
                           const int64_t* begin_off, const int64_t* end_off, const int64_t* committed_off,
                           int32_t reset_mode, const int64_t* cons_off, const int32_t* cons_rank,
                           int32_t* out_partition, int32_t* out_member_rank, int64_t* out_total_lag) {
    DeviceGuard restore_device;
    LaunchSpan span(ctx);
    HintSpender spend_hints(ctx);
    try {
        HostCall c;
        c.T = n_topics; c.part_off = part_off; c.pid = partition_id; c.begin = begin_off; c.end = end_off; c.committed = committed_off;
        c.reset_mode = reset_mode; c.cons_off = cons_off; c.cons_rank = cons_rank;
        c.out_pid = out_partition; c.out_rank = out_member_rank; c.out_total = out_total_lag;
        return assign_host(ctx, c);
    } catch (...) {
        return ctx ? fail(ctx, LA_ENOMEM, "exception in la_assign_batch") : LA_EINVAL;
    }
}

LA_API int la_assign_batch_lags(la_ctx* ctx, int32_t n_topics, const int64_t* part_off, const int32_t* partition_id,
                                const int64_t* lag, const int64_t* cons_off, const int32_t* cons_rank,
                                int32_t* out_partition, int32_t* out_member_rank, int64_t* out_total_lag) {
    DeviceGuard restore_device;
    LaunchSpan span(ctx);
    HintSpender spend_hints(ctx);
    try {
        if (ctx && !lag && n_topics > 0 && part_off && part_off[n_topics] > 0)
            return fail(ctx, LA_EINVAL, "lag is NULL");
        static const int64_t dummy = 0;
        HostCall c;
        c.T = n_topics; c.part_off = part_off; c.pid = partition_id;
        c.reset_mode = LA_RESET_LATEST; c.cons_off = cons_off; c.cons_rank = cons_rank;
        c.out_pid = out_partition; c.out_rank = out_member_rank; c.out_total = out_total_lag;
        c.lag = lag ? lag : &dummy;
        return assign_host(ctx, c);
    } catch (...) {
        return ctx ? fail(ctx, LA_ENOMEM, "exception in la_assign_batch_lags") : LA_EINVAL;
    }
}

LA_API int la_assign_batch_device_on(la_ctx* ctx, int shard, const la_device_batch* batch, void* stream) {
    return shard_entry<true>(ctx, shard, "exception in la_assign_batch_device", [&](Shard& sh) -> int {
        if (!batch) return fail(ctx, LA_EINVAL, "batch is NULL");
        return enqueue_batch(ctx, sh.lanes[0], batch, (hipStream_t)stream);
    });
}

LA_API int la_assign_batch_device(la_ctx* ctx, const la_device_batch* batch, void* stream) {
    return la_assign_batch_device_on(ctx, 0, batch, stream);
}

LA_API void* la_shard_stream(la_ctx* ctx, int shard) {
    if (!ctx || shard < 0 || shard >= (int)ctx->shards.size()) return nullptr;
    return (void*)ctx->shards[(size_t)shard].lanes[0].stream;
}

LA_API void* la_stream(la_ctx* ctx) { return la_shard_stream(ctx, 0); }

LA_API int la_group_by_member_device(la_ctx* ctx, int32_t n_topics, int64_t n_partitions, const int64_t* d_part_off,
                                     const int32_t* d_out_partition, const int32_t* d_out_member_rank,
                                     int32_t n_members, int64_t* d_member_off, int32_t* d_grouped_topic,
                                     int32_t* d_grouped_partition, void* stream) {
    return la_group_by_member_device_on(ctx, 0, n_topics, n_partitions, d_part_off, d_out_partition, d_out_member_rank,
                                        n_members, d_member_off, d_grouped_topic, d_grouped_partition, stream);
}

LA_API int la_group_by_member_device_on(la_ctx* ctx, int shard, int32_t n_topics, int64_t n_partitions,
                                        const int64_t* d_part_off, const int32_t* d_out_partition,
                                        const int32_t* d_out_member_rank, int32_t n_members, int64_t* d_member_off,
                                        int32_t* d_grouped_topic, int32_t* d_grouped_partition, void* stream) {
    return shard_entry<false>(ctx, shard, "exception in la_group_by_member_device", [&](Shard& sh) -> int {
        if (n_topics < 0 || n_partitions < 0 || n_members < 0) return fail(ctx, LA_EINVAL, "negative size");
        if (!d_member_off) return fail(ctx, LA_EINVAL, "member_off is NULL");
        if (n_partitions > 0 && (!d_out_partition || !d_out_member_rank || !d_grouped_partition ||
                                 (d_grouped_topic && !d_part_off)))
            return fail(ctx, LA_EINVAL, "null buffer");
        if (n_partitions > 0x7FFFFFFF) return fail(ctx, LA_ESHAPE, "at most 2^31-1 entries are supported");
        hipError_t e = la::group_by_member_launch(sh.lanes[0].large, n_partitions, n_members, n_topics, d_part_off,
                                                  d_out_partition, d_out_member_rank, d_member_off,
                                                  d_grouped_topic, d_grouped_partition, nullptr, sh.lanes[0].d_status,
                                                  (hipStream_t)stream);
        return e != hipSuccess ? hip_fail(ctx, e, "group_by_member: %s") : LA_OK;
    });
}

// Per-member roll-up of an assignment (la_loads.hip).  Owns no scratch: the bins are LDS and the caller's outputs, so the
// results kept for la_group_last_by_member stay as they are.
LA_API int la_member_loads_device(la_ctx* ctx, int64_t n_partitions, const int32_t* d_out_member_rank, int64_t n_consumers,
                                  const int32_t* d_cons_rank, const int64_t* d_out_total_lag, int32_t n_members,
                                  int64_t* d_member_partitions, int64_t* d_member_lag, int64_t* d_unassigned, void* stream) {
    return la_member_loads_device_on(ctx, 0, n_partitions, d_out_member_rank, n_consumers, d_cons_rank, d_out_total_lag,
                                     n_members, d_member_partitions, d_member_lag, d_unassigned, stream);
}

LA_API int la_member_loads_device_on(la_ctx* ctx, int shard, int64_t n_partitions, const int32_t* d_out_member_rank,
                                     int64_t n_consumers, const int32_t* d_cons_rank, const int64_t* d_out_total_lag,
                                     int32_t n_members, int64_t* d_member_partitions, int64_t* d_member_lag,
                                     int64_t* d_unassigned, void* stream) {
    return shard_entry<true>(ctx, shard, "exception in la_member_loads_device", [&](Shard& sh) -> int {
        if (n_partitions < 0 || n_consumers < 0 || n_members < 0) return fail(ctx, LA_EINVAL, "negative size");
        if (!d_out_member_rank && !d_cons_rank) return fail(ctx, LA_EINVAL, "d_out_member_rank and d_cons_rank are both NULL");
        if (!d_out_member_rank && (d_member_partitions || d_unassigned))
            return fail(ctx, LA_EINVAL, "d_member_partitions / d_unassigned given without d_out_member_rank");
        if (!d_cons_rank && (d_out_total_lag || d_member_lag))
            return fail(ctx, LA_EINVAL, "d_out_total_lag / d_member_lag given without d_cons_rank");
        if (d_out_member_rank && !d_member_partitions && n_members > 0) return fail(ctx, LA_EINVAL, "d_member_partitions is NULL");
        if (d_cons_rank && ((!d_member_lag && n_members > 0) || (!d_out_total_lag && n_consumers > 0)))
            return fail(ctx, LA_EINVAL, "d_member_lag or d_out_total_lag is NULL");
        hipError_t e = la::member_loads_launch(n_partitions, d_out_member_rank, n_consumers, d_cons_rank, d_out_total_lag,
                                               n_members, d_member_partitions, d_member_lag, d_unassigned,
                                               sh.lanes[0].d_status, (hipStream_t)stream);
        if (e != hipSuccess) return fail(ctx, LA_EHIP, "member_loads: %s", hipGetErrorString(e));
        return LA_OK;
    });
}

constexpr int kMovesArgsSizeOneLayout = 128;      // la_moves_args up to d_moved: what the struct was before the two-layout fields
static_assert(offsetof(la_moves_args, n_prev_topics) == kMovesArgsSizeOneLayout, "the two-layout fields follow the one-layout struct");
static_assert(LA_MOVES_NO_PREVIOUS == la::kMovesNoPrevious, "lagassign.h and la_kernels.h");

// the fields both forms of la_assignment_moves_device share
static la::MovesCall moves_call_of(const la_moves_args& g) {
    la::MovesCall c{};
    c.n_topics = g.n_topics;
    c.n_members = g.n_members;
    c.n_prev_members = g.d_prev_rank_map ? g.n_prev_members : g.n_members;
    c.n_partitions = g.n_partitions;
    c.max_partitions_per_topic = g.max_partitions_per_topic;
    c.part_off = g.d_part_off;
    c.out_partition = g.d_out_partition;
    c.out_member_rank = g.d_out_member_rank;
    c.prev_partition = g.d_prev_partition;
    c.prev_member_rank = g.d_prev_member_rank;
    c.map = g.d_prev_rank_map;
    c.prev_owner = g.d_prev_owner;
    c.topic_moved = g.d_topic_moved;
    c.member_gained = g.d_member_gained;
    c.member_lost = g.d_member_lost;
    c.moved = g.d_moved;
    return c;
}

// host copy of an offset array: from 0 to `total`, never descending
static bool offsets_ascend(const int64_t* off, int64_t n, int64_t total) {
    if (off[0] != 0 || off[n] != total) return false;
    for (int64_t t = 0; t < n; ++t)
        if (off[t + 1] < off[t]) return false;
    return true;
}

// la_assignment_moves_device with d_prev_part_off: a layout each (la_moves_layouts.hip); sizes, members and "some output" checked
static int moves_layouts(la_ctx* ctx, Shard& sh, const la_moves_args& g, hipStream_t stream) {
    const int64_t T = g.n_topics, N = g.n_partitions, NP = g.n_prev_partitions;
    if (g.n_prev_topics < 0 || NP < 0) return fail(ctx, LA_EINVAL, "negative size");
    if (g.reserved != 0) return fail(ctx, LA_EINVAL, "la_moves_args.reserved must be 0");
    if (!g.d_prev_topic && g.n_prev_topics != T) return fail(ctx, LA_EINVAL, "without d_prev_topic both layouts hold the same topics: n_prev_topics must equal n_topics");
    if ((T == 0 && N != 0) || (g.n_prev_topics == 0 && NP != 0)) return fail(ctx, LA_EINVAL, "partitions without topics");
    const bool work = T > 0 && (N > 0 || NP > 0);
    if ((work && !g.d_part_off) || (N > 0 && (!g.d_out_partition || !g.d_out_member_rank)) ||
        (NP > 0 && (!g.d_prev_partition || !g.d_prev_member_rank)))
        return fail(ctx, LA_EINVAL, "null buffer");
    const int32_t* h_prev_topic = g.d_prev_topic ? g.h_prev_topic : nullptr;      // it is the host copy of d_prev_topic, or nothing
    if (g.max_partitions_per_topic > la::kMovesLdsMaxPartitions && work) {
        // pairs beyond one workgroup's table are found on the host
        if (!g.h_part_off || !g.h_prev_part_off || (g.d_prev_topic && !g.h_prev_topic))
            return fail(ctx, LA_EINVAL, "h_part_off, h_prev_part_off and (with d_prev_topic) h_prev_topic are required when max_partitions_per_topic exceeds %lld", (long long)la::kMovesLdsMaxPartitions);
        if (!offsets_ascend(g.h_part_off, T, N)) return fail(ctx, LA_EINVAL, "h_part_off must ascend from 0 to n_partitions");
        if (!offsets_ascend(g.h_prev_part_off, g.n_prev_topics, NP)) return fail(ctx, LA_EINVAL, "h_prev_part_off must ascend from 0 to n_prev_partitions");
        for (int64_t t = 0; h_prev_topic && t < T; ++t)
            if (h_prev_topic[t] < -1 || h_prev_topic[t] >= g.n_prev_topics)
                return fail(ctx, LA_EINVAL, "h_prev_topic[%lld] lies outside [-1, n_prev_topics)", (long long)t);
    }
    la::MovesLayoutsCall c{};
    c.c = moves_call_of(g);
    c.n_prev_topics = g.n_prev_topics;
    c.n_prev_partitions = NP;
    c.prev_part_off = g.d_prev_part_off;
    c.prev_topic = g.d_prev_topic;
    c.topic_added = g.d_topic_added;
    c.topic_removed = g.d_topic_removed;
    c.added = g.d_added;
    c.removed = g.d_removed;
    hipError_t e = la::assignment_moves_layouts_launch(sh.moves, c, g.h_part_off, g.h_prev_part_off, h_prev_topic,
                                                       sh.lanes[0].d_status, stream);
    return e != hipSuccess ? hip_fail(ctx, e, "assignment_moves: %s") : LA_OK;
}

// Who moved between two assignments (la_moves.hip; la_moves_layouts.hip when the previous one has a layout of its own).  The
// global form's table is the shard's own buffer, not the assign scratch: the results kept for la_group_last_by_member stay as
// they are.
LA_API int la_assignment_moves_device(la_ctx* ctx, const la_moves_args* args, void* stream) {
    return la_assignment_moves_device_on(ctx, 0, args, stream);
}

LA_API int la_assignment_moves_device_on(la_ctx* ctx, int shard, const la_moves_args* args, void* stream) {
    return shard_entry<true>(ctx, shard, "exception in la_assignment_moves_device", [&](Shard& sh) -> int {
        if (!args) return fail(ctx, LA_EINVAL, "args is NULL");
        // the struct has grown once: a caller built against the one-layout header says 128, and nothing behind that is read
        if (args->struct_size != kMovesArgsSizeOneLayout && args->struct_size < (int32_t)sizeof(la_moves_args))
            return fail(ctx, LA_EINVAL, "la_moves_args.struct_size is %d, this library takes %d or %d and above", (int)args->struct_size, kMovesArgsSizeOneLayout, (int)sizeof(la_moves_args));
        la_moves_args g{};
        memcpy(&g, args, args->struct_size == kMovesArgsSizeOneLayout ? (size_t)kMovesArgsSizeOneLayout : sizeof g);
        const bool layouts = g.d_prev_part_off != nullptr;
        if (g.n_topics < 0 || g.n_partitions < 0 || g.n_members < 0) return fail(ctx, LA_EINVAL, "negative size");
        if (g.n_members > la::kMovesMaxMembers) return fail(ctx, LA_EINVAL, "n_members must be below 2^30");
        if (g.d_prev_rank_map && g.n_prev_members < 0) return fail(ctx, LA_EINVAL, "negative n_prev_members");
        if (!g.d_prev_owner && !g.d_topic_moved && !g.d_member_gained && !g.d_member_lost && !g.d_moved &&
            !(layouts && (g.d_topic_added || g.d_topic_removed || g.d_added || g.d_removed)))
            return fail(ctx, LA_EINVAL, "every output is NULL");
        if (layouts) return moves_layouts(ctx, sh, g, (hipStream_t)stream);
        if (g.n_topics == 0 && g.n_partitions != 0) return fail(ctx, LA_EINVAL, "partitions without topics");
        if (g.n_partitions > 0 && (!g.d_part_off || !g.d_out_partition || !g.d_out_member_rank || !g.d_prev_partition ||
                                   !g.d_prev_member_rank))
            return fail(ctx, LA_EINVAL, "null buffer");
        if (g.max_partitions_per_topic > la::kMovesLdsMaxPartitions && g.n_partitions > 0) {
            // topics beyond one workgroup's table are found on the host
            if (!g.h_part_off)
                return fail(ctx, LA_EINVAL, "h_part_off is required when max_partitions_per_topic exceeds %lld", (long long)la::kMovesLdsMaxPartitions);
            if (g.h_part_off[0] != 0 || g.h_part_off[g.n_topics] != g.n_partitions)
                return fail(ctx, LA_EINVAL, "h_part_off must run from 0 to n_partitions");
            for (int32_t t = 0; t < g.n_topics; ++t)
                if (g.h_part_off[t + 1] < g.h_part_off[t]) return fail(ctx, LA_EINVAL, "offsets of topic %d decrease", t);
        }
        const la::MovesCall c = moves_call_of(g);
        hipError_t e = la::assignment_moves_launch(sh.moves, c, g.h_part_off, sh.lanes[0].d_status, (hipStream_t)stream);
        return e != hipSuccess ? hip_fail(ctx, e, "assignment_moves: %s") : LA_OK;
    });
}

// Certifies an assignment (la_verify.hip).  Without LA_FLAG_VERIFY_LARGE it owns no scratch: everything lives in the workgroups'
// LDS and the caller's outputs.  With the flag the topics over the LDS limit go through tables in device memory -- the shard's
// own buffer, not the assign scratch.  Either way the results kept for la_group_last_by_member stay as they are.
LA_API int la_verify_assignment_device(la_ctx* ctx, const la_device_batch* batch, int32_t* d_topic_verdict, int64_t* d_summary,
                                       void* stream) {
    return la_verify_assignment_device_on(ctx, 0, batch, d_topic_verdict, d_summary, stream);
}

LA_API int la_verify_assignment_device_on(la_ctx* ctx, int shard, const la_device_batch* batch, int32_t* d_topic_verdict,
                                          int64_t* d_summary, void* stream) {
    return shard_entry<true>(ctx, shard, "exception in la_verify_assignment_device", [&](Shard& sh) -> int {
        if (!batch) return fail(ctx, LA_EINVAL, "batch is NULL");
        const la_device_batch& b = *batch;
        if (b.n_topics < 0 || b.n_partitions < 0 || b.n_consumers < 0) return fail(ctx, LA_EINVAL, "negative size");
        if (!d_topic_verdict && !d_summary) return fail(ctx, LA_EINVAL, "d_topic_verdict and d_summary are both NULL");
        if (b.flags & LA_FLAG_WIRE_OUT)
            return fail(ctx, LA_EINVAL, "LA_FLAG_WIRE_OUT: unpack the results with la_unpack_results_on before verifying them");
        if (b.n_topics == 0 && (b.n_partitions != 0 || b.n_consumers != 0)) return fail(ctx, LA_EINVAL, "partitions or consumers without topics");
        if (b.n_topics > 0 && (!b.d_part_off || !b.d_cons_off)) return fail(ctx, LA_EINVAL, "null offsets");
        if (b.n_partitions > 0 && (!b.d_out_partition || !b.d_out_member_rank)) return fail(ctx, LA_EINVAL, "null results");
        if (b.n_partitions > 0 && (!b.d_partition_id || (!b.d_lag && (!b.d_end_off || !b.d_committed_off))))
            return fail(ctx, LA_EINVAL, "null per-partition input");
        if (b.n_consumers > 0 && !b.d_cons_rank) return fail(ctx, LA_EINVAL, "null cons_rank");
        if (!b.d_lag && b.reset_mode != LA_RESET_LATEST && !b.d_begin_off && b.n_partitions > 0)
            return fail(ctx, LA_EINVAL, "begin_off is required unless reset_mode is LA_RESET_LATEST");
        const bool large = (b.flags & LA_FLAG_VERIFY_LARGE) != 0;
        if (large) {
            // topics beyond one workgroup's LDS are found on the host; the global form works from these offsets alone
            if (!b.h_part_off || !b.h_cons_off)
                return fail(ctx, LA_EINVAL, "LA_FLAG_VERIFY_LARGE: h_part_off and h_cons_off are required");
            for (int32_t t = 0; t <= b.n_topics; ++t) {
                const int64_t p = b.h_part_off[t], k = b.h_cons_off[t];
                if (p < 0 || p > b.n_partitions || k < 0 || k > b.n_consumers || (t > 0 && (p < b.h_part_off[t - 1] || k < b.h_cons_off[t - 1])))
                    return fail(ctx, LA_EINVAL, "LA_FLAG_VERIFY_LARGE: h_part_off / h_cons_off must ascend inside [0, n_partitions] / [0, n_consumers] (topic %d)", t < b.n_topics ? t : t - 1);
            }
        }
        la::VerifyCall c{};
        c.n_topics = b.n_topics;
        c.reset_latest = b.reset_mode == LA_RESET_LATEST ? 1 : 0;
        c.n_partitions = b.n_partitions;
        c.n_consumers = b.n_consumers;
        c.max_partitions_per_topic = b.max_partitions_per_topic;
        c.max_consumers_per_topic = b.max_consumers_per_topic;
        c.part_off = b.d_part_off;
        c.cons_off = b.d_cons_off;
        c.pid = b.d_partition_id;
        c.begin = b.d_begin_off;
        c.end = b.d_end_off;
        c.committed = b.d_committed_off;
        c.lag = b.d_lag;
        c.cons_rank = b.d_cons_rank;
        c.out_pid = b.d_out_partition;
        c.out_rank = b.d_out_member_rank;
        c.out_total = b.d_out_total_lag;
        c.verdict = d_topic_verdict;
        c.summary = d_summary;
        hipError_t e = la::verify_assignment_launch(large ? &sh.verify : nullptr, c, b.h_part_off, b.h_cons_off,
                                                    sh.lanes[0].d_status, (hipStream_t)stream);
        return e != hipSuccess ? hip_fail(ctx, e, "verify_assignment: %s") : LA_OK;
    });
}

LA_API int la_group_by_member(la_ctx* ctx, int32_t n_topics, const int64_t* part_off, const int32_t* out_partition,
                              const int32_t* out_member_rank, int32_t n_members, int64_t* member_off,
                              int32_t* grouped_topic, int32_t* grouped_partition) {
    DeviceGuard restore_device;
    LaunchSpan span(ctx);
    if (!ctx) return LA_EINVAL;
    try {
        ctx->last_valid = false;                       // this call reuses the scratch the last results live in
        if (n_topics < 0 || n_members < 0) return fail(ctx, LA_EINVAL, "negative size");
        if (!member_off || (n_topics > 0 && !part_off)) return fail(ctx, LA_EINVAL, "null buffer");
        const int64_t n = n_topics > 0 ? part_off[n_topics] : 0;
        if (n < 0) return fail(ctx, LA_EINVAL, "part_off decreases");
        if (n > 0 && (!out_partition || !out_member_rank || !grouped_partition)) return fail(ctx, LA_EINVAL, "null buffer");
        // A large input is split like an assign call's: contiguous topic ranges over the shards (la_plan_shards), each
        // grouped on its own device, the lists concatenated in shard order (a member's list is its per-topic appends in
        // topic order, Main.java:177-184, :264) -- the code la_group_last_by_member runs on results already resident.
        int S = (int)ctx->shards.size();
        if (!ctx->split_always) {
            const int64_t by_size = n / (4 * kMinShardPartitions);
            if (by_size < S) S = by_size < 1 ? 1 : (int)by_size;
        }
        if (S > n_topics) S = n_topics;
        if (S > 1) {
            for (int32_t t = 0; t < n_topics; ++t)
                if (part_off[t + 1] < part_off[t]) return fail(ctx, LA_EINVAL, "part_off decreases");
            plan_ranges(part_off, 0, n_topics, S, ctx->last_bounds);
            ctx->last_shards = S;
            int rc = run_workers(ctx, S, [&](int i) -> int {
                Shard& sh = ctx->shards[(size_t)i];
                const int32_t t0 = ctx->last_bounds[i], t1 = ctx->last_bounds[i + 1];
                const int64_t p0 = part_off[t0], m = part_off[t1] - p0;
                sh.last_t0 = t0; sh.last_topics = t1 - t0; sh.last_p0 = p0; sh.last_n = m;
                if (t1 == t0) return LA_OK;
                LA_HIP(ctx, hipSetDevice(sh.device));
                const size_t tb = (size_t)(t1 - t0 + 1) * 8, nb4 = (size_t)m * 4;
                int r;
                if ((r = reserve(ctx, sh.part_off, tb + 16)) || (r = reserve(ctx, sh.out_pid, nb4 + 16)) ||
                    (r = reserve(ctx, sh.out_rank, nb4 + 16)))
                    return r;
                sh.local_part_off.resize((size_t)(t1 - t0) + 1);
                for (int32_t t = 0; t <= t1 - t0; ++t) sh.local_part_off[(size_t)t] = part_off[t0 + t] - p0;
                hipStream_t st = sh.lanes[0].stream;
                LA_HIP(ctx, hipMemcpyAsync(sh.part_off.p, sh.local_part_off.data(), tb, hipMemcpyHostToDevice, st));
                if (m) {
                    LA_HIP(ctx, hipMemcpyAsync(sh.out_pid.p, out_partition + p0, nb4, hipMemcpyHostToDevice, st));
                    LA_HIP(ctx, hipMemcpyAsync(sh.out_rank.p, out_member_rank + p0, nb4, hipMemcpyHostToDevice, st));
                }
                LA_HIP(ctx, hipStreamSynchronize(st));           // local_part_off is read by the copy until here
                sh.last_part_off = (const int64_t*)sh.part_off.p;
                sh.last_out_pid = (const int32_t*)sh.out_pid.p;
                sh.last_out_rank = (const int32_t*)sh.out_rank.p;
                return LA_OK;
            });
            if (rc) return rc;
            return group_last_impl(ctx, n_members, member_off, grouped_topic, grouped_partition);
        }
        Shard& sh = ctx->shards[0];                    // one stable sort of the whole array: the first device
        LA_HIP(ctx, hipSetDevice(sh.device));
        const size_t nb4 = (size_t)n * 4, tb = (size_t)(n_topics + 1) * 8, mb = ((size_t)n_members + 1) * 8;
        int rc;
        // scratch reuse: out_pid <- out_partition, out_rank <- member ranks, pid <- grouped_partition,
        // cons_rank <- grouped_topic, out_total <- member_off
        if ((rc = reserve(ctx, sh.part_off, tb + 16)) || (rc = reserve(ctx, sh.out_pid, nb4 + 16)) ||
            (rc = reserve(ctx, sh.out_rank, nb4 + 16)) || (rc = reserve(ctx, sh.pid, nb4 + 16)) ||
            (rc = reserve(ctx, sh.cons_rank, nb4 + 16)) || (rc = reserve(ctx, sh.out_total, mb + 16)))
            return rc;
        hipStream_t st = sh.lanes[0].stream;
        if (n_topics > 0) LA_HIP(ctx, hipMemcpyAsync(sh.part_off.p, part_off, tb, hipMemcpyHostToDevice, st));
        if (n) {
            LA_HIP(ctx, hipMemcpyAsync(sh.out_pid.p, out_partition, nb4, hipMemcpyHostToDevice, st));
            LA_HIP(ctx, hipMemcpyAsync(sh.out_rank.p, out_member_rank, nb4, hipMemcpyHostToDevice, st));
        }
        rc = la_group_by_member_device(ctx, n_topics, n, (const int64_t*)sh.part_off.p, (const int32_t*)sh.out_pid.p,
                                       (const int32_t*)sh.out_rank.p, n_members, (int64_t*)sh.out_total.p,
                                       grouped_topic ? (int32_t*)sh.cons_rank.p : nullptr, (int32_t*)sh.pid.p, st);
        if (rc) return rc;
        LA_HIP(ctx, hipMemcpyAsync(member_off, sh.out_total.p, mb, hipMemcpyDeviceToHost, st));
        if (n) {
            LA_HIP(ctx, hipMemcpyAsync(grouped_partition, sh.pid.p, nb4, hipMemcpyDeviceToHost, st));
            if (grouped_topic) LA_HIP(ctx, hipMemcpyAsync(grouped_topic, sh.cons_rank.p, nb4, hipMemcpyDeviceToHost, st));
        }
        return sync_status(ctx, sh.lanes[0], st);
    } catch (...) {
        return fail(ctx, LA_ENOMEM, "exception in la_group_by_member");
    }
}

LA_API int la_group_last_by_member(la_ctx* ctx, int32_t n_members, int64_t* member_off, int32_t* grouped_topic,
                                   int32_t* grouped_partition) {
    DeviceGuard restore_device;
    LaunchSpan span(ctx);
    if (!ctx) return LA_EINVAL;
    try {
        if (!ctx->last_valid)
            return fail(ctx, LA_EINVAL, "no result of la_assign_batch / la_assign_batch_lags is held on the device");
        if (n_members < 0) return fail(ctx, LA_EINVAL, "negative size");
        return group_last_impl(ctx, n_members, member_off, grouped_topic, grouped_partition);
    } catch (...) {
        return fail(ctx, LA_ENOMEM, "exception in la_group_last_by_member");
    }
}

// la_wake: ONE-PARTITION REBALANCE through the path a real small call takes (zero-copy staging, the tile kernel with its fused
// end, the spin on the completion word), waited for, and one empty kernel on every other stream of the context.  Why a whole
// call and why synchronous (tools/cold_probe.py through ctypes, profiles/r06_j_cold_probe.txt, one box, a 100-partition grouped
// call: 30 us back to back, 135-175 us after 1 s of idle): an empty asynchronous launch leaves it at 107-124 us, a 1-element
// la_compute_lag (copies, a kernel, a stream wait) at 69-74, a dummy rebalance through the real path at 43-45.  At the C ABI
// (tools/cold_c.c, profiles/r06_p_cold_c.txt): 23 us back to back, 85 us after 1 s of idle, 34 us with la_wake 1-20 ms before
// it.  What is cold after an idle second is not one thing (the queue, the link, the mapped pages' translations, the runtime's
// and this library's own code and data in the host's caches): the cheapest way to warm all of it is to do the thing once.  It
// costs the caller the cold call it spares the rebalance (~95 us) -- at the top of assign(), where milliseconds of broker round
// trips follow anyway.  The pending hint and the diagnostics of the last real call survive; results kept on the device do not.
LA_API int la_wake(la_ctx* ctx) {
    if (!ctx) return LA_EINVAL;
    DeviceGuard restore_device;
    const la_call_hints saved_hints = ctx->hints;
    const bool saved_set = ctx->hints_set;
    const int saved_pipeline = ctx->last_pipeline;
    const int64_t saved_launches = ctx->last_launches;
    ctx->hints_set = false;
    int rc = LA_OK;
    try {
        static const int64_t off[2] = {0, 1}, begin[1] = {0}, end[1] = {1}, committed[1] = {0};
        static const int32_t pid[1] = {0}, rank[1] = {0};
        int64_t member_off[2] = {0, 0};
        int32_t grouped_partition[1] = {0};
        HostCall c;
        c.T = 1; c.part_off = off; c.pid = pid; c.begin = begin; c.end = end; c.committed = committed;
        c.reset_mode = LA_RESET_EARLIEST; c.cons_off = off; c.cons_rank = rank;
        c.g_members = 1; c.g_off = member_off; c.g_part = grouped_partition;
        rc = assign_grouped(ctx, c);
        if (rc == LA_OK && !(member_off[1] == 1 && grouped_partition[0] == 0))
            rc = fail(ctx, LA_EHIP, "la_wake: the one-partition rebalance came back wrong (member_off %lld %lld, partition %d)",
                      (long long)member_off[0], (long long)member_off[1], (int)grouped_partition[0]);
    } catch (...) {
        rc = fail(ctx, LA_ENOMEM, "exception in la_wake");
    }
    ctx->hints = saved_hints;
    ctx->hints_set = saved_set;
    ctx->last_pipeline = saved_pipeline;
    ctx->last_launches = saved_launches;
    ctx->last_valid = false;                                  // (the staging buffers of the last real call were reused)
    if (rc != LA_OK) return rc;
    for (size_t s = 0; s < ctx->shards.size(); ++s) {
        Shard& sh = ctx->shards[s];
        LA_HIP(ctx, hipSetDevice(sh.device));
        for (size_t i = (s == 0 ? 1 : 0); i < sh.lanes.size(); ++i)          // (shard 0's first lane just ran the call)
            if (sh.lanes[i].stream) LA_HIP(ctx, la::wake_launch(sh.lanes[i].stream));
    }
    return LA_OK;
}

LA_API int la_assign_batch_grouped(la_ctx* ctx, int32_t n_topics, const int64_t* part_off, const int32_t* partition_id,
                                   const int64_t* begin_off, const int64_t* end_off, const int64_t* committed_off,
                                   int32_t reset_mode, const int64_t* cons_off, const int32_t* cons_rank, int32_t n_members,
                                   int64_t* member_off, int32_t* grouped_topic, int32_t* grouped_partition,
                                   int64_t* out_total_lag) {
    DeviceGuard restore_device;
    LaunchSpan span(ctx);
    HintSpender spend_hints(ctx);
    if (!ctx) return LA_EINVAL;
    try {
        HostCall c;
        c.T = n_topics; c.part_off = part_off; c.pid = partition_id; c.begin = begin_off; c.end = end_off; c.committed = committed_off;
        c.reset_mode = reset_mode; c.cons_off = cons_off; c.cons_rank = cons_rank;
        c.g_members = n_members; c.g_off = member_off; c.g_topic = grouped_topic; c.g_part = grouped_partition; c.out_total = out_total_lag;
        return assign_grouped(ctx, c);
    } catch (...) {
        return fail(ctx, LA_ENOMEM, "exception in la_assign_batch_grouped");
    }
}

LA_API int la_assign_batch_sparse(la_ctx* ctx, int32_t n_topics, const int64_t* part_off, const int32_t* partition_id,
                                  const int64_t* end_off, const int64_t* committed_off, int32_t reset_mode, int64_t n_none,
                                  const int64_t* none_index, const int64_t* none_begin, const int64_t* cons_off,
                                  const int32_t* cons_rank, int32_t* out_partition, int32_t* out_member_rank,
                                  int64_t* out_total_lag) {
    DeviceGuard restore_device;
    LaunchSpan span(ctx);
    HintSpender spend_hints(ctx);
    try {
        HostCall c;
        c.T = n_topics; c.part_off = part_off; c.pid = partition_id; c.end = end_off; c.committed = committed_off;
        c.reset_mode = reset_mode; c.cons_off = cons_off; c.cons_rank = cons_rank;
        c.out_pid = out_partition; c.out_rank = out_member_rank; c.out_total = out_total_lag;
        c.sparse = true; c.n_none = n_none; c.none_index = none_index; c.none_begin = none_begin;
        return assign_host(ctx, c);
    } catch (...) {
        return ctx ? fail(ctx, LA_ENOMEM, "exception in la_assign_batch_sparse") : LA_EINVAL;
    }
}

LA_API int la_assign_batch_grouped_sparse(la_ctx* ctx, int32_t n_topics, const int64_t* part_off, const int32_t* partition_id,
                                          const int64_t* end_off, const int64_t* committed_off, int32_t reset_mode,
                                          int64_t n_none, const int64_t* none_index, const int64_t* none_begin,
                                          const int64_t* cons_off, const int32_t* cons_rank, int32_t n_members,
                                          int64_t* member_off, int32_t* grouped_topic, int32_t* grouped_partition,
                                          int64_t* out_total_lag) {
    DeviceGuard restore_device;
    LaunchSpan span(ctx);
    HintSpender spend_hints(ctx);
    if (!ctx) return LA_EINVAL;
    try {
        HostCall c;
        c.T = n_topics; c.part_off = part_off; c.pid = partition_id; c.end = end_off; c.committed = committed_off;
        c.reset_mode = reset_mode; c.cons_off = cons_off; c.cons_rank = cons_rank;
        c.g_members = n_members; c.g_off = member_off; c.g_topic = grouped_topic; c.g_part = grouped_partition; c.out_total = out_total_lag;
        c.sparse = true; c.n_none = n_none; c.none_index = none_index; c.none_begin = none_begin;
        return assign_grouped(ctx, c);
    } catch (...) {
        return fail(ctx, LA_ENOMEM, "exception in la_assign_batch_grouped_sparse");
    }
}

LA_API int la_last_phase_times(la_ctx* ctx, la_phase_times* out) {
    return shard_entry<false>(ctx, 0, "exception in la_last_phase_times", [&](Shard& sh) -> int {
        if (!out) return fail(ctx, LA_EINVAL, "out is NULL");
        float ms[3] = {};
        int passes[4] = {};
        int64_t n = 0;
        const hipError_t e = la::large_profile_read(sh.lanes[0].large, ms, passes, &n);
        if (e == hipErrorNotReady)
            return fail(ctx, LA_EINVAL, "no large-path topic was profiled (LA_FLAG_PROFILE on la_assign_batch_device)");
        if (e != hipSuccess) return fail(ctx, LA_EHIP, "la_last_phase_times: %s", hipGetErrorString(e));
        out->n_partitions = n;
        out->id_passes = passes[0];
        out->key_passes = passes[1];
        out->keys_ms = ms[0];
        out->sort_ms = ms[1];
        out->greedy_ms = ms[2];
        out->keys_first = passes[2];
        out->redone = passes[3];
        return LA_OK;
    });
}

LA_API int la_last_phase_times_sized(la_ctx* ctx, void* out, size_t out_size) {
    if (!ctx) return LA_EINVAL;
    if (!out) return fail(ctx, LA_EINVAL, "out is NULL");
    la_phase_times full{};
    if (int rc = la_last_phase_times(ctx, &full)) return rc;
    memcpy(out, &full, out_size < sizeof full ? out_size : sizeof full);
    return LA_OK;
}

LA_API int la_sync_on(la_ctx* ctx, int shard, void* stream) {
    return shard_entry<false>(ctx, shard, "exception in la_sync", [&](Shard& sh) -> int {
        return sync_status(ctx, sh.lanes[0], (hipStream_t)stream);
    });
}

LA_API int la_sync(la_ctx* ctx, void* stream) { return la_sync_on(ctx, 0, stream); }
