// la_pinned_large.hip -- the pinned assignment for topics of any size: the LARGE FORM of la_pinned.hip (LA_FLAG_PINNED_LARGE).
//
// Topics of more than kPinnedMaxPartitions partitions and at most kPinnedMaxConsumers consumers, listed by the host from
// h_part_off / h_cons_off (PinnedBig, a pinned list one copy brings over), all of a call side by side.  Their positions are
// numbered through the topics: q = q0 of the topic + i, L in all.  The phases of the LDS kernel are launches over regions in device
// memory; the ONLY grid-wide order the kernels here introduce is the launch boundary (no grid barrier, no spin, no cooperative
// launch -- the radix passes are la_radix.hip's as they are).  Workgroup steps of kPinnedLargeStep positions are numbered through
// the topics, so a step lies inside ONE topic; a workgroup bisects the list for its step.  A step is also the CHUNK of the scan.
//   memsets  the sorts' control words = 0; bins, per-topic counters and the total = 0
//   sort     sort_launch over a LargeItem per topic (la_radix.h): keys (lag ^ kLagKeyFlip, id ^ kPidBias through the assign call's
//            arithmetic), plan, the digit passes of every tile class.  The sorted buffer of a topic holds, per position, the lag
//            (its key) and the partition id (its payload): the reference's order, what la_assign_batch_device writes
//   K1  classify: out_pid[p0 + i]; the claimant of (topic, id) from the cooperative table; the topic's rank segment bisected in
//       device memory.  PINNED: out_rank, and the topic's bins seeded by device-scope atomics (count u32, total u64: the wrapping
//       sum does not depend on the order).  Any other position is flagged free (a topic without consumers: rank -1).  The free
//       count of the chunk; pinned and foreign counts of the topic.  The sort's order is checked on the way (kStatusOrder), the
//       device's four offsets of the topic against the host's (kStatusShape) and the rank segment (kStatusUnsorted) by step 0
//   K2  exclusive scan over the chunk counts (one workgroup), the total
//   K3  compact: fpos[rank] = i of every free position -- ascending, topic after topic
//   K4  the levels, ONE workgroup per topic: the bins (count, total, rank) and the active set in LDS, 28 B per consumer; the
//       free list streams from device memory, the lags from the sorted keys.  The level rule is la_pinned.hip's: the consumers at
//       the minimal count m, sorted by (total, rank), take the next free partitions one each; then m + 1.
//       A RUN FOR A LONE CONSUMER: when the active set is ONE consumer and the second-smallest count is m2, it takes the next
//       r = min(m2 - m, F - f0) free partitions in one step -- a sole minimum stays the sole argmin until its count reaches m2:
//       whatever its total, its count compares below every other's.  Its total takes the wrapping sum of their lags.
//       At the end out_total, topic_free[t] and the topic's shares of the summary.
// Safe on any content: an index comes from a loop counter, a bisection, a scan, a compaction or a slot counter bounded by the
// consumer count -- each compared against its range before use -- never from an id or a rank.  Every loop is bounded (a level or
// a run hands out at least one partition, else kStatusInternal ends the topic); barriers stand in workgroup-uniform control flow;
// every pointer is a kernel argument or an offset from one.
//
// WORKING MEMORY (PinnedLargeScratch, the shard's own, grown before anything is enqueued), bytes per large-topic partition:
//   the sort's two buffers: 2 x (key 8 + payload 4) = 24, its look-back granules, 2 KiB per tile of >= 4 096 elements: <= 0.5 |
//   flag 1 | fpos 4  => about 30 bytes, + 4 per chunk of 1 024 positions, 12 per consumer and, per topic, 32 of counters and
//   the sort's control block and histograms (about 26 KiB).
#include <algorithm>
#include <vector>

#include "la_pinned_sort.h"
#include "la_device.h"
#include "la_radix.h"
#include "la_sticky_match.h"

namespace la {

namespace {

constexpr int kPlThreads = 256;
constexpr int kPlPer = 4;                           // consecutive positions of a thread per workgroup step
constexpr int kPlScanThreads = 1024;                // the one workgroup of K2
static_assert(kPinnedLargeStep == (int64_t)kPlPer * kPlThreads, "a step is what a workgroup covers");
static_assert(kPinnedLargeLaunches == 2 + 3 * kDigits + 4, "keys, plan, the passes of three tile classes, four phases");
static_assert(kPinnedLargeMaxPartitions < ((int64_t)1 << 30), "positions and counts fit 32 bits; single-kernel radix passes");
static_assert(kPlThreads / kWave <= 4 && kPlScanThreads / kWave <= 16, "wave totals of a scan");
// the levels' LDS: totals, active keys | counts, active indices, ranks | the waves' sums | four counters
static_assert((size_t)kPinnedMaxConsumers * (8 + 8 + 4 + 4 + 4) + 8 * (kPinnedThreads / kWave) + 4 * 4 <= 64 * 1024, "static LDS");

struct PinnedLargeArgs {
    PinnedCall c;
    CoopTable table;
    uint32_t* status;
    PinnedLargeWork g;
};

__device__ __forceinline__ int big_of_step(const PinnedLargeWork& g, int64_t step) {      // the last topic that starts at or before it
    int lo = 0, hi = g.n_big;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g.big[mid].step0 <= step) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the sorted keys of a topic: the buffer its plan left the data in
__device__ __forceinline__ const uint64_t* sorted_keys(const PinnedLargeWork& g, const PinnedBig& b, uint32_t* fin_out) {
    const SortCtl* ctl = reinterpret_cast<const SortCtl*>(g.base + b.o_ctl);
    const uint32_t fin = ctl->cur[kFinal];
    *fin_out = fin;
    return reinterpret_cast<const uint64_t*>(g.base + (fin ? b.o_k1 : b.o_k0));
}

// K1 (PHASE 1) and K3 (PHASE 3) of the file comment: a thread takes kPlPer CONSECUTIVE positions, so that a scan over the threads
// is a scan over the positions
template <int PHASE>
__global__ __launch_bounds__(kPlThreads) void pinned_large_kernel(PinnedLargeArgs a) {
    constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
    __shared__ uint32_t wave_tot[kPlThreads / kWave];
    const PinnedCall& c = a.c;
    const PinnedLargeWork& g = a.g;
    const int tid = (int)threadIdx.x;
    const int64_t L = g.n_pos;
    uint32_t bad = 0;
    for (int64_t step = blockIdx.x; step < g.n_steps; step += gridDim.x) {
        const int idx = big_of_step(g, step);       // workgroup-uniform, as all that follows from it
        const PinnedBig b = g.big[idx];
        const int64_t s = step - b.step0;
        const int64_t P = b.np;
        const int C = (int)b.nc;                    // (<= kPinnedMaxConsumers: the host listed the topic)
        const int32_t* ranks = c.cons_rank + b.c0;
        uint32_t n_free = 0, n_pinned = 0, n_foreign = 0;
        uint32_t mine = 0;                          // K3: bit u = position u of this thread is free

        if (PHASE == 1 && s == 0) {
            // the large topics are read through the host's offsets alone: the device's must be the same
            const int64_t t = b.topic;
            if (c.part_off[t] != b.p0 || c.part_off[t + 1] != b.p0 + P || c.cons_off[t] != b.c0 || c.cons_off[t + 1] != b.c0 + C)
                bad |= kStatusShape;
            for (int k = tid; k + 1 < C; k += kPlThreads)
                if (ranks[k] >= ranks[k + 1]) bad |= kStatusUnsorted;
        }
        uint32_t fin = 0;
        const uint64_t* key = nullptr;
        const uint32_t* val = nullptr;
        if (PHASE == 1) {
            key = sorted_keys(g, b, &fin);
            val = reinterpret_cast<const uint32_t*>(g.base + (fin ? b.o_v1 : b.o_v0));
        }

#pragma unroll
        for (int u = 0; u < kPlPer; ++u) {
            const int64_t i = s * kPinnedLargeStep + (int64_t)tid * kPlPer + u;
            if (i >= P) continue;
            const int64_t q = b.q0 + i;
            if (PHASE == 1) {
                const uint64_t kw = key[i];
                const uint32_t v = val[i];
                if (i > 0) {
                    const uint64_t kp = key[i - 1];
                    if (kp > kw || (kp == kw && val[i - 1] > v)) bad |= kStatusOrder;
                }
                const int32_t id = (int32_t)(v ^ kPidBias);
                c.out_pid[b.p0 + i] = id;
                const int32_t who = coop_table_lookup(a.table, b.topic, id, &bad);
                bool pinned = false;
                if (who >= 0 && C > 0) {
                    int lo = 0, hi = C;             // the last index with ranks[index] <= who, if any
                    while (hi - lo > 1) {
                        const int mid = lo + ((hi - lo) >> 1);
                        if (ranks[mid] <= who) lo = mid;
                        else hi = mid;
                    }
                    if (ranks[lo] == who) {
                        pinned = true;
                        c.out_rank[b.p0 + i] = who;
                        __hip_atomic_fetch_add(g.bcount + b.k0 + lo, 1u, __ATOMIC_RELAXED, kScope);
                        __hip_atomic_fetch_add(g.btotal + b.k0 + lo, (unsigned long long)(kw ^ kLagKeyFlip), __ATOMIC_RELAXED, kScope);
                    }
                }
                if (pinned) {
                    ++n_pinned;
                } else {
                    ++n_free;
                    if (who >= 0) ++n_foreign;
                    if (C == 0) c.out_rank[b.p0 + i] = -1;
                }
                g.flag[q] = pinned ? 0 : 1;
            } else {
                if (g.flag[q]) {
                    mine |= 1u << u;
                    ++n_free;
                }
            }
        }

        uint32_t all = 0;
        const uint32_t before = workgroup_excl_scan<false>(n_free, wave_tot, tid, kPlThreads, &all);
        if (PHASE == 1) {
            if (tid == 0) g.cfree[step] = all;
            n_pinned = wave_sum_u32(n_pinned);
            n_foreign = wave_sum_u32(n_foreign);
            if ((tid & (kWave - 1)) == 0) {
                if (n_pinned) __hip_atomic_fetch_add(g.ctr + 4 * idx + 0, (unsigned long long)n_pinned, __ATOMIC_RELAXED, kScope);
                if (n_foreign) __hip_atomic_fetch_add(g.ctr + 4 * idx + 1, (unsigned long long)n_foreign, __ATOMIC_RELAXED, kScope);
            }
        } else {
            uint64_t r = (uint64_t)g.cfree[step] + before;      // (K2 has made it exclusive)
#pragma unroll
            for (int u = 0; u < kPlPer; ++u) {
                if (!(mine & (1u << u))) continue;
                const int64_t i = s * kPinnedLargeStep + (int64_t)tid * kPlPer + u;
                if (r < (uint64_t)L) g.fpos[r] = (uint32_t)i;
                ++r;
            }
        }
    }
    if (bad) atomicOr(a.status, bad);
}

// K2: exclusive scan over one word per chunk, in place, by ONE workgroup: a thread takes a contiguous share
__global__ __launch_bounds__(kPlScanThreads) void pinned_chunk_scan_kernel(uint32_t* v, int64_t n, unsigned long long* tot) {
    __shared__ uint32_t wave_tot[kPlScanThreads / kWave];
    const int tid = (int)threadIdx.x;
    const int64_t per = (n + kPlScanThreads - 1) / kPlScanThreads;
    const int64_t i0 = (int64_t)tid * per < n ? (int64_t)tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    uint32_t agg = 0;
    for (int64_t i = i0; i < i1; ++i) agg += v[i];
    uint32_t all = 0;
    uint32_t run = workgroup_excl_scan<false>(agg, wave_tot, tid, kPlScanThreads, &all);
    for (int64_t i = i0; i < i1; ++i) {
        const uint32_t e = v[i];
        v[i] = run;
        run += e;
    }
    if (tid == 0) tot[0] = all;
}

// K4: the levels of one topic per workgroup
__global__ __launch_bounds__(kPinnedThreads) void pinned_levels_kernel(PinnedLargeArgs a) {
    __shared__ uint64_t btotal[kPinnedMaxConsumers];      // the bins' totals
    __shared__ uint64_t akey[kPinnedMaxConsumers];        // the active set: total ^ kTotalBias
    __shared__ uint32_t bcount[kPinnedMaxConsumers];
    __shared__ uint32_t aidx[kPinnedMaxConsumers];        // the active set: index into the rank segment
    __shared__ int32_t ranks[kPinnedMaxConsumers];
    __shared__ uint64_t wsum[kPinnedThreads / kWave];
    __shared__ uint32_t ctr[4];                           // 0: slots of the active set  1: the minimal count  2: the second-smallest
    const PinnedCall& c = a.c;
    const PinnedLargeWork& g = a.g;
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    uint32_t bad = 0;
    for (int idx = (int)blockIdx.x; idx < g.n_big; idx += (int)gridDim.x) {
        const PinnedBig b = g.big[idx];                   // (workgroup-uniform, as all that follows from it)
        const int64_t P = b.np, L = g.n_pos;
        const int C = b.nc <= kPinnedMaxConsumers ? (int)b.nc : 0;
        const uint64_t f_begin = g.cfree[b.step0];
        const uint64_t f_end = idx + 1 < g.n_big ? (uint64_t)g.cfree[g.big[idx + 1].step0] : (uint64_t)g.tot[0];
        const uint64_t n_pinned = g.ctr[4 * idx + 0], n_foreign = g.ctr[4 * idx + 1];
        uint32_t F = 0;
        if (f_end < f_begin || f_end > (uint64_t)L || f_end - f_begin > (uint64_t)P || n_pinned + (f_end - f_begin) != (uint64_t)P ||
            b.nc > kPinnedMaxConsumers)
            bad |= kStatusInternal;                       // (never expected: the scan and the counters disagree)
        else
            F = (uint32_t)(f_end - f_begin);
        uint32_t fin = 0;
        const uint64_t* key = sorted_keys(g, b, &fin);
        const uint32_t* fpos = g.fpos + f_begin;          // (read below F only, and f_begin + F <= L)

        for (int k = tid; k < C; k += kPinnedThreads) {
            ranks[k] = c.cons_rank[b.c0 + k];
            btotal[k] = g.btotal[b.k0 + k];
            bcount[k] = g.bcount[b.k0 + k];
        }
        if (tid == 0) { ctr[0] = 0; ctr[1] = 0xFFFFFFFFu; ctr[2] = 0xFFFFFFFFu; }
        __syncthreads();
        if (C > 0 && F > 0)
            for (int k = tid; k < C; k += kPinnedThreads) atomicMin(ctr + 1, bcount[k]);
        __syncthreads();

        if (C > 0 && F > 0) {
            uint32_t m = ctr[1], f0 = 0;
            while (f0 < F) {
                for (int k = tid; k < C; k += kPinnedThreads) {
                    if (bcount[k] == m) {
                        const uint32_t s = atomicAdd(ctr + 0, 1u);      // below C: every k takes at most one slot
                        akey[s] = btotal[k] ^ kTotalBias;
                        aidx[s] = (uint32_t)k;
                    }
                }
                __syncthreads();
                const uint32_t n_active = ctr[0];
                __syncthreads();
                if (tid == 0) ctr[0] = 0;                                // (the next level adds behind this level's last barrier)
                if (n_active == 0 || n_active > (uint32_t)C) { bad |= kStatusInternal; break; }      // never expected
                if (n_active == 1) {
                    // a run: the sole minimum takes partitions until its count reaches the second-smallest one
                    const uint32_t k = aidx[0];
                    if (k >= (uint32_t)C) { bad |= kStatusInternal; break; }
                    for (int j = tid; j < C; j += kPinnedThreads)
                        if ((uint32_t)j != k) atomicMin(ctr + 2, bcount[j]);
                    __syncthreads();
                    const uint32_t m2 = ctr[2];                          // 0xFFFFFFFF: the topic's only consumer
                    if (m2 <= m) { bad |= kStatusInternal; break; }      // never expected: every other count is above m
                    const uint32_t r = m2 - m < F - f0 ? m2 - m : F - f0;      // >= 1
                    const int32_t rank = ranks[k];
                    uint64_t sum = 0;
                    for (uint32_t i = (uint32_t)tid; i < r; i += kPinnedThreads) {
                        const uint32_t pos = fpos[f0 + i];
                        if ((int64_t)pos >= P) { bad |= kStatusInternal; continue; }
                        c.out_rank[b.p0 + pos] = rank;
                        sum += key[pos] ^ kLagKeyFlip;
                    }
                    sum = wave_sum_u64(sum);
                    if (lane == 0) wsum[wave] = sum;
                    __syncthreads();
                    if (tid == 0) {
                        uint64_t all = 0;
                        for (int w = 0; w < kPinnedThreads / kWave; ++w) all += wsum[w];
                        btotal[k] += all;
                        bcount[k] = m + r;
                        ctr[2] = 0xFFFFFFFFu;
                    }
                    f0 += r;
                    m += r;
                    __syncthreads();
                    continue;
                }
                pinned_sort<false>(akey, aidx, nullptr, (int)n_active, tid);
                const uint32_t n = n_active < F - f0 ? n_active : F - f0;
                for (uint32_t i = (uint32_t)tid; i < n; i += kPinnedThreads) {
                    const uint32_t pos = fpos[f0 + i], k = aidx[i];     // one consumer, one partition: no atomics
                    if ((int64_t)pos >= P || k >= (uint32_t)C) { bad |= kStatusInternal; continue; }
                    c.out_rank[b.p0 + pos] = ranks[k];
                    btotal[k] += key[pos] ^ kLagKeyFlip;
                    bcount[k] += 1;
                }
                f0 += n;
                m += 1;
                __syncthreads();
            }
        }
        __syncthreads();
        if (c.out_total)
            for (int k = tid; k < C; k += kPinnedThreads) c.out_total[b.c0 + k] = (int64_t)btotal[k];
        if (tid == 0) {
            const uint64_t n_free = (uint64_t)P - n_pinned;
            if (c.topic_free) c.topic_free[b.topic] = (int64_t)n_free;
            if (c.summary) {
                if (n_pinned) global_add(c.summary + 0, n_pinned);
                if (n_free) global_add(c.summary + 1, n_free);
                if (n_foreign) global_add(c.summary + 2, n_foreign);
                const uint64_t hits = n_pinned + n_foreign;
                if (hits) global_add(c.summary + 3, (uint64_t)0 - hits);      // claimed - hits = stale
            }
        }
        __syncthreads();                                                 // the next topic overwrites the LDS
    }
    if (bad) atomicOr(a.status, bad);
}

inline bool is_big(const int64_t* h_part_off, const int64_t* h_cons_off, int64_t t) {
    const int64_t np = h_part_off[t + 1] - h_part_off[t], nc = h_cons_off[t + 1] - h_cons_off[t];
    return np > kPinnedMaxPartitions && np <= kPinnedLargeMaxPartitions && nc <= kPinnedMaxConsumers;
}

// the regions of s.work behind a reserve
struct PinnedRegions {
    size_t o_sort_data, o_flag, o_fpos, o_cfree, o_zero2, o_ctr, o_tot, o_btotal, o_bcount, zero2_bytes, sort_zero, bytes;
};

// the sorts' zero parts at 0 (one memset), then everything else; false: the sizes do not fit size_t
bool regions_for(const PinnedLargeScratch& s, size_t sort_zero, size_t sort_data, PinnedRegions* out) {
    PinnedRegions r{};
    const size_t L = (size_t)s.n_pos, n_steps = (size_t)s.n_steps, n_big = (size_t)s.n_big, n_bins = (size_t)s.n_bins;
    size_t at = 0;
    bool ok = true;
    const auto take = [&](size_t count, size_t elem) {
        size_t bytes = 0;
        at = align_up(at, 256);
        const size_t o = at;
        ok = ok && mul_ok(count, elem, &bytes) && add_ok(at, bytes, &at);
        return o;
    };
    r.sort_zero = sort_zero;
    (void)take(sort_zero, 1);
    r.o_sort_data = take(sort_data, 1);
    r.o_fpos = take(L, 4);
    r.o_cfree = take(n_steps, 4);
    r.o_flag = take(L, 1);
    r.o_zero2 = r.o_ctr = take(4 * n_big, 8);       // (zeroed by one memset from here on)
    r.o_tot = take(1, 8);
    r.o_btotal = take(n_bins, 8);
    r.o_bcount = take(n_bins, 4);
    r.zero2_bytes = at - r.o_zero2;
    r.bytes = at;
    *out = r;
    return ok;
}

// The call's large topics in the sort's tile-class order, their layouts and the two sums of the sort's parts
struct SortPlan {
    std::vector<int64_t> topic;                     // topic of item j
    std::vector<SortLayout> lay;                    // of item j
    std::vector<size_t> zoff, doff;
    size_t zero = 0, data = 0;
};

bool sort_plan_for(const PinnedCall& c, const int64_t* h_part_off, const int64_t* h_cons_off, SortPlan* out) {
    SortPlan p;
    for (int64_t t = 0; t < c.n_topics; ++t)
        if (is_big(h_part_off, h_cons_off, t)) p.topic.push_back(t);
    std::vector<SortLayout> lay;
    for (const int64_t t : p.topic) lay.push_back(sort_layout(h_part_off[t + 1] - h_part_off[t], false, false));
    std::vector<size_t> order(p.topic.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return lay[x].sweep_threads < lay[y].sweep_threads; });
    std::vector<int64_t> topic;
    for (const size_t i : order) {
        if (lay[i].multi_kernel) return false;      // (LA_SORT_MULTIKERNEL, a lab hook: side-by-side sorts have no such form)
        topic.push_back(p.topic[i]);
        p.lay.push_back(lay[i]);
        p.zoff.push_back(p.zero);
        p.doff.push_back(p.data);
        if (!add_ok(p.zero, lay[i].zero_bytes, &p.zero) || !add_ok(p.data, lay[i].data_bytes, &p.data)) return false;
    }
    p.topic = topic;
    *out = std::move(p);
    return true;
}

constexpr size_t list_items_at(size_t n_big) { return (n_big * sizeof(PinnedBig) + 255) / 256 * 256; }

}  // namespace

void pinned_large_scratch_release(PinnedLargeScratch& s) {
    s.list.release();
    if (s.work) (void)hipFree(s.work);
    s = PinnedLargeScratch{};
}

hipError_t pinned_large_reserve(PinnedLargeScratch& s, const PinnedCall& c, const int64_t* h_part_off, const int64_t* h_cons_off) {
    hipError_t e;
    s.n_big = s.n_pos = s.n_steps = s.n_bins = 0;
    int64_t n_big = 0;
    for (int64_t t = 0; t < c.n_topics; ++t) n_big += is_big(h_part_off, h_cons_off, t) ? 1 : 0;
    if (n_big == 0) return hipSuccess;

    SortPlan plan;
    if (!sort_plan_for(c, h_part_off, h_cons_off, &plan)) return hipErrorOutOfMemory;
    size_t big_bytes = 0, item_bytes = 0, list_bytes = 0;
    if (!mul_ok((size_t)n_big, sizeof(PinnedBig), &big_bytes) || !mul_ok((size_t)n_big, sizeof(LargeItem), &item_bytes) ||
        !add_ok(list_items_at((size_t)n_big), item_bytes, &list_bytes))
        return hipErrorOutOfMemory;
    if ((e = s.list.reserve(list_bytes)) != hipSuccess) return e;

    // the topics, ascending; then the sort's items in tile-class order
    PinnedBig* bigs = static_cast<PinnedBig*>(s.list.h);
    LargeItem* items = reinterpret_cast<LargeItem*>(static_cast<char*>(s.list.h) + list_items_at((size_t)n_big));
    int64_t j = 0, n_pos = 0, n_steps = 0, n_bins = 0;
    for (int64_t t = 0; t < c.n_topics; ++t) {
        if (!is_big(h_part_off, h_cons_off, t)) continue;
        PinnedBig& b = bigs[j++];
        b = PinnedBig{};
        b.topic = (int32_t)t;
        b.p0 = h_part_off[t];
        b.np = h_part_off[t + 1] - b.p0;
        b.c0 = h_cons_off[t];
        b.nc = h_cons_off[t + 1] - b.c0;
        b.q0 = n_pos;
        b.step0 = n_steps;
        b.k0 = n_bins;
        n_pos += b.np;
        if (n_pos > kPinnedLargeMaxPartitions) return hipErrorOutOfMemory;
        n_steps += (b.np + kPinnedLargeStep - 1) / kPinnedLargeStep;
        n_bins += b.nc;
    }
    PinnedLargeScratch sized{};                     // (s.n_big stays 0 until the memory is there: a failed reserve leaves "no large topic")
    sized.n_big = n_big; sized.n_pos = n_pos; sized.n_steps = n_steps; sized.n_bins = n_bins;
    PinnedRegions r{};
    if (!regions_for(sized, plan.zero, plan.data, &r)) return hipErrorOutOfMemory;
    for (size_t i = 0; i < plan.topic.size(); ++i) {
        const SortLayout& L = plan.lay[i];
        const int64_t t = plan.topic[i];
        LargeItem& it = items[i];
        it = LargeItem{};
        it.p0 = h_part_off[t]; it.n_part = L.n; it.c0 = h_cons_off[t]; it.n_cons = h_cons_off[t + 1] - h_cons_off[t];
        it.n = L.n; it.n_tiles = L.n_tiles; it.n_groups = L.n_groups;
        const uint64_t z = plan.zoff[i], d = r.o_sort_data + plan.doff[i];
        it.o_ctl = z + L.o_ctl; it.o_hist = z + L.o_hist; it.o_ticket = z + L.o_ticket; it.o_state = z + L.o_state;
        it.o_gbase = d + L.o_gbase; it.o_k0 = d + L.o_k0; it.o_k1 = d + L.o_k1; it.o_v0 = d + L.o_v0; it.o_v1 = d + L.o_v1;
        it.o_samp = 0;                              // (never keys first: the lookup wants (lag, id) order from the passes themselves)
        it.o_flag = z + L.o_flag;
        const auto at = std::lower_bound(bigs, bigs + n_big, t, [](const PinnedBig& b, int64_t x) { return (int64_t)b.topic < x; });
        at->o_ctl = it.o_ctl; at->o_k0 = it.o_k0; at->o_k1 = it.o_k1; at->o_v0 = it.o_v0; at->o_v1 = it.o_v1;
    }
    if ((e = grow_device(&s.work, &s.work_cap, r.bytes)) != hipSuccess) return e;
    s.n_big = n_big; s.n_pos = n_pos; s.n_steps = n_steps; s.n_bins = n_bins;
    return hipSuccess;
}

hipError_t pinned_large_enqueue(PinnedLargeScratch& s, const PinnedCall& c, const CoopTable& table, uint32_t* status,
                                hipStream_t stream, PinnedLargeWork* out) {
    hipError_t e;
    *out = PinnedLargeWork{};
    if (s.n_big == 0) return hipSuccess;
    const size_t n_big = (size_t)s.n_big;
    const LargeItem* items = reinterpret_cast<const LargeItem*>(static_cast<const char*>(s.list.h) + list_items_at(n_big));

    // the sort job over the items as the reserve laid them out (tile-class order)
    SortJob job{};
    size_t sort_zero = 0, sort_data = 0;
    for (size_t i = 0; i < n_big; ++i) {
        const SortLayout L = sort_layout(items[i].n, false, false);
        if (L.multi_kernel) return hipErrorOutOfMemory;
        sort_zero += L.zero_bytes;
        sort_data += L.data_bytes;
        if (L.n > job.max_n) job.max_n = L.n;
        if (job.n_cls == 0 || job.cls[job.n_cls - 1].sweep_threads != L.sweep_threads) {
            if (job.n_cls == 3) return hipErrorInvalidValue;      // (never expected: the items are in class order)
            job.cls[job.n_cls++] = SortClass{(int)i, 0, L.sweep_threads, 0};
        }
        SortClass& k = job.cls[job.n_cls - 1];
        ++k.n;
        if (L.n_tiles > k.max_tiles) k.max_tiles = L.n_tiles;
    }
    PinnedRegions r{};
    if (!regions_for(s, sort_zero, sort_data, &r) || r.bytes > s.work_cap) return hipErrorOutOfMemory;
    int cus = 0;
    if ((e = device_cus(&cus)) != hipSuccess) return e;
    char* const base = static_cast<char*>(s.work);

    PinnedLargeWork g{};
    g.base = base;
    g.big = static_cast<const PinnedBig*>(s.list.d);
    g.n_big = (int32_t)std::min<int64_t>(s.n_big, 0x7FFFFFFF);      // (T is 32 bits wide)
    g.n_pos = s.n_pos;
    g.n_steps = s.n_steps;
    g.flag = reinterpret_cast<uint8_t*>(base + r.o_flag);
    g.fpos = reinterpret_cast<uint32_t*>(base + r.o_fpos);
    g.cfree = reinterpret_cast<uint32_t*>(base + r.o_cfree);
    g.ctr = reinterpret_cast<unsigned long long*>(base + r.o_ctr);
    g.tot = reinterpret_cast<unsigned long long*>(base + r.o_tot);
    g.btotal = reinterpret_cast<unsigned long long*>(base + r.o_btotal);
    g.bcount = reinterpret_cast<uint32_t*>(base + r.o_bcount);

    PinnedLargeArgs a{};
    a.c = c;
    a.table = table;
    a.status = status;
    a.g = g;

    LargeArgs la{};                                 // the batch's arrays as the sort's keys kernel reads them; an item has the segment
    la.pid = c.pid; la.begin = c.begin; la.end = c.end; la.committed = c.committed; la.lag = c.lag;
    la.status = status;
    la.reset_latest = c.reset_latest;
    la.max_lag_hint = la.max_id_hint = -1;
    job.b.atomic_rank = large_atomic_rank_supported();
    job.items = reinterpret_cast<const LargeItem*>(static_cast<const char*>(s.list.d) + list_items_at(n_big));
    job.count = (int)n_big;
    job.base = base;
    job.keys_first = false;
    job.pass_mask = kAllPasses;                     // (no bounds are known here; the device-side plan makes a constant digit's pass return at once)
    job.status = status;

    if ((e = s.list.upload(list_items_at(n_big) + n_big * sizeof(LargeItem), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(base, 0, r.sort_zero, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(base + r.o_zero2, 0, r.zero2_bytes, stream)) != hipSuccess) return e;
    if ((e = sort_launch(la, job, stream, nullptr)) != hipSuccess) return e;
    const int64_t grid = std::min<int64_t>(g.n_steps, (int64_t)cus * 8);
    if ((e = launch_grid<pinned_large_kernel<1>>(grid, kPlThreads, 0, stream, a)) != hipSuccess) return e;
    LA_LAUNCH(pinned_chunk_scan_kernel, dim3(1), dim3(kPlScanThreads), 0, stream, g.cfree, g.n_steps, g.tot);
    if ((e = launch_grid<pinned_large_kernel<3>>(grid, kPlThreads, 0, stream, a)) != hipSuccess) return e;
    if ((e = launch_grid<pinned_levels_kernel>(std::min<int64_t>(g.n_big, (int64_t)cus * 2), kPinnedThreads, 0, stream, a)) != hipSuccess) return e;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    *out = g;
    return hipSuccess;
}

}  // namespace la
