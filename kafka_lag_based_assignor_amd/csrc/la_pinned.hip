// la_pinned.hip -- the pinned assignment (la_assign_pinned_device, lagassign.h): the follow-up of a cooperative rebalance that
// moves nothing that is owned.  A partition whose claimant is one of its topic's consumers stays with it; every consumer's bin
// starts from what it holds; only the other partitions are dealt out, by the reference's rule (fewest partitions, then least lag,
// then lowest member id: Main.java:240-263) in the reference's order (lag descending, id ascending: Main.java:228-235).
//
// Nothing in the reference computes it.  The rounds kernels of the assign call rest on equal counts -- every consumer gets one
// partition per round -- and seeded bins break that, so the greedy here goes LEVEL by level instead: the consumers at the minimal
// count m, ordered by (total, rank), take the next free partitions one each in that order.  That IS the sequential argmin: while
// a consumer of the level waits its turn its key does not change, whoever was served has m + 1 partitions and compares above
// all of them, and nobody outside the level has fewer than m + 1.  When the level is used up the minimal count is m + 1 exactly.
// One sort of the active set and one parallel hand-out per level; a follow-up with level counts and few free partitions is a
// handful of levels, a catch-up of one consumer that is h partitions behind is h levels of one.
//
// One workgroup of kPinnedThreads per topic (resident grid, workgroups walk the topics), everything in LDS:
//   1  stage ids and lags (lag_of: the assign call's arithmetic), look every (topic, id) up in the shard's cooperative table
//   2  bisect the topic's rank segment for the claimant: PINNED (its index), FOREIGN or unowned; seed the bins with LDS atomics
//      (the wrapping sum does not depend on the order)
//   3  sort the positions by (lag desc, id asc); write the ids and the pinned owners
//   4  compact the free positions by a scan
//   5  the levels
// Every index comes from a loop counter, a bisection, a scan or a slot counter bounded by the consumer count -- never from an id
// or a rank; every walk is bounded (a level hands out at least one partition); no thread waits for another except at a barrier.
// The sort is the direction-free bitonic network in plain HIP: the lower index of every pair keeps the smaller record, so the
// positions from n on, which no pair touches, stand for +infinity and any n sorts without padding.
//
// With LA_FLAG_PINNED_LARGE the topics over the partition limit are la_pinned_large.hip's: pinned_launch lists them from the host's
// offsets, runs the large form between the insert launch and the kernel here, and the kernel skips a listed topic silently.
#include "la_pinned_sort.h"

namespace la {

namespace {

// LDS, 8-byte arrays first: the partitions' sort keys, the bins' totals, the active set's keys | the partitions' tie-breaks and
// owners, the free positions | the bins' counts, the active set's indices, the rank segment | the waves' sums and three counters
constexpr size_t kPinnedLds = (size_t)kPinnedMaxPartitions * (8 + 4 + 4 + 4) + (size_t)kPinnedMaxConsumers * (8 + 8 + 4 + 4 + 4) +
                              4 * (kPinnedThreads / kWave) + 4 * 4;
static_assert(kPinnedMaxPartitions == 4 * kPinnedThreads, "the scan takes four positions per thread");
static_assert(kPinnedMaxConsumers <= kPinnedMaxPartitions && kPinnedMaxPartitions < (1 << 30), "indices and counts fit 32 bits");
static_assert(kPinnedLds <= 160 * 1024, "a topic at both limits fits one workgroup's LDS on gfx950");
static_assert(kPinnedThreads % kWave == 0 && kPinnedThreads <= 1024, "whole wavefronts, one workgroup");

constexpr int32_t kOwnNobody = -1, kOwnForeign = -2;      // pown: the consumer's index when pinned, else one of these

struct PinnedArgs {
    PinnedCall c;
    CoopTable table;
    uint32_t* status;
    const PinnedBig* big;       // the topics of the large form, ascending in topic (n_big == 0: none, null)
    int32_t n_big;
};

__global__ __launch_bounds__(kPinnedThreads) void pinned_kernel(PinnedArgs a) {
    extern __shared__ uint64_t pinned_lds[];
    uint64_t* const pkey = pinned_lds;                                   // [P] (uint64) lag ^ kLagKeyFlip
    uint64_t* const btotal = pkey + kPinnedMaxPartitions;                // [C] the bins' totals
    uint64_t* const akey = btotal + kPinnedMaxConsumers;                 // [C] the active set: total ^ kTotalBias
    uint32_t* const ptb = reinterpret_cast<uint32_t*>(akey + kPinnedMaxConsumers);      // [P] id ^ kPidBias
    int32_t* const pown = reinterpret_cast<int32_t*>(ptb + kPinnedMaxPartitions);       // [P]
    uint32_t* const fpos = reinterpret_cast<uint32_t*>(pown + kPinnedMaxPartitions);    // [P] the free positions, ascending
    uint32_t* const bcount = fpos + kPinnedMaxPartitions;                // [C]
    uint32_t* const aidx = bcount + kPinnedMaxConsumers;                 // [C] the active set: index into the rank segment
    int32_t* const ranks = reinterpret_cast<int32_t*>(aidx + kPinnedMaxConsumers);      // [C]
    uint32_t* const wsum = reinterpret_cast<uint32_t*>(ranks + kPinnedMaxConsumers);    // one per wavefront
    uint32_t* const ctr = wsum + kPinnedThreads / kWave;                 // 0: slots of the active set  1: the minimal count

    const PinnedCall& c = a.c;
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t T = c.n_topics, N = c.n_partitions, K = c.n_consumers;
    uint32_t bad = 0;
    uint64_t n_pinned = 0, n_free = 0, n_foreign = 0;
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        // (everything up to the first barrier is the same in every thread: the offsets are loaded from one address)
        if (a.n_big > 0) {                                               // the large form's topic: not this kernel's, no error
            int lo = 0, hi = a.n_big;
            while (hi - lo > 1) {
                const int mid = lo + ((hi - lo) >> 1);
                if ((int64_t)a.big[mid].topic <= t) lo = mid;
                else hi = mid;
            }
            if ((int64_t)a.big[lo].topic == t) continue;
        }
        const int64_t p0 = c.part_off[t], p1 = c.part_off[t + 1], c0 = c.cons_off[t], c1 = c.cons_off[t + 1];
        if (p0 < 0 || p1 < p0 || p1 > N || c0 < 0 || c1 < c0 || c1 > K) { bad |= kStatusShape; continue; }
        if (p1 - p0 > kPinnedMaxPartitions || c1 - c0 > kPinnedMaxConsumers) { bad |= kStatusShape; continue; }
        const int P = (int)(p1 - p0), C = (int)(c1 - c0);

        // 1: the topic into LDS, the claimants from the table
        for (int j = tid; j < P; j += kPinnedThreads) {
            const int64_t i = p0 + j;
            const int32_t id = c.pid[i];
            pkey[j] = (uint64_t)lag_of(c, i) ^ kLagKeyFlip;
            ptb[j] = (uint32_t)id ^ kPidBias;
            pown[j] = coop_table_lookup(a.table, (int32_t)t, id, &bad);
        }
        for (int k = tid; k < C; k += kPinnedThreads) {
            ranks[k] = c.cons_rank[c0 + k];
            btotal[k] = 0;
            bcount[k] = 0;
        }
        if (tid == 0) { ctr[0] = 0; ctr[1] = 0xFFFFFFFFu; }
        __syncthreads();

        // 2: who of the claimants consumes the topic; their partitions into the bins
        for (int k = tid; k + 1 < C; k += kPinnedThreads)
            if (ranks[k] >= ranks[k + 1]) bad |= kStatusUnsorted;
        for (int j = tid; j < P; j += kPinnedThreads) {
            const int32_t q = pown[j];
            int32_t own = q >= 0 ? kOwnForeign : kOwnNobody;
            if (q >= 0 && C > 0) {
                int lo = 0, hi = C;                                      // the last index with ranks[index] <= q, if any
                while (hi - lo > 1) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (ranks[mid] <= q) lo = mid;
                    else hi = mid;
                }
                if (ranks[lo] == q) {
                    own = lo;
                    atomicAdd(bcount + lo, 1u);
                    atomicAdd(reinterpret_cast<unsigned long long*>(btotal + lo), (unsigned long long)(pkey[j] ^ kLagKeyFlip));
                }
            }
            pown[j] = own;
        }
        __syncthreads();

        // 3: the reference's order; ids and pinned owners out
        pinned_sort<true>(pkey, ptb, pown, P, tid);
        uint32_t mine = 0;                                               // bit i: position 4 tid + i is free
        for (int i = 0; i < 4; ++i) {
            const int pos = 4 * tid + i;
            if (pos >= P) break;
            const int32_t own = pown[pos];
            c.out_pid[p0 + pos] = (int32_t)(ptb[pos] ^ kPidBias);
            if (own >= 0) {
                c.out_rank[p0 + pos] = ranks[own];
                ++n_pinned;
            } else {
                mine |= 1u << i;
                ++n_free;
                if (own == kOwnForeign) ++n_foreign;
                if (C == 0) c.out_rank[p0 + pos] = -1;
            }
        }

        // 4: the free positions, ascending
        const uint32_t cnt = (uint32_t)__builtin_popcount(mine);
        const uint32_t incl = wave_incl_scan_u32(cnt);
        if (lane == kWave - 1) wsum[wave] = incl;
        __syncthreads();
        uint32_t at = incl - cnt, F = 0;
        for (int w = 0; w < kPinnedThreads / kWave; ++w) {
            const uint32_t s = wsum[w];
            if (w < wave) at += s;
            F += s;
        }
        for (int i = 0; i < 4; ++i)
            if (mine & (1u << i)) fpos[at++] = (uint32_t)(4 * tid + i);
        if (C > 0 && F > 0)
            for (int k = tid; k < C; k += kPinnedThreads) atomicMin(ctr + 1, bcount[k]);
        if (tid == 0 && c.topic_free) c.topic_free[t] = (int64_t)F;
        __syncthreads();

        // 5: the levels
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
                pinned_sort<false>(akey, aidx, nullptr, (int)n_active, tid);
                const uint32_t g = n_active < F - f0 ? n_active : F - f0;
                for (uint32_t i = (uint32_t)tid; i < g; i += kPinnedThreads) {
                    const uint32_t pos = fpos[f0 + i], k = aidx[i];     // one consumer, one partition: no atomics
                    c.out_rank[p0 + pos] = ranks[k];
                    btotal[k] += pkey[pos] ^ kLagKeyFlip;
                    bcount[k] += 1;
                }
                f0 += g;
                m += 1;
                __syncthreads();
            }
        }
        if (c.out_total)
            for (int k = tid; k < C; k += kPinnedThreads) c.out_total[c0 + k] = (int64_t)btotal[k];
        __syncthreads();                                                 // the next topic overwrites the LDS
    }
    if (c.summary) {
        n_pinned = wave_sum_u64(n_pinned);
        n_free = wave_sum_u64(n_free);
        n_foreign = wave_sum_u64(n_foreign);
        if (lane == 0) {
            if (n_pinned) global_add(c.summary + 0, n_pinned);
            if (n_free) global_add(c.summary + 1, n_free);
            if (n_foreign) global_add(c.summary + 2, n_foreign);
            const uint64_t hits = n_pinned + n_foreign;
            if (hits) global_add(c.summary + 3, (uint64_t)0 - hits);    // claimed - hits = stale
        }
    }
    if (bad) atomicOr(a.status, bad);
}

}  // namespace

hipError_t pinned_launch(CoopScratch& s, const PinnedCall& c, uint32_t* status, hipStream_t stream, PinnedLargeScratch* large,
                         const int64_t* h_part_off, const int64_t* h_cons_off) {
    hipError_t e;
    const int64_t T = c.n_topics;
    // the table and the large form's memory first: when either cannot be had nothing has been enqueued
    PinnedArgs a{};
    if ((e = coop_table_reserve(s, c.n_owned, &a.table)) != hipSuccess) return e;
    if (large && (e = pinned_large_reserve(*large, c, h_part_off, h_cons_off)) != hipSuccess) return e;
    a.c = c;
    a.status = status;
    if (c.topic_free && T && (e = hipMemsetAsync(c.topic_free, 0, (size_t)T * 8, stream)) != hipSuccess) return e;
    if (c.summary && (e = hipMemsetAsync(c.summary, 0, 4 * 8, stream)) != hipSuccess) return e;
    CoopCall owned{};
    owned.n_topics = c.n_topics;
    owned.n_members = c.n_members;
    owned.n_owned = c.n_owned;
    owned.owned_off = c.owned_off;
    owned.owned_topic = c.owned_topic;
    owned.owned_partition = c.owned_partition;
    if ((e = coop_table_insert_launch(a.table, owned, c.summary ? c.summary + 3 : nullptr, status, stream)) != hipSuccess) return e;
    if (large && large->n_big > 0) {
        PinnedLargeWork g{};
        if ((e = pinned_large_enqueue(*large, c, a.table, status, stream, &g)) != hipSuccess) return e;
        a.big = g.big;
        a.n_big = g.n_big;
    }
    return launch_resident_lds<pinned_kernel, kPinnedLds>(T, kPinnedThreads, kPinnedLds, stream, a);
}

}  // namespace la
