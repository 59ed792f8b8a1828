// la_verify.hip -- certify an assignment on the device (la_verify_assignment_device, lagassign.h).
//
// The reference's result for a topic is unique (Main.java:204-266): the partitions by (lag descending, id ascending), and in
// every round of C positions the k-th partition to the k-th consumer by (total lag at the start of the round, rank) --
// oracle/round_form.py states it.  Checking that needs neither the sort nor the chain of dependent rounds:
//
//   V1  every output id is an input id of the topic, none twice            hash join (la_join.h), payload = the input's index
//   V2  neighbours are in (lag desc, id asc) order                          independent compares on the lags the join found
//   V3  owners subscribe, are distinct inside a round, and their keys (total before the round, rank) ascend along the
//       round; in a partial last round every consumer left out has a larger key than the last one picked
//   V4  out_total_lag is every consumer's final total
//
// One workgroup per topic, persistent workgroups walk topics blockIdx.x, + gridDim.x, ...  Per topic, in LDS:
//   [A: the table, 2^ceil(log2(2 P)) words; once the lookups are done: before[P] | tot_last[C]]
//   [lag[P]] [rank[C]] [slot[rounds x C] of 16 bits] [kidx[P] of 16 bits] [the topic's verdict bits]
//   1  clear the table and the slots, stage the ranks
//   2  insert the input ids (a duplicate: UNCHECKED); ranks strictly ascending (else UNCHECKED)
//   3  look every output id up (a miss or a second hit: IDS), lag[i] from the input entry; bisect the owner's rank -> k
//      (a miss: OWNER), slot[round x C + k] = i
//   4  neighbours' order (V2); slot read back: another entry's index means two owners in one round (OWNER)
//   5  one thread per consumer walks its rounds: before[i] = its total so far, tot_last = its total before the last round,
//      the final total against out_total_lag (V4)
//   6  (before, rank) of neighbours that share a round; the consumers a partial last round left out (V3)
//   7  the verdict: one plain store, counts and lowest indices kept by thread 0 and added to the summary once per workgroup
// Every phase is safe on any content: an index comes from the join's own payload or from a bisection, never from an id or a
// rank, so a failing topic is walked to the end like any other and leaves nothing behind -- every word a later topic reads it
// has written itself behind a barrier.  Accesses are one element wide.  No thread waits for another; every walk is bounded.
#include <algorithm>

#include "la_kernels.h"
#include "la_device.h"
#include "la_join.h"

namespace la {

namespace {

constexpr int kVerifyThreads = 256;
constexpr int kVerifyFewThreads = 64;               // topics up to kVerifyFewPartitions: one wavefront, barriers cost nothing
constexpr int64_t kVerifyFewPartitions = 256;
constexpr uint16_t kNoIndex = 0xFFFF;
static_assert(kVerifyMaxPartitions <= kNoIndex && kVerifyMaxConsumers <= kNoIndex, "16-bit indices");

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

struct VerifyArgs {
    VerifyCall c;
    uint32_t* status;
    int32_t cap_p, cap_c;       // partitions / consumers of a topic the LDS request holds
    uint32_t off_lag, off_rank, off_slot, off_kidx, off_bits;      // byte offsets of the regions behind A
};

struct VerifyLayout {
    uint32_t off_lag, off_rank, off_slot, off_kidx, off_bits;
    size_t bytes;
};

inline int ceil_log2(int64_t x) {                  // smallest b with 2^b >= x, at least 1
    int b = 1;
    while (((int64_t)1 << b) < x) ++b;
    return b;
}

inline VerifyLayout layout_for(int64_t cap_p, int64_t cap_c) {
    VerifyLayout l{};
    const size_t a = std::max((size_t)8 << ceil_log2(2 * cap_p), (size_t)8 * (size_t)(cap_p + cap_c));
    size_t at = up16(a);
    l.off_lag = (uint32_t)at;   at += up16(8 * (size_t)cap_p);
    l.off_rank = (uint32_t)at;  at += up16(4 * (size_t)cap_c);
    l.off_slot = (uint32_t)at;  at += up16(2 * (size_t)(cap_p + cap_c));      // rounds x C = ceil(P / C) C < P + C
    l.off_kidx = (uint32_t)at;  at += up16(2 * (size_t)cap_p);
    l.off_bits = (uint32_t)at;  at += 16;
    l.bytes = at;
    return l;
}
constexpr size_t kVerifyMaxLdsBytes = 8 * 2 * (size_t)kVerifyMaxPartitions + 8 * (size_t)kVerifyMaxPartitions +
                                      4 * (size_t)kVerifyMaxConsumers + 2 * (size_t)(kVerifyMaxPartitions + kVerifyMaxConsumers) +
                                      2 * (size_t)kVerifyMaxPartitions + 16;
static_assert((kVerifyMaxPartitions & (kVerifyMaxPartitions - 1)) == 0, "2 x the limit is the table of the largest topic");
static_assert(kVerifyMaxConsumers <= kVerifyMaxPartitions, "before | tot_last fit the largest table");
static_assert(kVerifyMaxLdsBytes <= 160 * 1024, "one workgroup's LDS on gfx950");

// computePartitionLag (Main.java:376-404) of input entry i, as the assign call computes it; `begin` only where it is read
__device__ __forceinline__ int64_t lag_of(const VerifyCall& c, int64_t i) {
    if (c.lag) return c.lag[i];
    const int64_t end = c.end[i], committed = c.committed[i];
    int64_t begin = 0;
    if (committed < 0 && !c.reset_latest && c.begin) begin = c.begin[i];
    return partition_lag(begin, end, committed, c.reset_latest != 0);
}

struct VerifyTally {            // thread 0: what this workgroup's topics add to the summary
    uint64_t failed = 0, unchecked = 0;
    uint64_t first_failed = ~0ull, first_unchecked = ~0ull;
};

__device__ __forceinline__ void record(const VerifyCall& c, VerifyTally& y, int64_t t, uint32_t bits) {
    if (bits & kVerdictUnchecked) {
        bits = kVerdictUnchecked;                   // a topic that could not be verified says nothing else
        ++y.unchecked;
        if ((uint64_t)t < y.first_unchecked) y.first_unchecked = (uint64_t)t;
    } else if (bits) {
        ++y.failed;
        if ((uint64_t)t < y.first_failed) y.first_failed = (uint64_t)t;
    }
    if (c.verdict) c.verdict[t] = (int32_t)bits;
}

__global__ __launch_bounds__(kVerifyThreads) void verify_kernel(VerifyArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char verify_lds[];
    constexpr int kScope = __HIP_MEMORY_SCOPE_WORKGROUP;
    const VerifyCall& c = a.c;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    uint64_t* table = reinterpret_cast<uint64_t*>(verify_lds);
    int64_t* before = reinterpret_cast<int64_t*>(verify_lds);            // A again, once the lookups are done
    int64_t* tot_last = before + a.cap_p;
    int64_t* lag = reinterpret_cast<int64_t*>(verify_lds + a.off_lag);
    int32_t* rank = reinterpret_cast<int32_t*>(verify_lds + a.off_rank);
    uint16_t* slot = reinterpret_cast<uint16_t*>(verify_lds + a.off_slot);
    uint16_t* kidx = reinterpret_cast<uint16_t*>(verify_lds + a.off_kidx);
    uint32_t* topic_bits = reinterpret_cast<uint32_t*>(verify_lds + a.off_bits);
    if (tid == 0) *topic_bits = 0;                  // (the first topic's barriers order it before the first OR)
    uint32_t bad = 0;
    VerifyTally tally;
    for (int64_t t = blockIdx.x; t < c.n_topics; t += gridDim.x) {
        // workgroup-uniform, as all that follows from it
        const int64_t p0 = c.part_off[t], p1 = c.part_off[t + 1], c0 = c.cons_off[t], c1 = c.cons_off[t + 1];
        const int64_t np = p1 - p0, nc = c1 - c0;
        const bool outside = p0 < 0 || p1 < p0 || p1 > c.n_partitions || c0 < 0 || c1 < c0 || c1 > c.n_consumers;
        const bool over_limit = !outside && (np > kVerifyMaxPartitions || nc > kVerifyMaxConsumers);
        const bool over_hint = !outside && !over_limit && (np > a.cap_p || nc > a.cap_c);
        if (outside || over_limit || over_hint) {   // nothing is read through such offsets
            if (outside || over_hint) bad |= kStatusShape;
            if (tid == 0) record(c, tally, t, kVerdictUnchecked);
            continue;
        }
        const int P = (int)np, C = (int)nc;
        const int bits = P > 0 ? 32 - __builtin_clz((uint32_t)(2 * P - 1)) : 1;      // 2^bits >= 2 P: at most half full
        const int rounds = C > 0 ? (P + C - 1) / C : 0;
        uint32_t v = 0;

        // 1
        if (P > 0)
            for (int i = tid; i < (1 << bits); i += nt) table[i] = 0;
        for (int i = tid; i < rounds * C; i += nt) slot[i] = kNoIndex;
        for (int k = tid; k < C; k += nt) rank[k] = c.cons_rank[c0 + k];
        __syncthreads();

        // 2
        for (int j = tid; j < P; j += nt) {
            const uint32_t st = table_insert<kScope>(table, bits, c.pid[p0 + j], j);
            if (st) v |= kVerdictUnchecked;
            bad |= st & kStatusInternal;
        }
        for (int k = tid; k + 1 < C; k += nt)
            if (!(rank[k] < rank[k + 1])) v |= kVerdictUnchecked;
        __syncthreads();

        // 3
        for (int i = tid; i < P; i += nt) {
            int32_t j = 0;
            const uint32_t st = table_lookup<kScope>(table, bits, c.out_pid[p0 + i], &j);
            int64_t l = 0;
            if (st) {
                v |= kVerdictIds;
                bad |= st & kStatusInternal;
            } else if (j >= 0 && j < P) {           // (the payload this topic's insert stored)
                l = lag_of(c, p0 + j);
            } else {
                v |= kVerdictIds;
                bad |= kStatusInternal;
            }
            lag[i] = l;
            const int32_t r = c.out_rank[p0 + i];
            uint16_t k = kNoIndex;
            if (C == 0) {
                if (r != -1) v |= kVerdictOwner;
            } else {
                int lo = 0, hi = C;                 // first k with rank[k] >= r; the interval shrinks whatever the ranks hold
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (rank[mid] < r) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < C && rank[lo] == r) {
                    k = (uint16_t)lo;
                    slot[(i / C) * C + lo] = (uint16_t)i;
                } else {
                    v |= kVerdictOwner;
                }
            }
            kidx[i] = k;
        }
        __syncthreads();

        // 4
        for (int i = tid; i < P; i += nt) {
            if (i + 1 < P) {
                const int64_t l0 = lag[i], l1 = lag[i + 1];
                if (!(l0 > l1) && (l0 != l1 || !(c.out_pid[p0 + i] < c.out_pid[p0 + i + 1]))) v |= kVerdictOrder;
            }
            const uint16_t k = kidx[i];
            if (k != kNoIndex && slot[(i / C) * C + k] != (uint16_t)i) v |= kVerdictOwner;
        }
        // 5 (touches A, which 4 does not)
        for (int k = tid; k < C; k += nt) {
            uint64_t tot = 0;
            for (int r = 0; r < rounds; ++r) {
                if (r == rounds - 1) tot_last[k] = (int64_t)tot;
                const uint16_t i = slot[r * C + k];
                if (i != kNoIndex) {
                    before[i] = (int64_t)tot;
                    tot += (uint64_t)lag[i];
                }
            }
            if (c.out_total && c.out_total[c0 + k] != (int64_t)tot) v |= kVerdictTotals;
        }
        __syncthreads();

        // 6
        if (C > 0) {
            for (int i = tid; i + 1 < P; i += nt) {
                if ((i + 1) % C == 0) continue;     // i closes its round
                const uint16_t k0 = kidx[i], k1 = kidx[i + 1];
                if (k0 == kNoIndex || k1 == kNoIndex) continue;
                const int64_t b0 = before[i], b1 = before[i + 1];
                if (!(b0 < b1 || (b0 == b1 && rank[k0] < rank[k1]))) v |= kVerdictGreedy;
            }
            const uint16_t k_last = P > 0 ? kidx[P - 1] : kNoIndex;
            if (P % C != 0 && k_last != kNoIndex) {
                const int64_t b_last = before[P - 1];
                const int32_t r_last = rank[k_last];
                for (int k = tid; k < C; k += nt) {
                    if (slot[(rounds - 1) * C + k] != kNoIndex) continue;
                    const int64_t b = tot_last[k];
                    if (!(b > b_last || (b == b_last && rank[k] > r_last))) v |= kVerdictGreedy;
                }
            }
        }

        // 7
        v = wave_or_u32(v);
        if ((tid & (kWave - 1)) == 0 && v) __hip_atomic_fetch_or(topic_bits, v, __ATOMIC_RELAXED, kScope);
        __syncthreads();                            // (also: every thread is done with this topic's LDS)
        if (tid == 0) {                             // (thread 0 also zeroes the word for the next topic: barriers in between)
            const uint32_t all = *topic_bits;
            *topic_bits = 0;
            record(c, tally, t, all);
        }
    }
    if (tid == 0 && c.summary) {                    // [2], [3] hold all ones (-1) until a topic is counted: an unsigned minimum
        unsigned long long* s = reinterpret_cast<unsigned long long*>(c.summary);
        if (tally.failed) {
            __hip_atomic_fetch_add(s + 0, (unsigned long long)tally.failed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(s + 2, (unsigned long long)tally.first_failed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tally.unchecked) {
            __hip_atomic_fetch_add(s + 1, (unsigned long long)tally.unchecked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(s + 3, (unsigned long long)tally.first_unchecked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (bad) atomicOr(a.status, bad);
}

// Resident workgroups of the kernel for a workgroup size and its dynamic LDS, per device; one word per device:
// LDS bytes << 40 | threads << 24 | workgroups.  It remembers the last request only (host arithmetic otherwise).
hipError_t verify_resident(int threads, size_t lds, int* out) {
    static std::atomic<uint64_t> s_cache[32];
    int dev = 0, cus = 0, per_cu = 0;
    hipError_t e;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    const bool cached = dev >= 0 && dev < 32;
    const uint64_t key = ((uint64_t)lds << 40) | ((uint64_t)threads << 24);
    if (cached) {
        const uint64_t w = s_cache[dev].load(std::memory_order_relaxed);
        if ((w & 0xFFFFFFu) != 0 && (w & ~(uint64_t)0xFFFFFFu) == key) { *out = (int)(w & 0xFFFFFFu); return hipSuccess; }
    }
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, verify_kernel, threads, lds)) != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    if (cus < 1) cus = 1;
    *out = (int)std::min<int64_t>((int64_t)cus * per_cu, 0xFFFFFF);
    if (cached) s_cache[dev].store(key | (uint32_t)*out, std::memory_order_relaxed);
    return hipSuccess;
}

}  // namespace

hipError_t verify_assignment_launch(const VerifyCall& c, uint32_t* status, hipStream_t stream) {
    hipError_t e;
    if (c.summary) {
        if ((e = hipMemsetAsync(c.summary, 0, 16, stream)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(c.summary + 2, 0xFF, 16, stream)) != hipSuccess) return e;
    }
    if (c.n_topics <= 0) return hipSuccess;

    // the hints size the LDS request and nothing else; without a usable one the request is the limit's
    const auto cap_of = [](int64_t hint, int64_t limit) { return hint <= 0 || hint > limit ? limit : hint; };
    VerifyArgs a{};
    a.c = c;
    a.status = status;
    a.cap_p = (int32_t)cap_of(c.max_partitions_per_topic, kVerifyMaxPartitions);
    a.cap_c = (int32_t)cap_of(c.max_consumers_per_topic, kVerifyMaxConsumers);
    const VerifyLayout l = layout_for(a.cap_p, a.cap_c);
    a.off_lag = l.off_lag;
    a.off_rank = l.off_rank;
    a.off_slot = l.off_slot;
    a.off_kidx = l.off_kidx;
    a.off_bits = l.off_bits;
    const int threads = a.cap_p <= kVerifyFewPartitions ? kVerifyFewThreads : kVerifyThreads;
    static PerDeviceOnce lds_opt_in;
    if ((e = lds_opt_in.run([] {
             return hipFuncSetAttribute((const void*)verify_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)kVerifyMaxLdsBytes);
         })) != hipSuccess)
        return e;
    int resident = 0;
    if ((e = verify_resident(threads, l.bytes, &resident)) != hipSuccess) return e;
    const dim3 grid((unsigned)std::min<int64_t>(c.n_topics, resident)), block((unsigned)threads);
    LA_LAUNCH(verify_kernel, grid, block, l.bytes, stream, a);
    return hipGetLastError();
}

}  // namespace la
