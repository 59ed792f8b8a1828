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
//
// GLOBAL FORM (LA_FLAG_VERIFY_LARGE): topics of more than kVerifyMaxPartitions partitions or kVerifyMaxConsumers consumers, listed
// by the host from h_part_off / h_cons_off (VerifyBig, a pinned list one copy brings over), all of a call side by side.  The
// same regions live in device memory -- table, lag[P], kidx[P] (64 bits: any consumer count), slot[rounds x C] of 32 bits,
// before[P], tot_last[C], the chunk sums, one word of verdict bits per topic -- and the same phases are launches; the ONLY
// grid-wide order is the launch boundary (no grid barrier, no spin, no cooperative launch).  Workgroup steps are numbered
// through the topics per domain (partitions, consumers, (chunk, consumer) pairs); a workgroup bisects the list for its step.
//   memsets  table = 0, slot = none, bits = 0
//   G0  insert the input ids (duplicate: UNCHECKED) | neighbouring ranks | the host's offsets against the device's (a mismatch:
//       UNCHECKED + kStatusShape; everything below works from the HOST's offsets, validated on the host, whatever the device's say)
//   G1  look every output id up, lag[i], bisect the owner in the topic's cons_rank segment, slot[round x C + k] = i, kidx[i] = k
//   G2  neighbours' order, the slot read back | per (chunk of ~sqrt(rounds) rounds, consumer): the sum of lag[slot]
//   G3  per consumer: exclusive scan over its chunk sums (in place), the final total against out_total_lag (V4)
//   G4  per (chunk, consumer): walk the chunk's rounds from the scanned sum -> before[i], tot_last[k]
//   G5  (before, rank) of neighbours in a round | the consumers a partial last round left out
// The totals are wrapping unsigned 64-bit sums, so the two-level association gives the reference's bits; no thread walks more
// than ~sqrt(rounds) entries.  The LDS kernel runs LAST and is the one place a verdict is stored and counted: for a topic of
// the list it records the bits the global form left, for an over-limit topic that is NOT in the list (the device's offsets
// disagree with the host's) UNCHECKED + kStatusShape -- every topic exactly once.
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

struct VerifyBig {              // one topic of the global form; every offset and size is the HOST's, inside [0, N] / [0, K]
    int64_t p0, np, c0, nc;
    int64_t wp, wc;             // what is verified: np, nc -- or 0, 0 for a topic the join cannot hold (skip: UNCHECKED)
    int64_t rounds, chunk_rounds, n_chunks;      // ceil(wp / wc) rounds in n_chunks chunks of chunk_rounds ~ sqrt(rounds)
    int64_t table0, part0, slot0, cons0, sum0;   // its regions: table slots, lag / kidx / before, slot, tot_last, chunk sums
    int64_t step0[3];           // first workgroup step per domain (kDomPart / kDomCons / kDomPair), numbered through the topics
    int32_t topic, bits;        // the table region has 1 << bits slots
    int32_t skip, pad_;
};

struct VerifyWork {             // the global form's device memory
    uint64_t* table;
    int64_t *lag, *kidx, *before, *tot_last;
    uint32_t* slot;
    uint64_t* sums;
    uint32_t* bits;             // [n_big] verdict bits, OR-ed with agent-scope atomics only when non-zero
    const VerifyBig* big;       // ascending in topic
    int32_t n_big;
    int64_t steps[3];           // workgroup steps per domain
};

struct VerifyArgs {
    VerifyCall c;
    uint32_t* status;
    VerifyWork g;               // n_big == 0: no topic went through the global form
    int32_t large;              // LA_FLAG_VERIFY_LARGE: an over-limit topic outside the list is a shape error
    int32_t cap_p, cap_c;       // partitions / consumers of a topic the LDS request holds
    uint32_t off_lag, off_rank, off_slot, off_kidx, off_bits;      // byte offsets of the regions behind A
};

struct VerifyLayout {
    uint32_t off_lag, off_rank, off_slot, off_kidx, off_bits;
    size_t bytes;
};

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
        if (a.g.n_big > 0) {                        // a topic of the host's list: the global form has left its bits
            int lo = 0, hi = a.g.n_big;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)a.g.big[mid].topic <= t) lo = mid;
                else hi = mid;
            }
            if ((int64_t)a.g.big[lo].topic == t) {
                if (tid == 0) record(c, tally, t, a.g.bits[lo]);
                continue;
            }
        }
        if (outside || over_limit || over_hint) {   // nothing is read through such offsets
            if (outside || over_hint || (over_limit && a.large)) bad |= kStatusShape;      // (the host's list would have held it)
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

// ---- the global form -----------------------------------------------------------------------------------------------------------
constexpr int kVgThreads = 256;
constexpr int kVgPer = 4;                           // partitions / consumers of a thread per workgroup step
constexpr int64_t kVgStep = (int64_t)kVgPer * kVgThreads;
constexpr int64_t kVgPairStep = kVgThreads;         // (chunk, consumer) pairs of a step: one per thread, each walks a chunk's rounds
constexpr uint32_t kNoPos = 0xFFFFFFFFu;            // slot: nobody (what the memset leaves)
constexpr int kDomPart = 0, kDomCons = 1, kDomPair = 2;
static_assert(kVerifyGlobalMaxPartitions < (int64_t)kNoPos, "32-bit positions inside a topic");

struct VerifyGlobalArgs {
    VerifyCall c;
    uint32_t* status;
    VerifyWork g;
};

__device__ __forceinline__ int big_of_step(const VerifyWork& g, int dom, int64_t step) {      // the last topic that starts at or before it
    int lo = 0, hi = g.n_big;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g.big[mid].step0[dom] <= step) lo = mid;
        else hi = mid;
    }
    return lo;
}

// G0 .. G5 of the file comment.  A step belongs to ONE topic, so its threads' bits are OR-ed per wavefront into that topic's word.
template <int PHASE>
__global__ __launch_bounds__(kVgThreads) void verify_global_kernel(VerifyGlobalArgs a) {
    constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
    constexpr int kDomA = PHASE == 3 ? kDomCons : (PHASE == 4 ? kDomPair : kDomPart);      // the launch's first domain ...
    constexpr int kDomB = PHASE == 0 || PHASE == 5 ? kDomCons : (PHASE == 2 ? kDomPair : -1);      // ... and its second, if any
    const VerifyCall& c = a.c;
    const VerifyWork& g = a.g;
    const int tid = (int)threadIdx.x;
    const int64_t steps_a = g.steps[kDomA], n_steps = steps_a + (kDomB >= 0 ? g.steps[kDomB >= 0 ? kDomB : kDomA] : 0);
    uint32_t bad = 0;
    for (int64_t step = blockIdx.x; step < n_steps; step += gridDim.x) {
        const int dom = step < steps_a ? kDomA : kDomB;                        // workgroup-uniform, as all that follows from it
        const int idx = big_of_step(g, dom, step < steps_a ? step : step - steps_a);
        const VerifyBig b = g.big[idx];
        const int64_t s = (step < steps_a ? step : step - steps_a) - b.step0[dom];
        const int64_t P = b.wp, C = b.wc;
        uint64_t* table = g.table + b.table0;
        int64_t* lag = g.lag + b.part0;
        int64_t* kidx = g.kidx + b.part0;
        int64_t* before = g.before + b.part0;
        uint32_t* slot = g.slot + b.slot0;
        int64_t* tot_last = g.tot_last + b.cons0;
        uint64_t* sums = g.sums + b.sum0;
        const int32_t* rank = c.cons_rank + b.c0;
        uint32_t v = 0;

        if (dom == kDomPart) {
            if (PHASE == 0 && s == 0 && tid == 0) {
                if (b.skip) v |= kVerdictUnchecked;
                if (c.part_off[b.topic] != b.p0 || c.part_off[b.topic + 1] != b.p0 + b.np || c.cons_off[b.topic] != b.c0 ||
                    c.cons_off[b.topic + 1] != b.c0 + b.nc) {
                    v |= kVerdictUnchecked;
                    bad |= kStatusShape;
                }
            }
#pragma unroll
            for (int u = 0; u < kVgPer; ++u) {
                const int64_t i = s * kVgStep + u * kVgThreads + tid;
                if (i >= P) continue;
                if (PHASE == 0) {
                    const uint32_t st = table_insert<kScope>(table, b.bits, c.pid[b.p0 + i], (int32_t)i);
                    if (st) v |= kVerdictUnchecked;
                    bad |= st & kStatusInternal;
                } else if (PHASE == 1) {
                    int32_t j = 0;
                    const uint32_t st = table_lookup<kScope>(table, b.bits, c.out_pid[b.p0 + i], &j);
                    int64_t l = 0;
                    if (st) {
                        v |= kVerdictIds;
                        bad |= st & kStatusInternal;
                    } else if (j >= 0 && (int64_t)j < P) {      // (the payload this topic's insert stored)
                        l = lag_of(c, b.p0 + j);
                    } else {
                        v |= kVerdictIds;
                        bad |= kStatusInternal;
                    }
                    lag[i] = l;
                    const int32_t r = c.out_rank[b.p0 + i];
                    int64_t k = -1;
                    if (C == 0) {
                        if (r != -1) v |= kVerdictOwner;
                    } else {
                        int64_t lo = 0, hi = C;     // first k with rank[k] >= r; the interval shrinks whatever the ranks hold
                        while (lo < hi) {
                            const int64_t mid = lo + ((hi - lo) >> 1);
                            if (rank[mid] < r) lo = mid + 1;
                            else hi = mid;
                        }
                        if (lo < C && rank[lo] == r) {
                            k = lo;
                            slot[(i / C) * C + lo] = (uint32_t)i;
                        } else {
                            v |= kVerdictOwner;
                        }
                    }
                    kidx[i] = k;
                } else if (PHASE == 2) {
                    if (i + 1 < P) {
                        const int64_t l0 = lag[i], l1 = lag[i + 1];
                        if (!(l0 > l1) && (l0 != l1 || !(c.out_pid[b.p0 + i] < c.out_pid[b.p0 + i + 1]))) v |= kVerdictOrder;
                    }
                    const int64_t k = kidx[i];
                    if (k >= 0 && k < C && slot[(i / C) * C + k] != (uint32_t)i) v |= kVerdictOwner;
                } else if (PHASE == 5) {
                    if (C == 0 || i + 1 >= P || (i + 1) % C == 0) continue;      // i closes its round
                    if (kidx[i] < 0 || kidx[i + 1] < 0) continue;
                    const int64_t b0 = before[i], b1 = before[i + 1];
                    // (an owner that was found IS its consumer's rank)
                    if (!(b0 < b1 || (b0 == b1 && c.out_rank[b.p0 + i] < c.out_rank[b.p0 + i + 1]))) v |= kVerdictGreedy;
                }
            }
        } else if (dom == kDomCons) {
            int64_t k_last = -1, b_last = 0;
            int32_t r_last = 0;
            if (PHASE == 5 && C > 0 && P % C != 0) {                            // (P > 0 then)
                k_last = kidx[P - 1];
                if (k_last >= 0 && k_last < C) {
                    b_last = before[P - 1];
                    r_last = rank[k_last];
                } else {
                    k_last = -1;
                }
            }
#pragma unroll
            for (int u = 0; u < kVgPer; ++u) {
                const int64_t k = s * kVgStep + u * kVgThreads + tid;
                if (k >= C) continue;
                if (PHASE == 0) {
                    if (k + 1 < C && !(rank[k] < rank[k + 1])) v |= kVerdictUnchecked;
                } else if (PHASE == 3) {
                    uint64_t run = 0;
                    for (int64_t ch = 0; ch < b.n_chunks; ++ch) {
                        const uint64_t x = sums[ch * C + k];
                        sums[ch * C + k] = run;
                        run += x;
                    }
                    if (c.out_total && c.out_total[b.c0 + k] != (int64_t)run) v |= kVerdictTotals;
                } else if (PHASE == 5) {
                    if (k_last < 0 || slot[(b.rounds - 1) * C + k] != kNoPos) continue;
                    const int64_t t0 = tot_last[k];
                    if (!(t0 > b_last || (t0 == b_last && rank[k] > r_last))) v |= kVerdictGreedy;
                }
            }
        } else {                                    // kDomPair: PHASE 2 sums a chunk, PHASE 4 walks it from the scanned sum
            const int64_t q = s * kVgPairStep + tid;
            if (q < b.n_chunks * C) {
                const int64_t ch = q / C, k = q - ch * C;
                const int64_t r0 = ch * b.chunk_rounds, r1 = r0 + b.chunk_rounds < b.rounds ? r0 + b.chunk_rounds : b.rounds;
                uint64_t tot = PHASE == 4 ? sums[q] : 0;
                for (int64_t r = r0; r < r1; ++r) {
                    if (PHASE == 4 && r == b.rounds - 1) tot_last[k] = (int64_t)tot;
                    const uint32_t i = slot[r * C + k];
                    if (i == kNoPos || (int64_t)i >= P) continue;               // (only positions of this topic are ever stored)
                    if (PHASE == 4) before[i] = (int64_t)tot;
                    tot += (uint64_t)lag[i];
                }
                if (PHASE == 2) sums[q] = tot;
            }
        }

        v = wave_or_u32(v);
        if ((tid & (kWave - 1)) == 0 && v) __hip_atomic_fetch_or(g.bits + idx, v, __ATOMIC_RELAXED, kScope);
    }
    if (bad) atomicOr(a.status, bad);
}

// a phase of the global form: a grid of 8 workgroups per compute unit walks its steps (a phase without steps launches nothing)
template <int PHASE>
hipError_t verify_global_launch(const VerifyGlobalArgs& a, int64_t steps, int cus, hipStream_t stream) {
    return launch_grid<verify_global_kernel<PHASE>>(std::min<int64_t>(steps, (int64_t)cus * 8), kVgThreads, 0, stream, a);
}

// Lists the topics over the LDS limit from the host's offsets, takes their working memory and enqueues the global form.
// Nothing is enqueued before every buffer is there.  n_big == 0 on return: the batch holds no such topic (nothing was touched).
hipError_t verify_global_form(VerifyScratch& s, const VerifyCall& c, const int64_t* h_part_off, const int64_t* h_cons_off,
                              uint32_t* status, hipStream_t stream, VerifyWork* out) {
    hipError_t e;
    const int64_t T = c.n_topics;
    const auto is_big = [&](int64_t t) {
        return h_part_off[t + 1] - h_part_off[t] > kVerifyMaxPartitions || h_cons_off[t + 1] - h_cons_off[t] > kVerifyMaxConsumers;
    };
    int64_t n_big = 0;
    for (int64_t t = 0; t < T; ++t) n_big += is_big(t) ? 1 : 0;
    *out = VerifyWork{};
    if (n_big == 0) return hipSuccess;

    size_t item_bytes = 0;
    if (!mul_ok((size_t)n_big, sizeof(VerifyBig), &item_bytes)) return hipErrorOutOfMemory;
    if ((e = s.list.reserve(item_bytes)) != hipSuccess) return e;

    // regions, counted in elements; every sum is checked (a count that does not fit cannot be allocated either)
    VerifyBig* items = static_cast<VerifyBig*>(s.list.h);
    size_t n_table = 0, n_part = 0, n_slot = 0, n_cons = 0, n_sum = 0;
    int64_t steps[3] = {0, 0, 0};
    int64_t j = 0;
    bool fits = true;
    for (int64_t t = 0; t < T; ++t) {
        if (!is_big(t)) continue;
        VerifyBig& b = items[j++];
        b = VerifyBig{};
        b.topic = (int32_t)t;
        b.p0 = h_part_off[t];
        b.np = h_part_off[t + 1] - b.p0;
        b.c0 = h_cons_off[t];
        b.nc = h_cons_off[t + 1] - b.c0;
        b.skip = b.np > kVerifyGlobalMaxPartitions ? 1 : 0;
        b.wp = b.skip ? 0 : b.np;
        b.wc = b.skip ? 0 : b.nc;
        b.rounds = b.wc > 0 ? (b.wp + b.wc - 1) / b.wc : 0;
        b.chunk_rounds = ceil_sqrt(b.rounds);
        b.n_chunks = (b.rounds + b.chunk_rounds - 1) / b.chunk_rounds;
        b.bits = ceil_log2(2 * b.wp);
        b.table0 = (int64_t)n_table;
        b.part0 = (int64_t)n_part;
        b.slot0 = (int64_t)n_slot;
        b.cons0 = (int64_t)n_cons;
        b.sum0 = (int64_t)n_sum;
        size_t slots = 0, pairs = 0;                // rounds x C < P + C; chunks x C
        fits = fits && mul_ok((size_t)b.rounds, (size_t)b.wc, &slots) && mul_ok((size_t)b.n_chunks, (size_t)b.wc, &pairs) &&
               add_ok(n_table, (size_t)1 << b.bits, &n_table) && add_ok(n_part, (size_t)b.wp, &n_part) &&
               add_ok(n_slot, slots, &n_slot) && add_ok(n_cons, (size_t)b.wc, &n_cons) && add_ok(n_sum, pairs, &n_sum);
        if (!fits) return hipErrorOutOfMemory;
        b.step0[kDomPart] = steps[kDomPart];
        b.step0[kDomCons] = steps[kDomCons];
        b.step0[kDomPair] = steps[kDomPair];
        steps[kDomPart] += std::max<int64_t>(1, (b.wp + kVgStep - 1) / kVgStep);      // (one at least: the offsets are compared there)
        steps[kDomCons] += (b.wc + kVgStep - 1) / kVgStep;
        steps[kDomPair] += ((int64_t)pairs + kVgPairStep - 1) / kVgPairStep;
    }
    // [table | lag | kidx | before | tot_last | sums : 8-byte words][slot | bits : 4-byte words]
    size_t words8 = 0, words4 = 0, bytes8 = 0, bytes4 = 0, bytes = 0, three = 0;
    fits = mul_ok(n_part, 3, &three) && add_ok(n_table, three, &words8) && add_ok(words8, n_cons, &words8) &&
           add_ok(words8, n_sum, &words8) && add_ok(n_slot, (size_t)n_big, &words4) && mul_ok(words8, 8, &bytes8) &&
           mul_ok(words4, 4, &bytes4) && add_ok(bytes8, bytes4, &bytes);
    if (!fits) return hipErrorOutOfMemory;
    if ((e = grow_device(&s.work, &s.work_cap, bytes)) != hipSuccess) return e;
    int cus = 0;
    if ((e = device_cus(&cus)) != hipSuccess) return e;

    VerifyWork g{};
    g.table = static_cast<uint64_t*>(s.work);
    g.lag = reinterpret_cast<int64_t*>(g.table + n_table);
    g.kidx = g.lag + n_part;
    g.before = g.kidx + n_part;
    g.tot_last = g.before + n_part;
    g.sums = reinterpret_cast<uint64_t*>(g.tot_last + n_cons);
    g.slot = reinterpret_cast<uint32_t*>(g.sums + n_sum);
    g.bits = g.slot + n_slot;
    g.big = static_cast<const VerifyBig*>(s.list.d);
    g.n_big = (int32_t)std::min<int64_t>(n_big, 0x7FFFFFFF);      // (T is 32 bits wide)
    for (int d = 0; d < 3; ++d) g.steps[d] = steps[d];

    if ((e = s.list.upload(item_bytes, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(g.table, 0, n_table * 8, stream)) != hipSuccess) return e;
    if (n_slot && (e = hipMemsetAsync(g.slot, 0xFF, n_slot * 4, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(g.bits, 0, (size_t)n_big * 4, stream)) != hipSuccess) return e;

    VerifyGlobalArgs a{};
    a.c = c;
    a.status = status;
    a.g = g;
    if ((e = verify_global_launch<0>(a, steps[kDomPart] + steps[kDomCons], cus, stream)) != hipSuccess) return e;
    if ((e = verify_global_launch<1>(a, steps[kDomPart], cus, stream)) != hipSuccess) return e;
    if ((e = verify_global_launch<2>(a, steps[kDomPart] + steps[kDomPair], cus, stream)) != hipSuccess) return e;
    if ((e = verify_global_launch<3>(a, steps[kDomCons], cus, stream)) != hipSuccess) return e;
    if ((e = verify_global_launch<4>(a, steps[kDomPair], cus, stream)) != hipSuccess) return e;
    if ((e = verify_global_launch<5>(a, steps[kDomPart] + steps[kDomCons], cus, stream)) != hipSuccess) return e;
    *out = g;
    return hipSuccess;
}

}  // namespace

void verify_scratch_release(VerifyScratch& s) {
    s.list.release();
    if (s.work) (void)hipFree(s.work);
    s = VerifyScratch{};
}

hipError_t verify_assignment_launch(VerifyScratch* large, const VerifyCall& c, const int64_t* h_part_off,
                                    const int64_t* h_cons_off, uint32_t* status, hipStream_t stream) {
    hipError_t e;
    VerifyWork g{};
    // the global form first: the LDS kernel behind it stores and counts the verdicts of its topics too
    if (large && c.n_topics > 0 && (e = verify_global_form(*large, c, h_part_off, h_cons_off, status, stream, &g)) != hipSuccess)
        return e;
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
    a.g = g;
    a.large = large ? 1 : 0;
    a.cap_p = (int32_t)cap_of(c.max_partitions_per_topic, kVerifyMaxPartitions);
    a.cap_c = (int32_t)cap_of(c.max_consumers_per_topic, kVerifyMaxConsumers);
    const VerifyLayout l = layout_for(a.cap_p, a.cap_c);
    a.off_lag = l.off_lag;
    a.off_rank = l.off_rank;
    a.off_slot = l.off_slot;
    a.off_kidx = l.off_kidx;
    a.off_bits = l.off_bits;
    const int threads = a.cap_p <= kVerifyFewPartitions ? kVerifyFewThreads : kVerifyThreads;
    return launch_resident_lds<verify_kernel, kVerifyMaxLdsBytes>(c.n_topics, threads, l.bytes, stream, a);
}

}  // namespace la
