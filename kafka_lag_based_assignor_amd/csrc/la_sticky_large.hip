// la_sticky_large.hip -- sticky ties for topics of any size: the GLOBAL FORM of la_sticky.hip's re-matching (LA_FLAG_STICKY_LARGE).
//
// Topics of more than kVerifyMaxPartitions partitions, listed by the host from h_part_off (StickyBig, a pinned list one copy
// brings over), all of a call side by side.  Their positions are numbered through the topics: q = q0 of the topic + i, L in all.
// The phases of the LDS kernel are launches over regions in device memory; the ONLY grid-wide order the kernels here introduce is
// the launch boundary (no grid barrier, no spin, no cooperative launch -- the radix passes are la_radix.hip's as they are).
// Workgroup steps of kStickyStep positions are numbered through the topics, so a step lies inside ONE topic; a workgroup bisects
// the list for its step.  A step is also the CHUNK of the two device-wide scans.
//   memsets  table = 0, counters = 0, src_of = nobody, placed = 0, the sort's control words = 0
//   K0  insert the topic's input ids, payload = the input's index (a duplicate: the topic is BAD)
//   K1  look every output id up (a miss or a second hit: BAD), lag[q] through lag_of; count kept before
//   K2  run heads: q + 1 where lag[q] != lag[q - 1] OR q is its topic's first position, else 0; the maximum of every chunk
//   K3  exclusive max-scan over the chunk maxima (one workgroup; a topic's first position is a head, so no value crosses a topic)
//   K4  run start of every position = max(scanned chunk value, the heads before it in its chunk); the sort keys
//           key64 = run start << 32 | member << 1 | (0: the position's owner, S; 1: its partition's previous owner, W)
//       for q's two elements 2 q and 2 q + 1, val32 = the element's own index -- ascending, so the id passes are skipped; an owner
//       or previous owner below 0 gets the run field L, beyond every run start.  Run starts are < L < 2^30 and a member is 31
//       bits: the top bit stays free and no key is all ones.  The digit histograms of the 8 key digits.
//   sort    sort_plan_and_passes over the digits that can differ: 4 member digits, the run-start digits L leaves possible.  The
//       stable LSD passes leave every (run, member) group as its S elements, positions ascending, then its W elements likewise
//   K5  every W element bisects the start of its group and of the group's W half: the k-th W entry takes the k-th S entry when
//       k < |S| -> src_of[S position] = W position, placed[W position] = 1
//   K6  per chunk: partitions not placed, positions not filled
//   K7  exclusive scan over both chunk counts (one workgroup), the two totals
//   K8  loose[rank] = q of every partition not placed, hole_rank[q] of every position not filled
//   K9  sticky[d] = out_partition[src_of[d], or loose[hole_rank[d]]]; kept after, the changed flag, per topic
// WHY THE SCAN PAIRING IS SOUND: K5 pairs inside a (run, member) group only, so in every run as many partitions are placed as
// positions are filled, whatever the data (a BAD topic included: its lags are whatever the join found, its runs are runs all the
// same).  Left over are equally many of both in every run; the exclusive counts of both therefore agree at every run start, and
// the k-th loose partition of the WHOLE list lies in the run of the k-th hole: ranks by one scan over all topics pair leftovers
// ascending into holes ascending inside each run, rule 4 of lagassign.h.  K9 still checks that the totals agree and that a source
// lies inside the topic of its destination; otherwise kStatusInternal and the identity.
// The LDS kernel (la_sticky.hip) runs LAST and is the one place where d_topic_kept / d_topic_saved are stored and the summary is
// added to: for a topic of the list from the counters left here.  A BAD topic is copied by K9 and counts as passed through.
// Safe on any content: an index comes from the join's payload, a bisection, a scan or the sort's payload -- each compared against
// its range before use -- never from an id or a rank.  Every loop is bounded; accesses are one element wide; every pointer is a
// kernel argument or an offset from one.
//
// WORKING MEMORY (StickyScratch, the shard's own, grown before anything is enqueued), bytes per large-topic partition:
//   table 16 .. 32 (2^ceil(log2(2 P)) slots of 8) | lag 8 | placed, src_of, hole_rank, loose 4 each | the sort's two elements:
//   2 x (2 keys of 8 + 2 payloads of 4) = 48, and its look-back granules, 2 KiB per tile of >= 4 096 elements: <= 1
//   => 89 .. 105 bytes, + 12 per chunk of 1 024 positions and 32 per topic.
#include <algorithm>

#include "la_kernels.h"
#include "la_device.h"
#include "la_join.h"
#include "la_radix.h"
#include "la_sticky_match.h"

namespace la {

namespace {

constexpr int kSgThreads = 256;
constexpr int kSgPer = 4;                           // positions of a thread per workgroup step
constexpr int64_t kStickyStep = (int64_t)kSgPer * kSgThreads;
constexpr int kSgScanThreads = 1024;                // the one workgroup of K3 / K7
constexpr uint32_t kNobody = 0xFFFFFFFFu;           // src_of: nobody (what the memset leaves)
constexpr int kKeyRunBit = 32;
static_assert(kStickyGlobalMaxTotal < ((int64_t)1 << 30), "a run start | the run field of no member stay below bit 63; 2 L sort elements in 31 bits");
static_assert(kStickyGlobalMaxPartitions <= kStickyGlobalMaxTotal, "one topic of the largest size fits a call");
static_assert(kStickyStep * 2 < 65536, "a chunk's two counts in one word");
static_assert(kSgThreads / kWave <= 4 && kSgScanThreads / kWave <= 16, "wave totals of a scan");

struct StickyGlobalArgs {
    StickyCall c;
    uint32_t* status;
    StickyWork g;
    SortBufs b;
    uint32_t pass_mask;
};

__device__ __forceinline__ int big_of_step(const StickyWork& g, int64_t step) {      // the last topic that starts at or before it
    int lo = 0, hi = g.n_big;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g.big[mid].step0 <= step) lo = mid;
        else hi = mid;
    }
    return lo;
}

// first index in [lo, hi) whose key is not below x (hi when there is none); the interval shrinks whatever the keys hold
__device__ __forceinline__ int64_t first_not_below64(const uint64_t* keys, int64_t lo, int64_t hi, uint64_t x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// K0, K1, K2, K4, K6, K8, K9 of the file comment (PHASE = the K number).  K2, K4, K6 and K8 scan: a thread takes kSgPer CONSECUTIVE
// positions, so that a scan over the threads is a scan over the positions; the others take positions a workgroup width apart.
template <int PHASE>
__global__ __launch_bounds__(kSgThreads) void sticky_global_kernel(StickyGlobalArgs a) {
    constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
    constexpr bool kBlocked = PHASE == 2 || PHASE == 4 || PHASE == 6 || PHASE == 8;
    __shared__ uint32_t wave_tot[kSgThreads / kWave];
    __shared__ uint32_t hist[PHASE == 4 ? 8 * kRadix : 1];
    const StickyCall& c = a.c;
    const StickyWork& g = a.g;
    const int tid = (int)threadIdx.x;
    const int64_t L = g.n_pos;
    uint32_t bad = 0;
    if (PHASE == 4) {
        for (int i = tid; i < 8 * kRadix; i += kSgThreads) hist[i] = 0;
        __syncthreads();
    }
    bool sound = true;
    uint64_t n_loose = 0;
    if (PHASE == 9) {
        n_loose = g.tot[0];
        sound = n_loose == g.tot[1];                // as many left over as places left
        if (!sound) bad |= kStatusInternal;
    }
    for (int64_t step = blockIdx.x; step < g.n_steps; step += gridDim.x) {
        const int idx = big_of_step(g, step);       // workgroup-uniform, as all that follows from it
        const StickyBig b = g.big[idx];
        const int64_t s = step - b.step0;
        const int64_t P = b.np;
        uint64_t* table = g.table + b.table0;
        uint32_t f = 0, n_kept = 0;
        uint32_t head[kSgPer] = {}, mine = 0;       // K2 / K4: q + 1 of a head, else 0; K6 / K8: not placed | not filled << 16
        bool topic_bad = false;
        if (PHASE == 9) topic_bad = (__hip_atomic_load(g.ctr + 4 * idx + 2, __ATOMIC_RELAXED, kScope) & kStickyBigBad) != 0;

#pragma unroll
        for (int u = 0; u < kSgPer; ++u) {
            const int64_t i = s * kStickyStep + (kBlocked ? (int64_t)tid * kSgPer + u : (int64_t)u * kSgThreads + tid);
            if (i >= P) continue;
            const int64_t q = b.q0 + i;
            if (PHASE == 0) {
                const uint32_t st = table_insert<kScope>(table, b.bits, c.pid[b.p0 + i], (int32_t)i);
                if (st) f |= kStickyBigBad;
                bad |= st & kStatusInternal;
            } else if (PHASE == 1) {
                int32_t j = 0;
                const uint32_t st = table_lookup<kScope>(table, b.bits, c.out_pid[b.p0 + i], &j);
                int64_t l = 0;
                if (st) {
                    f |= kStickyBigBad;
                    bad |= st & kStatusInternal;
                } else if (j >= 0 && (int64_t)j < P) {      // (the payload this topic's insert stored)
                    l = lag_of(c, b.p0 + j);
                } else {
                    f |= kStickyBigBad;
                    bad |= kStatusInternal;
                }
                g.lag[q] = l;
                const int32_t ci = c.out_rank[b.p0 + i];
                n_kept += (ci >= 0 && c.prev_owner[b.p0 + i] == ci) ? 1 : 0;
            } else if (PHASE == 2 || PHASE == 4) {
                head[u] = (i == 0 || g.lag[q] != g.lag[q - 1]) ? (uint32_t)q + 1 : 0u;
                mine = head[u] > mine ? head[u] : mine;
            } else if (PHASE == 6 || PHASE == 8) {
                head[u] = (g.placed[q] ? 0u : 1u) + (g.src_of[q] == kNobody ? 1u << 16 : 0u);
                mine += head[u];
            } else {                                // K9
                int64_t src = g.src_of[q];
                if (src == (int64_t)kNobody) {
                    const uint32_t r = g.hole_rank[q];
                    src = (uint64_t)r < n_loose && (int64_t)r < L ? (int64_t)g.loose[r] : -1;
                }
                if (sound && !topic_bad && (src < b.q0 || src >= b.q0 + P)) {      // (never expected: a source of another topic)
                    bad |= kStatusInternal;
                    src = q;
                }
                if (!sound || topic_bad) src = q;
                const int64_t j = src - b.q0;
                c.sticky[b.p0 + i] = c.out_pid[b.p0 + j];
                const int32_t qs = c.prev_owner[b.p0 + j];
                n_kept += (qs >= 0 && qs == c.out_rank[b.p0 + i]) ? 1 : 0;
                if (src != q) f |= kStickyBigChanged;
            }
        }

        if (PHASE == 0 || PHASE == 1 || PHASE == 9) {
            f = wave_or_u32(f);
            if (PHASE != 0) n_kept = wave_sum_u32(n_kept);
            if ((tid & (kWave - 1)) == 0) {
                if (f) __hip_atomic_fetch_or(g.ctr + 4 * idx + 2, (unsigned long long)f, __ATOMIC_RELAXED, kScope);
                if (n_kept) __hip_atomic_fetch_add(g.ctr + 4 * idx + (PHASE == 1 ? 0 : 1), (unsigned long long)n_kept, __ATOMIC_RELAXED, kScope);
            }
        } else if (PHASE == 2 || PHASE == 6) {
            uint32_t all = 0;
            (void)workgroup_excl_scan<PHASE == 2>(mine, wave_tot, tid, kSgThreads, &all);
            if (tid == 0) {
                if (PHASE == 2) {
                    g.cmax[step] = all;
                } else {
                    g.csum_loose[step] = all & 0xFFFFu;
                    g.csum_hole[step] = all >> 16;
                }
            }
        } else if (PHASE == 4) {
            uint32_t unused = 0;
            uint32_t run = workgroup_excl_scan<true>(mine, wave_tot, tid, kSgThreads, &unused);
            const uint32_t carry = g.cmax[step];    // (K3 has made it exclusive)
            run = carry > run ? carry : run;
#pragma unroll
            for (int u = 0; u < kSgPer; ++u) {
                const int64_t i = s * kStickyStep + (int64_t)tid * kSgPer + u;
                if (i >= P) continue;
                const int64_t q = b.q0 + i;
                if (head[u]) run = head[u];
                // (run >= 1 always: a topic's first position is a head; 0 would only send the element to run "L" below)
                const uint64_t start = run ? (uint64_t)(run - 1) : (uint64_t)L;
                const int32_t ci = c.out_rank[b.p0 + i], qi = c.prev_owner[b.p0 + i];
                const uint64_t nobody = (uint64_t)L << kKeyRunBit;
                const uint64_t ks = ci >= 0 ? (start << kKeyRunBit) | ((uint64_t)(uint32_t)ci << 1) : nobody;
                const uint64_t kw = qi >= 0 ? (start << kKeyRunBit) | ((uint64_t)(uint32_t)qi << 1) | 1u : nobody;
                a.b.key[0][2 * q] = ks;
                a.b.key[0][2 * q + 1] = kw;
                a.b.val[0][2 * q] = (uint32_t)(2 * q);
                a.b.val[0][2 * q + 1] = (uint32_t)(2 * q + 1);
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    if (!((a.pass_mask >> (4 + p)) & 1u)) continue;
                    atomicAdd(&hist[p * kRadix + ((uint32_t)(ks >> (8 * p)) & 0xFFu)], 1u);
                    atomicAdd(&hist[p * kRadix + ((uint32_t)(kw >> (8 * p)) & 0xFFu)], 1u);
                }
            }
        } else {                                    // K8
            uint32_t unused = 0;
            const uint32_t ranks = workgroup_excl_scan<false>(mine, wave_tot, tid, kSgThreads, &unused);
            uint64_t r_loose = (uint64_t)g.csum_loose[step] + (ranks & 0xFFFFu), r_hole = (uint64_t)g.csum_hole[step] + (ranks >> 16);
#pragma unroll
            for (int u = 0; u < kSgPer; ++u) {
                const int64_t i = s * kStickyStep + (int64_t)tid * kSgPer + u;
                if (i >= P) continue;
                const int64_t q = b.q0 + i;
                if (head[u] & 0xFFFFu) {
                    if (r_loose < (uint64_t)L) g.loose[r_loose] = (uint32_t)q;
                    ++r_loose;
                }
                if (head[u] >> 16) {
                    g.hole_rank[q] = r_hole < (uint64_t)L ? (uint32_t)r_hole : kNobody;
                    ++r_hole;
                }
            }
        }
    }
    if (PHASE == 4) {
        __syncthreads();
        for (int i = tid; i < 8 * kRadix; i += kSgThreads)
            if (hist[i]) atomicAdd(&a.b.hist[4 * kRadix + i], hist[i]);
        // digits the loop did not count: the payloads are ascending (skipped by the plan), the key bits outside the mask are zero
        if (blockIdx.x == 0 && tid < kDigits && (tid < 4 || !((a.pass_mask >> tid) & 1u))) a.b.hist[tid * kRadix] = (uint32_t)a.b.n;
    }
    if (bad) atomicOr(a.status, bad);
}

// K5: the sorted elements, one per thread.  The sort's result is checked on the way (as member_emit_kernel does).
__global__ __launch_bounds__(kSgThreads) void sticky_match_kernel(StickyGlobalArgs a) {
    const StickyWork& g = a.g;
    const uint32_t fin = a.b.ctl->cur[kFinal];
    const uint64_t* key = key_buf(a.b, fin);
    const uint32_t* val = val_buf(a.b, fin);
    const int64_t n = a.b.n, L = g.n_pos;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint32_t bad = 0;
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += stride) {
        const uint64_t kw = key[x];
        if (x > 0) {
            const uint64_t kp = key[x - 1];
            if (kp > kw || (kp == kw && val[x - 1] >= val[x])) bad |= kStatusOrder;
        }
        if ((kw >> kKeyRunBit) >= (uint64_t)L || !(kw & 1u)) continue;      // nobody's, or an S element
        const int64_t w0 = first_not_below64(key, 0, x, kw);                  // the group's W half starts here ...
        const int64_t s0 = first_not_below64(key, 0, w0, kw & ~1ull);        // ... and its S half here
        const int64_t k = x - w0;
        if (k < w0 - s0) {
            const int64_t src = (int64_t)(val[x] >> 1), dst = (int64_t)(val[s0 + k] >> 1);
            if (src < L && dst < L) {               // (positions K4 put into the payloads)
                g.src_of[dst] = (uint32_t)src;
                g.placed[src] = 1;
            }
        }
    }
    if (bad) atomicOr(a.status, bad);
}

// K3 (MAX) / K7: exclusive scan over one word per chunk, in place, by ONE workgroup: a thread takes a contiguous share.
// K7 scans two arrays and leaves their totals in tot[0], tot[1].
template <bool MAX>
__global__ __launch_bounds__(kSgScanThreads) void sticky_chunk_scan_kernel(uint32_t* x, uint32_t* y, int64_t n, unsigned long long* tot) {
    __shared__ uint32_t wave_tot[kSgScanThreads / kWave];
    const int tid = (int)threadIdx.x;
    const int64_t per = (n + kSgScanThreads - 1) / kSgScanThreads;
    const int64_t i0 = (int64_t)tid * per < n ? (int64_t)tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    for (int w = 0; w < 2; ++w) {
        uint32_t* v = w == 0 ? x : y;
        if (!v) break;                              // (uniform)
        uint32_t agg = 0;
        for (int64_t i = i0; i < i1; ++i) agg = MAX ? (v[i] > agg ? v[i] : agg) : agg + v[i];
        uint32_t all = 0;
        uint32_t run = workgroup_excl_scan<MAX>(agg, wave_tot, tid, kSgScanThreads, &all);
        for (int64_t i = i0; i < i1; ++i) {
            const uint32_t e = v[i];
            v[i] = run;
            run = MAX ? (e > run ? e : run) : run + e;
        }
        if (tot && tid == 0) tot[w] = all;
    }
}

template <int PHASE>
hipError_t sticky_global_launch(const StickyGlobalArgs& a, int cus, hipStream_t stream) {
    return launch_grid<sticky_global_kernel<PHASE>>(std::min<int64_t>(a.g.n_steps, (int64_t)cus * 8), kSgThreads, 0, stream, a);
}

inline bool is_big(const int64_t* h_part_off, int64_t t) {
    const int64_t np = h_part_off[t + 1] - h_part_off[t];
    return np > kVerifyMaxPartitions && np <= kStickyGlobalMaxPartitions;
}

// the regions of s.work behind a reserve; false: the sizes do not fit size_t (cannot be allocated either)
struct StickyRegions {
    size_t o_lag, o_ctr, o_tot, o_placed, o_src, o_hole, o_loose, o_cmax, o_cl, o_ch, o_sort_zero, o_sort_data, bytes;
    SortLayout sort;
};

bool regions_for(const StickyScratch& s, StickyRegions* out) {
    StickyRegions r{};
    const size_t L = (size_t)s.n_pos, n_steps = (size_t)s.n_steps, n_big = (size_t)s.n_big;
    r.sort = sort_layout(2 * s.n_pos, false);
    size_t at = 0;
    bool ok = true;
    const auto take = [&](size_t count, size_t elem) {
        size_t bytes = 0;
        const size_t o = at;
        ok = ok && mul_ok(count, elem, &bytes) && add_ok(at, bytes, &at);
        return o;
    };
    (void)take(s.n_table, 8);                       // the table, at 0
    r.o_lag = take(L, 8);
    r.o_ctr = take(4 * n_big, 8);
    r.o_tot = take(2, 8);
    r.o_placed = take(L, 4);
    r.o_src = take(L, 4);
    r.o_hole = take(L, 4);
    r.o_loose = take(L, 4);
    r.o_cmax = take(n_steps, 4);
    r.o_cl = take(n_steps, 4);
    r.o_ch = take(n_steps, 4);
    at = align_up(at, 256);
    r.o_sort_zero = take(r.sort.zero_bytes, 1);
    r.o_sort_data = take(r.sort.data_bytes, 1);
    r.bytes = at;
    *out = r;
    return ok;
}

}  // namespace

void sticky_scratch_release(StickyScratch& s) {
    s.list.release();
    if (s.work) (void)hipFree(s.work);
    s = StickyScratch{};
}

hipError_t sticky_large_reserve(StickyScratch& s, const StickyCall& c, const int64_t* h_part_off) {
    hipError_t e;
    const int64_t T = c.n_topics;
    s.n_big = s.n_pos = s.n_steps = 0;
    s.n_table = 0;
    int64_t n_big = 0;
    for (int64_t t = 0; t < T; ++t) n_big += is_big(h_part_off, t) ? 1 : 0;
    if (n_big == 0) return hipSuccess;

    size_t item_bytes = 0;
    if (!mul_ok((size_t)n_big, sizeof(StickyBig), &item_bytes)) return hipErrorOutOfMemory;
    if ((e = s.list.reserve(item_bytes)) != hipSuccess) return e;
    StickyBig* items = static_cast<StickyBig*>(s.list.h);
    int64_t j = 0, n_pos = 0, n_steps = 0;
    size_t n_table = 0;
    for (int64_t t = 0; t < T; ++t) {
        if (!is_big(h_part_off, t)) continue;
        StickyBig& b = items[j++];
        b = StickyBig{};
        b.topic = (int32_t)t;
        b.p0 = h_part_off[t];
        b.np = h_part_off[t + 1] - b.p0;
        b.q0 = n_pos;
        b.bits = ceil_log2(2 * b.np);
        b.table0 = (int64_t)n_table;
        b.step0 = n_steps;
        n_pos += b.np;
        if (n_pos > kStickyGlobalMaxTotal || !add_ok(n_table, (size_t)1 << b.bits, &n_table)) return hipErrorOutOfMemory;
        n_steps += (b.np + kStickyStep - 1) / kStickyStep;
    }
    s.n_pos = n_pos;
    s.n_steps = n_steps;
    s.n_table = n_table;
    StickyRegions r{};
    if (!regions_for(s, &r)) return hipErrorOutOfMemory;
    if ((e = grow_device(&s.work, &s.work_cap, r.bytes)) != hipSuccess) return e;
    s.n_big = n_big;                                // (last: a failed reserve leaves "no large topic")
    return hipSuccess;
}

hipError_t sticky_large_enqueue(StickyScratch& s, const StickyCall& c, uint32_t* status, hipStream_t stream, StickyWork* out) {
    hipError_t e;
    *out = StickyWork{};
    if (s.n_big == 0) return hipSuccess;
    StickyRegions r{};
    if (!regions_for(s, &r) || r.bytes > s.work_cap) return hipErrorOutOfMemory;
    int cus = 0;
    if ((e = device_cus(&cus)) != hipSuccess) return e;
    char* const base = static_cast<char*>(s.work);
    const size_t L = (size_t)s.n_pos;

    StickyWork g{};
    g.table = reinterpret_cast<uint64_t*>(base);
    g.lag = reinterpret_cast<int64_t*>(base + r.o_lag);
    g.ctr = reinterpret_cast<unsigned long long*>(base + r.o_ctr);
    g.tot = reinterpret_cast<unsigned long long*>(base + r.o_tot);
    g.placed = reinterpret_cast<uint32_t*>(base + r.o_placed);
    g.src_of = reinterpret_cast<uint32_t*>(base + r.o_src);
    g.hole_rank = reinterpret_cast<uint32_t*>(base + r.o_hole);
    g.loose = reinterpret_cast<uint32_t*>(base + r.o_loose);
    g.cmax = reinterpret_cast<uint32_t*>(base + r.o_cmax);
    g.csum_loose = reinterpret_cast<uint32_t*>(base + r.o_cl);
    g.csum_hole = reinterpret_cast<uint32_t*>(base + r.o_ch);
    g.big = static_cast<const StickyBig*>(s.list.d);
    g.n_big = (int32_t)std::min<int64_t>(s.n_big, 0x7FFFFFFF);      // (T is 32 bits wide)
    g.n_pos = s.n_pos;
    g.n_steps = s.n_steps;

    StickyGlobalArgs a{};
    a.c = c;
    a.status = status;
    a.g = g;
    a.b = sort_bind(r.sort, base + r.o_sort_zero, base + r.o_sort_data);
    // the digits that can differ: the member | S/W word, and as much of a run start as L has bits
    a.pass_mask = 0xFu << 4;
    for (int d = 0; d < 4 && (s.n_pos >> (8 * d)) != 0; ++d) a.pass_mask |= 1u << (8 + d);

    if ((e = s.list.upload((size_t)s.n_big * sizeof(StickyBig), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(g.table, 0, s.n_table * 8, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(g.ctr, 0, ((size_t)4 * s.n_big + 2) * 8, stream)) != hipSuccess) return e;      // (ctr | tot)
    if ((e = hipMemsetAsync(g.placed, 0, L * 4, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(g.src_of, 0xFF, L * 4, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(base + r.o_sort_zero, 0, r.sort.zero_bytes, stream)) != hipSuccess) return e;

    if ((e = sticky_global_launch<0>(a, cus, stream)) != hipSuccess) return e;
    if ((e = sticky_global_launch<1>(a, cus, stream)) != hipSuccess) return e;
    if ((e = sticky_global_launch<2>(a, cus, stream)) != hipSuccess) return e;
    LA_LAUNCH(sticky_chunk_scan_kernel<true>, dim3(1), dim3(kSgScanThreads), 0, stream, g.cmax, (uint32_t*)nullptr, g.n_steps,
              (unsigned long long*)nullptr);
    if ((e = sticky_global_launch<4>(a, cus, stream)) != hipSuccess) return e;
    sort_plan_and_passes(sort_job_single(a.b, a.pass_mask, status), stream, nullptr);
    LA_LAUNCH(sticky_match_kernel, dim3(grid_256(a.b.n)), dim3(kSgThreads), 0, stream, a);
    if ((e = sticky_global_launch<6>(a, cus, stream)) != hipSuccess) return e;
    LA_LAUNCH(sticky_chunk_scan_kernel<false>, dim3(1), dim3(kSgScanThreads), 0, stream, g.csum_loose, g.csum_hole, g.n_steps, g.tot);
    if ((e = sticky_global_launch<8>(a, cus, stream)) != hipSuccess) return e;
    if ((e = sticky_global_launch<9>(a, cus, stream)) != hipSuccess) return e;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    *out = g;
    return hipSuccess;
}

}  // namespace la
