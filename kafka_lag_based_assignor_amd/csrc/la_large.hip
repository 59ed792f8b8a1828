// la_large.hip -- topics that do not fit one wave tile (> 1024 partitions or > 64 consumers): the greedy behind the device-wide
// radix sort of la_radix.hip.  Everything runs on the device, no host round trip between the launches of a call.  In file order:
//
//   ids and greedy    emit_ids_kernel writes the sorted ids and checks the order.  greedy_rounds_kernel: ONE workgroup per
//                     topic (the chain of rounds is serial), consumer bins in registers, each round orders the bins by
//                     (total lag, member) and hands the round's C partitions out in that order -- ceil(P/C) rounds instead
//                     of P argmins.  Packed 64-bit bins are ordered by a full sort (the workgroup network of la_sort64.h, or a
//                     sample sort), by merging a few ascending runs, or by sorting only the bins that moved; bins that do not pack
//                     keep the 96-bit form.  greedy_argmin_kernel (LA_ALGO_ARGMIN) is the literal form: bins in LDS, one
//                     argmin per partition.  map_ranks_kernel turns consumer indices into member ranks.
//   host: one topic   large_topic_launch: the sort (sort_launch, la_radix.h), ids, rounds.
//   host: a batch     large_topics_launch: several large topics in the same launches, a LargeItem each, one set of pass
//                     launches per tile class and one rounds launch per rounds class; a single topic takes the serial form.
//   huge path         huge_topic_launch, more than kLargeMaxConsumers consumers: bins in HBM, one radix sort of the bins and
//                     one huge_round_kernel per round.
//   read-outs         the lab builds' instrumentation arrays (la_debug_round_*), large_profile_read.
//
// No environment hook is read here: the sort's are la_radix.hip's and la_radix.h's, the grouping's la_group.hip's.
#include "la_radix.h"
#include "la_device.h"
#include "la_sort64.h"

#include <algorithm>
#include <vector>

namespace la {

namespace {

// The rounds kernel's lags as 32-bit words and its results as 16-bit consumer indices where they fit (rounds_io): from how many
// bins per thread on (8: more than 4 096 consumers; at 4 bins per thread it lost 3 %)
constexpr int kRoundsNarrowEc = 8;
// x (bins per thread of the round) = the most bins the wide form of the moved-bins sort is tried on (moved_sort_bins; 512 = all
// that fit)
constexpr int kWideMovedLimit = 512;

// ---- outputs that do not depend on the greedy ----------------------------------------------------
// It also CHECKS the sort: neighbours must be in (key, id) order.  Every LSD pass has to be stable, and the default ranking of a pass
// (one returning LDS atomic per element) is stable only because colliding lanes are served in lane order -- a property of
// the hardware checked once at la_create on an idle device, not a promise of the ISA.  A violation under load would scramble
// the order silently; here it raises kStatusOrder (LA_EHIP at the next sync) for 8 B more read per element.
// ---- what the rounds kernel reads and writes per round -------------------------------------------------------------------------
// greedy_rounds_kernel is ONE workgroup on one compute unit, and every round of a topic of C consumers used to pull C sorted 64-bit
// keys in and push C 32-bit consumer indices out through that unit's address path -- 96 KB per round at 8 192 consumers, in 16-byte
// pieces that each touch every cache line of a wavefront's stretch: measured with the stores left out and with half the loads
// (profiles/r06_am_rounds_memory.txt), 1.65 us of a 3.4 us round in which nothing else happens, ~0.2 ms of cfg5's 0.83.  The
// NARROW form: where the topic has more than 4 096 consumers, its bins pack and no lag needs more than 32 bits, emit_ids_kernel leaves the lags as 32-bit words in
// the sort's other key buffer and the rounds kernel leaves its results as 16-bit consumer indices in the sort's other value
// buffer -- both with every round's stretch starting on a multiple of 8 elements (stride `cpad`), so a thread's 8 lags are two
// aligned 16-byte loads, its 8 results ONE 16-byte store, and a wavefront's accesses are contiguous; map_ranks_kernel, which
// turns indices into member ranks on the whole chip anyway, reads the 16-bit form.  emit_ids_kernel, greedy_rounds_kernel and
// map_ranks_kernel each decide from the same sorted keys (the first carries the largest lag, the last the smallest).
__host__ __device__ inline void rounds_class(int64_t n_cons, int* ec, int* threads);
struct RoundsIo {
    int idx_bits;          // the bins pack into (total << idx_bits) | index; 0: they do not (96-bit bins)
    bool narrow;           // 32-bit lags in, 16-bit indices out, rounds `cpad` elements apart
    int64_t cpad;          // C rounded up to a multiple of 8
    bool zero_tail;        // the smallest lag is zero: the topic's last rounds may hand out zeros only (greedy_rounds_packed)
};
// only_narrow: the caller wants `narrow` alone (emit_ids_kernel, map_ranks_kernel) -- decided without a look at the keys where it can be
__device__ __forceinline__ RoundsIo rounds_io(const LargeArgs& a, const uint64_t* key, int64_t P, int64_t C, const bool only_narrow = false) {
    RoundsIo io{0, false, (C + 7) & ~(int64_t)7, false};
    if (P <= 0 || C <= 0) return io;
    int ec = 1, threads = 64;
    rounds_class(C, &ec, &threads);
    if (only_narrow && !(a.rounds_follow != 0 && ec >= kRoundsNarrowEc && P >= 8)) return io;   // (no key is read)
    const int n = ec * threads;
    const int64_t rounds = (P + C - 1) / C;
    const int64_t lmax = (int64_t)(key[0] ^ kLagKeyFlip), lmin = (int64_t)(key[P - 1] ^ kLagKeyFlip);
    const int idx_bits = 31 - __builtin_clz(n);                                  // n is a power of two
    const int lag_bits = lmax > 0 ? 64 - __builtin_clzll((unsigned long long)lmax) : 0;
    const int round_bits = 64 - __builtin_clzll((unsigned long long)rounds);
    if (lmin >= 0 && lag_bits + round_bits + idx_bits <= 62) io.idx_bits = idx_bits;
    io.zero_tail = lmin == 0;
    // (the last element written is P - 1 + 7 (rounds - 1) < 2 P: both buffers hold twice as many narrow elements as partitions)
    io.narrow = a.rounds_follow != 0 && io.idx_bits != 0 && ec >= kRoundsNarrowEc && lag_bits <= 32 && P >= 8;
    return io;
}

__global__ __launch_bounds__(256) void emit_ids_kernel(LargeArgs a0, SortBufs b0, const LargeItem* items, char* scratch) {
    LA_PICK_ITEM(a, b, a0, b0, items, scratch, blockIdx.y)
    if ((int64_t)blockIdx.x * blockDim.x >= b.n) return;
    const bool fill_rank_minus1 = a.n_cons == 0;                       // nobody to assign to: Main.java:211-214
    const uint32_t fin = b.ctl->cur[kFinal];
    const uint32_t* val = val_buf(b, fin);
    const uint64_t* key = key_buf(b, fin);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const RoundsIo io = rounds_io(a, key, b.n, a.n_cons, true);
    uint32_t* lag32 = reinterpret_cast<uint32_t*>(key_buf(b, fin ^ 1u));          // (narrow form: the rounds' lags)
    const uint32_t C32 = (uint32_t)a.n_cons;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < b.n; i += stride) {
        const uint32_t v = val[i];
        const uint64_t k = key[i];
        if (i > 0) {
            const uint64_t kp = key[i - 1];
            bad |= kp > k || (kp == k && val[i - 1] > v);
        }
        if (io.narrow) {
            const uint32_t q = (uint32_t)i / C32;                                // (b.n < 2^31)
            lag32[(int64_t)q * io.cpad + ((uint32_t)i - q * C32)] = (uint32_t)(k ^ kLagKeyFlip);
        }
        a.out_pid[a.p0 + i] = (int32_t)(v ^ kPidBias);
        if (fill_rank_minus1) a.out_rank[a.p0 + i] = -1;
    }
    if (__any(bad) && (threadIdx.x & (kWave - 1)) == 0) atomicOr(a.status, kStatusOrder);
}

// ---- kernel 3, packed form: bins are one 64-bit word -----------------------------------------------------
// (total << idx_bits) | index, ascending = (total, member) ascending, the comparator of Main.java:253-259.
// Element i = tid*EC + r.  Strides inside a wavefront run through the instruction-level networks of
// la_sort64.h (registers, DPP); strides across wavefronts go through LDS: 10 exchanges per round at 8 192 bins
// (workgroup_sort_p64).

#ifdef LA_ROUND_CLOCKS   // development build: thread 0 accumulates the cycles of every phase of a round (tools/cfg5_probe.py)
__device__ unsigned long long g_round_clocks[16];
__device__ unsigned long long g_round_stamp[520];        // [q] clock at the start of round q; [260 + q] path << 32 | bins that moved
#define LA_STAMP(q, path, m)                                                                           \
    do {                                                                                               \
        if (threadIdx.x == 0 && (q) < 259) {                                                           \
            g_round_stamp[q] = clock64();                                                              \
            g_round_stamp[260 + (q)] = ((unsigned long long)(path) << 32) | (unsigned)(m);             \
        }                                                                                              \
    } while (0)
#define LA_CLK(i)                                                          \
    do {                                                                   \
        if (threadIdx.x == 0) {                                            \
            const unsigned long long now_ = clock64();                     \
            g_round_clocks[i] += now_ - clk_;                              \
            clk_ = now_;                                                   \
        }                                                                  \
    } while (0)
#define LA_CLK_START unsigned long long clk_ = clock64()
#define LA_CLK_PARAM , unsigned long long& clk_          // a helper that times its phases on the caller's clock
#define LA_CLK_ARG , clk_
#else
#define LA_CLK_PARAM
#define LA_CLK_ARG
#define LA_CLK(i) do {} while (0)
#define LA_CLK_START do {} while (0)
#define LA_STAMP(q, path, m) do {} while (0)
#endif

constexpr int kSampleThreads = 1024;
constexpr uint32_t kMaxBucket = 96;
constexpr uint32_t kMaxBucket2 = 192;                        // second level: samples per super-sample bucket (~16)
// The rank walks read a bucket four staged bins at a time and may run past its end -- past the end of the staged array for
// the last bucket: that many sentinels (all ones: larger than any bin) close the array, so the loops need no clamp.
constexpr int kWalkPad = (int)kMaxBucket + 4, kWalkPad2 = (int)kMaxBucket2 + 4;

constexpr int kSamplesPerThread = 1;                         // 1 024 splitters: buckets of ~EC bins (2 per thread: the
                                                             // walk halves, but the sample sort's chain of steps grows more)

struct SampleLds {
    ulonglong2* stage;    // [n]  staged bins in bucket order: (bin, bucket size << 16 | slot); the final order
                          //      (uint64 [n]) is written over it once every staged bin is back in a register
    uint64_t* spl;        // [2 * NS] splitters in the first half; before that the two exchange buffers of the sample
                          //      sort's LDS steps (nothing else may be in flight there: the staging area is still being read
                          //      by slower threads when the fastest start the next round)
    uint32_t* cnt;        // [NS + 1] bucket counts, then (first position | size << 16)
    uint32_t* misc;       // [32] per-wavefront sums and maxima; [32 .. 32 + 66) second-level bucket counts, flag
    uint32_t* moved;      // [kMovedWords] the moved-bins sort's own words (moved_sort_bins): nothing else touches them
};
constexpr int kMovedWords = 352;

__host__ __device__ constexpr size_t sample_lds_bytes(int ec) {
    return ((size_t)ec * kSampleThreads + kWalkPad) * 16 + (size_t)kSamplesPerThread * kSampleThreads * (16 + 4) + 64 + (32 + 128) * 4 +
           (size_t)kMovedWords * 4;
}

__device__ __forceinline__ SampleLds sample_lds_carve(void* smem, int n) {
    SampleLds L;
    L.stage = reinterpret_cast<ulonglong2*>(smem);
    L.spl = reinterpret_cast<uint64_t*>(L.stage + n + kWalkPad);   // stage[n ..): sentinels, larger than any bin
    L.cnt = reinterpret_cast<uint32_t*>(L.spl + 2 * kSamplesPerThread * kSampleThreads);
    L.misc = L.cnt + kSamplesPerThread * kSampleThreads + 16;
    L.moved = L.misc + 32 + 128;
    return L;
}

// max over the wavefront, in every lane, without the LDS pipe (DPP + v_permlane*_swap butterflies)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = max(v, shfl_xor<1>(v));
    v = max(v, shfl_xor<2>(v));
    v = max(v, shfl_xor<4>(v));
    v = max(v, shfl_xor<8>(v));
    v = max(v, shfl_xor<16>(v));
    v = max(v, shfl_xor<32>(v));
    return v;
}

template <int EC>
__device__ __forceinline__ bool sample_sort_bins(P64 (&rec)[EC], const SampleLds& L, int tid, uint32_t bucket_limit) {
    constexpr int NT = kSampleThreads, N = EC * NT;
    constexpr int SPT = (EC >= 2 * kSamplesPerThread) ? kSamplesPerThread : 1;   // samples per thread
    constexpr int NS = SPT * NT;                                                   // splitters; NS + 1 buckets
    const int lane = tid & 63, wave = tid >> 6;
    LA_CLK_START;
    // 1. splitters: regular samples of last round's order, one bin per thread, SORTED -- by the same scheme one level
    //    down: 64 of the 1 024 samples are sorted by one wavefront (one per lane, DPP only), every sample finds its
    //    bucket among them (6 LDS reads), takes a slot, is staged, and is ranked by the walk over its bucket (~16
    //    samples).  6 barriers and ~50 LDS operations per thread, where the block-wide network over the samples
    //    needs 45 DPP steps, 10 LDS exchanges and 11 barriers -- a chain of latencies, 14k cycles of a 53k-cycle round.
    //    A second-level bucket above kMaxBucket2 sends the samples through the network instead.
    static_assert(SPT == 1, "one sample per thread");
    bool samples_sorted = false;
    {
        constexpr int S2 = 64;                                    // super-samples = lanes of the sorting wavefront
        uint64_t* smpbuf = L.spl + NS;                            // not the staging area: slower threads may still be
        uint32_t* cnt2 = L.misc + 32;                             // reading last round's final order out of it
        const uint64_t mine = p64_value(rec[EC / 2]);
        smpbuf[tid] = mine;
        L.cnt[tid] = 0;
        if (tid == 0) L.cnt[NS] = 0;
        if (tid < S2 + 2) cnt2[tid] = 0;
        lds_barrier();                                          // (1) from here on the staging area is free
        uint64_t* sup = reinterpret_cast<uint64_t*>(L.stage);     // [64] sorted super-samples
        ulonglong2* stage2 = L.stage + 64;                        // [NS + 2] staged samples
        if (wave == 0) {
            P64 v = p64_from(smpbuf[lane * (NS / S2) + NS / (2 * S2)]);
            asm volatile("s_nop 1" : "+v"(v.lo), "+v"(v.hi));
            bitonic_sort_lanes_p64<64>(v);
            sup[lane] = p64_value(v);
        } else if (tid - 64 < kWalkPad2) {
            stage2[NS + tid - 64] = make_ulonglong2(~0ull, 0);    // sentinels of the walk below
        }
        lds_barrier();                                          // (2)
        uint32_t b2 = 0;
#pragma unroll
        for (int step = S2 / 2; step >= 1; step >>= 1) b2 += (sup[b2 + step - 1] < mine) ? (uint32_t)step : 0u;
        b2 += (sup[S2 - 1] < mine) ? 1u : 0u;
        const uint32_t slot2 = atomicAdd(&cnt2[b2], 1u);
        lds_barrier();                                          // (3)
        if (wave == 0) {                                          // first positions of the 65 buckets; the largest one
            const uint32_t c = cnt2[lane];
            const uint32_t incl = wave_incl_scan_u32(c);
            const uint32_t last = cnt2[S2];
            const uint32_t mx = wave_max_u32(max(c, last));
            __builtin_amdgcn_wave_barrier();
            cnt2[lane] = (incl - c) | (c << 16);
            if (lane == 63) { cnt2[S2] = incl | (last << 16); cnt2[S2 + 1] = mx; }
        }
        lds_barrier();                                          // (4)
        // (the test hook that tightens the first level tightens this one too, so that all three forms of a round mix)
        if (cnt2[S2 + 1] <= (bucket_limit < kMaxBucket ? 24u : kMaxBucket2)) {      // workgroup-uniform
            const uint32_t sc = cnt2[b2];
            stage2[(sc & 0xFFFFu) + slot2] = make_ulonglong2(mine, (uint64_t)((sc & 0xFFFF0000u) | slot2));
            lds_barrier();                                      // (5)
            const ulonglong2 e = stage2[tid];
            const uint32_t inf = (uint32_t)e.y;
            const uint32_t s0 = (uint32_t)tid - (inf & 0xFFFFu);
            const uint32_t cmax = wave_max_u32(inf >> 16);
            const uint64_t* keys2 = reinterpret_cast<const uint64_t*>(stage2 + s0);      // the bucket's first staged sample
            uint32_t below = 0;
#pragma unroll 2
            for (uint32_t k = 0; k < cmax; k += 4) {
                const uint64_t o0 = keys2[2 * k], o1 = keys2[2 * k + 2], o2 = keys2[2 * k + 4], o3 = keys2[2 * k + 6];
                below += (o0 < e.x ? 1u : 0u) + (o1 < e.x ? 1u : 0u) + (o2 < e.x ? 1u : 0u) + (o3 < e.x ? 1u : 0u);
            }
            L.spl[s0 + below] = e.x;
            samples_sorted = true;
        }
    }
    if (!samples_sorted) {
        // the block-wide network over the samples (one per thread)
        lds_barrier();
        P64 smp[SPT];
#pragma unroll
        for (int u = 0; u < SPT; ++u) smp[u] = rec[(2 * u + 1) * EC / (2 * SPT)];
        workgroup_sort_p64<SPT>(smp, L.spl, NS, tid);
        lds_barrier();                            // the last step's reads, before the splitters go over its buffer
#pragma unroll
        for (int u = 0; u < SPT; ++u) L.spl[tid * SPT + u] = p64_value(smp[u]);
    }
    lds_barrier();
    LA_CLK(0);
    // 2. bucket of every bin = number of splitters below it (0 .. NS); a slot inside the bucket
    uint64_t x[EC];
    uint32_t b[EC], slot[EC];
#pragma unroll
    for (int r = 0; r < EC; ++r) { x[r] = p64_value(rec[r]); b[r] = 0; }
#pragma unroll
    for (int step = NS / 2; step >= 1; step >>= 1) {
#pragma unroll
        for (int r = 0; r < EC; ++r) b[r] += (L.spl[b[r] + step - 1] < x[r]) ? (uint32_t)step : 0u;
    }
    {
        const uint64_t top = L.spl[NS - 1];
#pragma unroll
        for (int r = 0; r < EC; ++r) b[r] += (top < x[r]) ? 1u : 0u;     // only where b is already NS - 1
    }
    LA_CLK(1);
#pragma unroll
    for (int r = 0; r < EC; ++r) slot[r] = atomicAdd(&L.cnt[b[r]], 1u);
    lds_barrier();
    {   // exclusive scan of the counts (thread t owns buckets t*SPT ..; bucket NS is what is left), largest bucket
        uint32_t c[SPT], sum = 0, m = 0;
#pragma unroll
        for (int u = 0; u < SPT; ++u) { c[u] = L.cnt[tid * SPT + u]; sum += c[u]; m = max(m, c[u]); }
        const uint32_t incl = wave_incl_scan_u32(sum);
        if (tid == 0) m = max(m, L.cnt[NS]);
        m = wave_max_u32(m);
        if (lane == 63) L.misc[wave] = incl;
        if (lane == 0) L.misc[16 + wave] = m;
        lds_barrier();
        const uint4* mv = reinterpret_cast<const uint4*>(L.misc);          // 16 sums, 16 maxima: eight 16-byte reads
        uint32_t base = 0, mx = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 sv = mv[q], xv = mv[4 + q];
            base += (4 * q + 0 < wave ? sv.x : 0u) + (4 * q + 1 < wave ? sv.y : 0u) + (4 * q + 2 < wave ? sv.z : 0u) +
                    (4 * q + 3 < wave ? sv.w : 0u);
            mx = max(max(mx, max(xv.x, xv.y)), max(xv.z, xv.w));
        }
        if (mx > bucket_limit) return false;          // workgroup-uniform: the caller sorts with the full network
        uint32_t first = base + incl - sum;
#pragma unroll
        for (int u = 0; u < SPT; ++u) {
            L.cnt[tid * SPT + u] = first | (c[u] << 16);
            first += c[u];
        }
        if (tid == NT - 1) L.cnt[NS] = first | (((uint32_t)N - first) << 16);
    }
    lds_barrier();
    LA_CLK(2);
    // 3. stage bucket by bucket, with (bucket size << 16 | slot) beside every staged bin
#pragma unroll
    for (int r = 0; r < EC; ++r) {
        const uint32_t sc = L.cnt[b[r]];
        L.stage[(sc & 0xFFFFu) + slot[r]] = make_ulonglong2(x[r], (uint64_t)((sc & 0xFFFF0000u) | slot[r]));
    }
    lds_barrier();
    LA_CLK(3);
    // Walk the staged bins wave-striped: 64 consecutive positions per step, a handful of consecutive buckets.
    // Final position = bucket start + members below the bin.  Reading past the bucket's end is harmless -- the bins
    // of later buckets are all larger, and two sentinels close the array -- so the loop has no per-lane bound.
    uint32_t pos[EC];
    uint64_t y[EC];
    const uint64_t* keys = reinterpret_cast<const uint64_t*>(L.stage);       // staged bin j at keys[2 * j]
#pragma unroll
    for (int it = 0; it < EC; ++it) {
        const uint32_t j = (uint32_t)(wave * 64 * EC + it * 64 + lane);
        const ulonglong2 e = L.stage[j];
        y[it] = e.x;
        const uint32_t inf = (uint32_t)e.y;
        const uint32_t s0 = j - (inf & 0xFFFFu);
        const uint32_t cmax = wave_max_u32(inf >> 16);
        const uint64_t* bk = keys + 2 * s0;                          // the bucket's first staged bin
        uint32_t below = 0;
#pragma unroll 2
        for (uint32_t k = 0; k < cmax; k += 4) {                     // past the array's end: kWalkPad sentinels
            const uint64_t o0 = bk[2 * k], o1 = bk[2 * k + 2], o2 = bk[2 * k + 4], o3 = bk[2 * k + 6];
            below += (o0 < y[it] ? 1u : 0u) + (o1 < y[it] ? 1u : 0u) + (o2 < y[it] ? 1u : 0u) + (o3 < y[it] ? 1u : 0u);
        }
        pos[it] = s0 + below;
    }
    LA_CLK(4);
    lds_barrier();                                 // every staged bin is in a register: the final order goes over them
    // 4. final order, back to blocked registers
    uint64_t* sorted = reinterpret_cast<uint64_t*>(L.stage);
#pragma unroll
    for (int it = 0; it < EC; ++it) sorted[pos[it]] = y[it];
    lds_barrier();
#pragma unroll
    for (int r = 0; r < EC; ++r) rec[r] = p64_from(sorted[tid * EC + r]);
    LA_CLK(5);
    return true;
}

// ---- a round whose bins are a few ascending runs: merge them ------------------------------------------------------------
// Out of a round the bins are (ascending totals) + (descending lags).  Where the lags of a round take few distinct values
// -- the flat tail of a power-law topic, ties, zero lags -- the new values are a handful of ascending RUNS (cfg5: 1 700
// runs in round 2, 95 in round 16, 30 in round 32, 4 - 16 from round 48 on; one run = already in order).  Sorting them is
// then a tree of pairwise merges of adjacent runs, ceil(log2 R) levels, each level one pass of the bins through LDS:
// every thread owns 8 consecutive OUTPUT positions, finds where its first output starts in the two runs of its pair
// (merge path: one binary search), and merges sequentially from there -- ~45 dependent LDS reads per thread and level
// where a sample-sorted round costs ~350 LDS operations and 16 barriers.
// Returns false (and leaves rec alone) when there are more than kMaxRuns runs: the caller sorts as before.  *runs_out = the
// number of runs found, so that the caller can decide when to look again.
constexpr int kMaxRuns = 32;

template <int EC>
__device__ __forceinline__ bool merge_runs_bins(P64 (&rec)[EC], const SampleLds& L, int tid, int* runs_out) {
    constexpr int NT = kSampleThreads, N = EC * NT;
    const int lane = tid & 63, wave = tid >> 6;
    uint64_t* buf_a = reinterpret_cast<uint64_t*>(L.stage);          // [N] the runs
    uint64_t* buf_b = buf_a + N;                                     // [N] the merged runs of a level
    uint32_t* bnd = L.cnt;                                           // [R + 1] first position of every run, then N
    uint32_t* wsum = L.misc;                                         // [16] descents per wavefront
    // Position p of the sorted order lives at word (p % EC) * NT + p / EC of a buffer (register-major): a thread's EC
    // consecutive positions are NT words apart, so the 64 lanes of every blocked read or write hit 64 consecutive words
    // (position-major, they would sit 64 bytes apart: 16-way bank conflicts on every level's output).
    auto at = [](uint32_t p) -> uint32_t { return (p % EC) * NT + p / EC; };
    lds_barrier();                                                   // last round's readers of the staging area are done
    uint64_t v[EC];
#pragma unroll
    for (int r = 0; r < EC; ++r) { v[r] = p64_value(rec[r]); buf_a[r * NT + tid] = v[r]; }
    lds_barrier();
    // descents: position p starts a new run when bins[p - 1] > bins[p]  (p = tid * EC + r; the bins are distinct)
    const uint64_t before = tid > 0 ? buf_a[(EC - 1) * NT + tid - 1] : 0;
    uint32_t starts = 0, mine = 0;                                   // bit r: my r-th position starts a run
#pragma unroll
    for (int r = 0; r < EC; ++r) {
        const bool st = (r == 0 ? before : v[r - 1]) > v[r];
        starts |= st ? (1u << r) : 0u;
        mine += st ? 1u : 0u;
    }
    const uint32_t incl = wave_incl_scan_u32(mine);
    if (lane == 63) wsum[wave] = incl;
    lds_barrier();
    uint32_t base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const uint32_t x = wsum[w];
        base += w < wave ? x : 0u;
        total += x;
    }
    const int R = (int)total + 1;
    *runs_out = R;
    if (R > kMaxRuns) return false;                                  // workgroup-uniform
    if (R == 1) return true;                                         // in order already: rec is untouched and right
    {
        uint32_t at = 1 + base + incl - mine;                        // run number of my first start
#pragma unroll
        for (int r = 0; r < EC; ++r)
            if (starts & (1u << r)) bnd[at++] = (uint32_t)(tid * EC + r);
        if (tid == 0) { bnd[0] = 0; bnd[R] = (uint32_t)N; }
    }
    lds_barrier();
    // the tree: at level `stride` the runs are bnd[0], bnd[stride], bnd[2 stride] ..; pair k merges runs 2k and 2k + 1 of them
    uint64_t* src = buf_a;
    uint64_t* dst = buf_b;
    for (int stride = 1; stride < R; stride <<= 1) {
        auto at_run = [&](int i) -> uint32_t { return bnd[i < R ? i : R]; };
        const int n_pairs = (R + 2 * stride - 1) / (2 * stride);
        const uint32_t o = (uint32_t)(tid * EC);                     // my first output position
        // the pair my first output falls into: the last k with at_run(2 k stride) <= o
        int k = 0;
        for (int step = kMaxRuns / 2; step >= 1; step >>= 1)         // n_pairs <= kMaxRuns / 2
            if (k + step < n_pairs && at_run(2 * (k + step) * stride) <= o) k += step;
        uint32_t a0 = at_run(2 * k * stride), a1 = at_run((2 * k + 1) * stride), a2 = at_run((2 * k + 2) * stride);
        // merge path: of the d = o - a0 outputs before mine, i come from the first run and d - i from the second
        const uint32_t d = o - a0, len_a = a1 - a0, len_b = a2 - a1;
        uint32_t lo = d > len_b ? d - len_b : 0u, hi = d < len_a ? d : len_a;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (src[at(a0 + mid)] < src[at(a1 + (d - mid - 1))]) lo = mid + 1; else hi = mid;
        }
        uint32_t ia = a0 + lo, ib = a1 + (d - lo);                   // next element of either run
        uint64_t xa = ia < a1 ? src[at(ia)] : ~0ull, xb = ib < a2 ? src[at(ib)] : ~0ull;
        uint64_t out[EC];
#pragma unroll
        for (int r = 0; r < EC; ++r) {
            if (ia >= a1 && ib >= a2) {                              // my outputs run on into the next pair
                ++k;
                a0 = a2; a1 = at_run((2 * k + 1) * stride); a2 = at_run((2 * k + 2) * stride);
                ia = a0; ib = a1;
                xa = ia < a1 ? src[at(ia)] : ~0ull;
                xb = ib < a2 ? src[at(ib)] : ~0ull;
            }
            const bool take_a = ib >= a2 || (ia < a1 && xa < xb);
            out[r] = take_a ? xa : xb;
            if (take_a) { ++ia; xa = ia < a1 ? src[at(ia)] : ~0ull; }
            else { ++ib; xb = ib < a2 ? src[at(ib)] : ~0ull; }
        }
#pragma unroll
        for (int r = 0; r < EC; ++r) dst[r * NT + tid] = out[r];
        lds_barrier();
        uint64_t* t = src; src = dst; dst = t;
    }
#pragma unroll
    for (int r = 0; r < EC; ++r) rec[r] = p64_from(src[r * NT + tid]);
    return true;
}

// ---- a round that moves few bins: only those are sorted ------------------------------------------------------------------
// Out of a round the bins are (ascending totals) + (descending lags).  On a power-law topic most of the consumers stand far
// apart after the first round -- the few that took the huge lags, a long thin tail -- and a round's lags differ by less than
// their distances: they keep their places.  Only the dense bulk moves: cfg5 (8 192 consumers) moves 3 168 bins in round 1,
// 1 263 in round 2, 850 - 1 060 in rounds 3 - 75 and ~500 after that, while the round's bins are up to 600 ascending runs
// (`profiles/archive/r04_cfg5_rounds.txt`).  A bin STAYS where it is when it is larger than every bin before it and smaller than
// every bin behind it (a prefix maximum and a suffix minimum); such a bin separates what comes before it from what comes
// behind it, so the bins that do not stay are sorted among themselves and go back, in order, to the places they came from.
//   1. per thread (EC consecutive bins): ascending inside, above the maximum of everything before, below the minimum of
//      everything behind?  A wavefront whose 64 * EC bins ascend needs no scan for that (its maximum is its last bin); the
//      others scan their lanes (DPP).  Across wavefronts: 16 maxima / minima through LDS.  Only the wavefronts that hold a
//      thread with a bin that moves look at single bins and count them.
//   2. the bins that move are written side by side, in the order of their places (m of them, at most a quarter of the
//      round's bins) and sorted with one or two per thread by the scheme of the sample sort one level down: 64 of them, evenly
//      spaced, are ranked against each other (four per wavefront: one compare + ballot each), every bin finds its bucket
//      among those (7 LDS reads), takes a slot, is staged by bucket and ranked by the walk over its bucket (~m / 64 bins).
//      m <= 64: one wavefront sorts them in registers.
//   3. the sorted bins go back to the places the bins that move came from.
// Six barriers and ~60 LDS operations in the threads that take part; the wavefronts whose bins all stay (13 of 16 on cfg5)
// spend ~100 VALU instructions on finding that out -- on a CU with 16 wavefronts every instruction that all of them execute
// costs 16 cycles, which is what a round is made of.  Returns false -- rec untouched -- when more bins move than fit (or a
// bucket is larger than `bucket_limit`): the caller sorts the round as before.  *moved_out = the number of bins that move.
constexpr int kMovedPad = 164;                               // sentinels behind the staged bins (the walk reads four at a time)
constexpr uint32_t kMovedBucket = 160;

// inclusive prefix maximum over the lanes of the wavefront (row shifts, then the row broadcasts; a lane without a source
// reads zero, the identity)
__device__ __forceinline__ uint64_t wave_incl_max_u64(uint64_t v) {
#define LA_MAX_STEP(CTRL, ROWS)                                                                                          \
    {                                                                                                                    \
        const uint32_t lo_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROWS, 0xF, false);         \
        const uint32_t hi_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROWS, 0xF, false); \
        const uint64_t o_ = ((uint64_t)hi_ << 32) | lo_;                                                                 \
        v = o_ > v ? o_ : v;                                                                                             \
    }
    LA_MAX_STEP(0x111, 0xF)        // row_shr:1
    LA_MAX_STEP(0x112, 0xF)        // row_shr:2
    LA_MAX_STEP(0x114, 0xF)        // row_shr:4
    LA_MAX_STEP(0x118, 0xF)        // row_shr:8
    LA_MAX_STEP(0x142, 0xA)        // row_bcast:15 -> rows 1, 3
    LA_MAX_STEP(0x143, 0xC)        // row_bcast:31 -> rows 2, 3
#undef LA_MAX_STEP
    return v;
}

__device__ __forceinline__ uint64_t wave_shr1_u64(uint64_t v) {            // lane - 1's value; lane 0 reads zero
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x138, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x138, 0xF, 0xF, false);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t wave_mirror_u64(uint64_t v) {          // lane 63 - lane's value
    return ((uint64_t)shfl_mirror<64>((uint32_t)(v >> 32)) << 32) | shfl_mirror<64>((uint32_t)v);
}

template <int J>
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v) {
    return ((uint64_t)shfl_xor<J>((uint32_t)(v >> 32)) << 32) | shfl_xor<J>((uint32_t)v);
}

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int lane) {   // (lane: wavefront-uniform)
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
}

// The small sort of moved_sort_bins: the m bins that move stand side by side in comp[0 .. m); on return they stand there in
// order.  NS samples (64 or 128) cut them into NS + 1 buckets; a bin's place is its bucket's first place plus the number of
// bins of its bucket below it.  CPT = bins per thread (m <= CPT * 1 024).  false: a bucket grew beyond `bucket_limit` (the
// caller sorts the round another way; comp is spent either way).
template <int CPT, int NS>
__device__ __forceinline__ bool moved_small_sort(uint64_t* comp, ulonglong2* stage2, uint64_t* sup, uint64_t* sup1, uint32_t* cnt2,
                                                 const int m, const int tid, const uint32_t bucket_limit LA_CLK_PARAM) {
    constexpr int NT = kSampleThreads;
    constexpr int NSUP = NS / 8;                                 // every eighth sample
    static_assert(NS == 64 || NS == 128, "one or two samples per lane");
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        // NS evenly spaced samples (distinct places: m > NS), every wavefront ranks NS / 16 of them: the number of samples
        // below one is its place among them
        if constexpr (NS == 64) {
            const uint64_t smp = comp[((uint32_t)lane * (uint32_t)m + (uint32_t)m / 2u) >> 6];
#pragma unroll
            for (int k = 0; k < 64 / (NT / 64); ++k) {
                const uint64_t s = readlane_u64(smp, wave * (64 / (NT / 64)) + k);
                const int rank = __builtin_popcountll(__builtin_amdgcn_ballot_w64(smp < s));
                if (lane == 0) {
                    sup[rank] = s;
                    if ((rank & 7) == 7) sup1[rank >> 3] = s;
                }
            }
        } else {
            const uint64_t smp0 = comp[((uint32_t)lane * (uint32_t)m + (uint32_t)m / 2u) >> 7];
            const uint64_t smp1 = comp[((uint32_t)(64 + lane) * (uint32_t)m + (uint32_t)m / 2u) >> 7];
            const uint64_t mine = wave < 8 ? smp0 : smp1;        // wavefronts 0 .. 7 rank samples 0 .. 63, the others 64 .. 127
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint64_t s = readlane_u64(mine, (wave & 7) * 8 + k);
                const int rank = __builtin_popcountll(__builtin_amdgcn_ballot_w64(smp0 < s)) +
                                 __builtin_popcountll(__builtin_amdgcn_ballot_w64(smp1 < s));
                if (lane == 0) {
                    sup[rank] = s;
                    if ((rank & 7) == 7) sup1[rank >> 3] = s;
                }
            }
        }
        if (tid < kMovedPad) stage2[m + tid] = make_ulonglong2(~0ull, 0);     // sentinels behind the staged bins
    }
    lds_barrier();                                               // (3)
    LA_CLK(10);
    uint64_t x[CPT];
    uint32_t b2[CPT], slot[CPT];
#pragma unroll
    for (int u = 0; u < CPT; ++u) {
        const int c = tid + u * NT;
        x[u] = ~0ull; b2[u] = 0; slot[u] = 0;
        if (u * NT + wave * 64 < m) {                            // (wavefront-uniform: a wavefront without a bin skips the phase)
            const bool valid = c < m;
            x[u] = comp[valid ? c : 0];
            // bucket = the number of samples below the bin, in two steps (two dependent trips to LDS where a binary search
            // makes seven): which eighth (sixteenth) of the samples, then where inside it
            uint32_t c1 = 0, c2 = 0;
#pragma unroll
            for (int i = 0; i < NSUP; ++i) c1 += (sup1[i] < x[u]) ? 1u : 0u;
            const uint32_t r1 = c1 < (uint32_t)(NSUP - 1) ? c1 : (uint32_t)(NSUP - 1);
            const uint64_t* row = sup + 8u * r1;
#pragma unroll
            for (int i = 0; i < 8; ++i) c2 += (row[i] < x[u]) ? 1u : 0u;           // (c1 < NSUP: row[7] is not below)
            const uint32_t b = 8u * r1 + c2;
            b2[u] = b;
            if (valid) slot[u] = atomicAdd(&cnt2[b], 1u);
        }
    }
    lds_barrier();                                               // (4)
    LA_CLK(11);
    // first places of the NS + 1 buckets, the largest bucket: every wavefront for itself (a scan over its lanes), no barrier
    uint32_t first[CPT], size[CPT];
    if constexpr (NS == 64) {
        const uint32_t c = cnt2[lane];
        const uint32_t incl = wave_incl_scan_u32(c);
        const uint32_t last = cnt2[64];
        if (wave_max_u32(max(c, last)) > bucket_limit) return false;             // (workgroup-uniform: same counts everywhere)
        const uint32_t all = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
#pragma unroll
        for (int u = 0; u < CPT; ++u) {
            const uint32_t bl = b2[u] & 63u;
            const uint32_t f = (uint32_t)__shfl((int)(incl - c), (int)bl), z = (uint32_t)__shfl((int)c, (int)bl);
            first[u] = b2[u] < 64u ? f : all;
            size[u] = b2[u] < 64u ? z : last;
        }
    } else {
        const uint32_t c0 = cnt2[lane], c1 = cnt2[64 + lane];
        const uint32_t last = cnt2[128];
        if (wave_max_u32(max(max(c0, c1), last)) > bucket_limit) return false;   // (workgroup-uniform)
        const uint32_t incl0 = wave_incl_scan_u32(c0);
        const uint32_t all0 = (uint32_t)__builtin_amdgcn_readlane((int)incl0, 63);
        const uint32_t incl1 = wave_incl_scan_u32(c1) + all0;
        const uint32_t all = (uint32_t)__builtin_amdgcn_readlane((int)incl1, 63);
#pragma unroll
        for (int u = 0; u < CPT; ++u) {
            const uint32_t bl = b2[u] & 63u;
            const uint32_t f0 = (uint32_t)__shfl((int)(incl0 - c0), (int)bl), z0 = (uint32_t)__shfl((int)c0, (int)bl);
            const uint32_t f1 = (uint32_t)__shfl((int)(incl1 - c1), (int)bl), z1 = (uint32_t)__shfl((int)c1, (int)bl);
            first[u] = b2[u] < 64u ? f0 : (b2[u] < 128u ? f1 : all);
            size[u] = b2[u] < 64u ? z0 : (b2[u] < 128u ? z1 : last);
        }
    }
    LA_CLK(12);
#pragma unroll
    for (int u = 0; u < CPT; ++u) {
        const int c = tid + u * NT;
        if (c < m) stage2[first[u] + slot[u]] = make_ulonglong2(x[u], (uint64_t)((size[u] << 16) | slot[u]));
    }
    lds_barrier();                                               // (5)
    LA_CLK(13);
    const uint64_t* keys = reinterpret_cast<const uint64_t*>(stage2);
#pragma unroll
    for (int u = 0; u < CPT; ++u) {
        const int c = tid + u * NT;
        if (u * NT + wave * 64 < m) {                            // (wavefront-uniform: the walk's bound is a wavefront maximum)
            const bool valid = c < m;
            const ulonglong2 e = valid ? stage2[c] : make_ulonglong2(~0ull, 0);
            const uint32_t inf = (uint32_t)e.y;
            const uint32_t s0 = valid ? (uint32_t)c - (inf & 0xFFFFu) : 0u;
            const uint32_t cmax = wave_max_u32(inf >> 16);
            const uint64_t* bk = keys + 2 * s0;
            uint32_t below = 0;
#pragma unroll 2
            for (uint32_t k = 0; k < cmax; k += 4) {
                const uint64_t o0 = bk[2 * k], o1 = bk[2 * k + 2], o2 = bk[2 * k + 4], o3 = bk[2 * k + 6];
                below += (o0 < e.x ? 1u : 0u) + (o1 < e.x ? 1u : 0u) + (o2 < e.x ? 1u : 0u) + (o3 < e.x ? 1u : 0u);
            }
            if (valid) comp[s0 + below] = e.x;                   // (comp was last read before barrier 4)
        }
    }
    lds_barrier();                                               // (6)
    LA_CLK(14);
    return true;
}

template <int EC>
__device__ __forceinline__ bool moved_sort_bins(P64 (&rec)[EC], const SampleLds& L, int tid, uint32_t bucket_limit, int* moved_out,
                                                const int parity) {
    constexpr int NT = kSampleThreads;
    constexpr int CPT = EC >= 8 ? 2 : 1;                         // bins of the small sort per thread
    constexpr int kCapN = 256 * EC;                              // its capacity (a quarter of the round's bins) in the narrow form
    constexpr bool kWide = EC >= 4;        // the wide form: twice the capacity, twice the bins per thread, 128 buckets
    constexpr int kCap = kWide ? 2 * kCapN : kCapN;              // what the side-by-side array holds
    static_assert(kCapN <= CPT * NT && NT == 1024, "capacity");
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // [16] a wavefront's largest bin, [16] its smallest, [16] whether its bins ascend: two sets, calls alternate (`parity`) -- a round
    // in which nothing moves leaves after barrier (1), and the fastest wavefront writes the next call's words while the slowest
    // still reads this call's
    uint64_t* wmax = reinterpret_cast<uint64_t*>(L.moved + ((parity & 1) ? 256 : 0));
    uint64_t* wmin = wmax + 16;
    uint32_t* wasc = L.moved + 320 + ((parity & 1) ? 16 : 0);
    uint32_t* wcnt = L.moved + 64;                               // [16] its bins that move
    uint32_t* cnt2 = L.moved + 80;                               // [128 + 1] bucket counts (64 + 1 in the narrow form)
    uint32_t* taken = L.moved + 210;                             // [1] places of the side-by-side array handed out so far
    uint64_t* comp = reinterpret_cast<uint64_t*>(L.stage);       // [kCap] the bins that move, in the order of their places; then sorted
    ulonglong2* stage2 = reinterpret_cast<ulonglong2*>(comp + kCap);     // [kCap + kMovedPad] staged by bucket
    uint64_t* sup = reinterpret_cast<uint64_t*>(stage2 + kCap + kMovedPad);   // [64 | 128] the samples in order
    uint64_t* sup1 = sup + 128;                                  // [8 | 16] every eighth of them (sup[7], sup[15] ..)
    LA_CLK_START;
    // 1. who stays
    uint64_t v[EC];
#pragma unroll
    for (int r = 0; r < EC; ++r) v[r] = p64_value(rec[r]);
    bool asc = true;
#pragma unroll
    for (int r = 1; r < EC; ++r) asc &= v[r - 1] < v[r];
    const uint64_t prev_last = wave_shr1_u64(v[EC - 1]);         // (every lane executes the shift: la_sort64.h on masked sources)
    const bool asc_w = asc & ((lane == 0) | (prev_last < v[0]));
    const bool wave_asc = __builtin_amdgcn_ballot_w64(!asc_w) == 0;              // wavefront-uniform
    uint64_t pm_in = 0, sm_in = ~0ull;                           // over the earlier / later lanes of this wavefront
    uint64_t w_hi, w_lo;
    if (wave_asc) {
        w_hi = readlane_u64(v[EC - 1], 63);
        w_lo = readlane_u64(v[0], 0);
    } else {
        uint64_t tmax = v[0], tmin = v[0];
#pragma unroll
        for (int r = 1; r < EC; ++r) { tmax = v[r] > tmax ? v[r] : tmax; tmin = v[r] < tmin ? v[r] : tmin; }
        const uint64_t incl = wave_incl_max_u64(tmax);
        pm_in = wave_shr1_u64(incl);
        w_hi = readlane_u64(incl, 63);
        // the suffix minimum is the prefix maximum of the complements, lanes mirrored
        const uint64_t incl_m = wave_incl_max_u64(wave_mirror_u64(~tmin));
        sm_in = ~wave_mirror_u64(wave_shr1_u64(incl_m));
        w_lo = ~readlane_u64(incl_m, 63);
    }
    if (lane == 0) { wmax[wave] = w_hi; wmin[wave] = w_lo; wasc[wave] = wave_asc ? 1u : 0u; }
    if (tid < 129) cnt2[tid] = 0;
    if (tid == 129) *taken = 0;
    lds_barrier();                                               // (1)
    LA_CLK(7);
    // the sixteen wavefronts' words, one read each (lane l and its copies in the other rows hold wavefront l & 15's)
    const uint64_t hi_l = wmax[lane & 15], lo_l = wmin[lane & 15];
    {
        // nothing moves at all?  Every wavefront ascends and begins above the one before it: the round's bins are in order, and
        // the round is over -- no second barrier, no counts (a topic of equal lags, a consumer group that has caught up: every round)
        const uint32_t as_l = wasc[lane & 15];
        const uint32_t hb_lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)hi_l, 0x111, 0xF, 0xF, false);          // row_shr:1
        const uint32_t hb_hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(hi_l >> 32), 0x111, 0xF, 0xF, false);
        const uint64_t hi_before = ((uint64_t)hb_hi << 32) | hb_lo;                // (a row's first lane: zero)
        const bool fine = as_l != 0 && hi_before < lo_l;
        if (__builtin_amdgcn_ballot_w64(!fine) == 0) {
            *moved_out = 0;
            return true;
        }
    }
    uint64_t pm_w, sm_w;                                         // over the earlier / later wavefronts
    {
        uint64_t a = lane < wave ? hi_l : 0;
        uint64_t b = (lane > wave && lane < NT / 64) ? lo_l : ~0ull;
#define LA_RED_STEP(J)                                                        \
        {                                                                     \
            const uint64_t oa_ = shfl_xor_u64<J>(a), ob_ = shfl_xor_u64<J>(b); \
            a = oa_ > a ? oa_ : a;                                            \
            b = ob_ < b ? ob_ : b;                                            \
        }
        LA_RED_STEP(1) LA_RED_STEP(2) LA_RED_STEP(4) LA_RED_STEP(8)
#undef LA_RED_STEP
        pm_w = readlane_u64(a, 0);
        sm_w = readlane_u64(b, 0);
    }
    const uint64_t before = pm_in > pm_w ? pm_in : pm_w, behind = sm_in < sm_w ? sm_in : sm_w;
    const bool moves = !(asc & (before < v[0]) & (v[EC - 1] < behind));
    const bool wave_moves = __builtin_amdgcn_ballot_w64(moves) != 0;             // wavefront-uniform
    uint32_t mask = 0, off = 0;                                  // my bins that move; how many move before them
    if (wave_moves) {
        // bin r stays when everything before it is smaller and everything behind it is larger
        uint64_t sm[EC];
        {
            uint64_t x = behind;
#pragma unroll
            for (int r = EC - 1; r >= 0; --r) { sm[r] = x; x = v[r] < x ? v[r] : x; }
        }
        uint64_t run = before;
#pragma unroll
        for (int r = 0; r < EC; ++r) {
            mask |= ((run < v[r]) & (v[r] < sm[r])) ? 0u : (1u << r);
            run = v[r] > run ? v[r] : run;
        }
        const uint32_t mine = (uint32_t)__builtin_popcount(mask);
        const uint32_t incl = wave_incl_scan_u32(mine);
        off = incl - mine;
        // 2. the bins that move, side by side: the wavefront takes as many places as it needs (in whatever order the
        //    wavefronts come: the order of the PLACES is kept in `off`, for the way back) and fills them
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        uint32_t k = 0;
        if (lane == 0) { k = atomicAdd(taken, total); wcnt[wave] = total; }
        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k) + off;
#pragma unroll
        for (int r = 0; r < EC; ++r)
            if (mask & (1u << r)) {
                if (k < (uint32_t)kCap) comp[k] = v[r];
                ++k;
            }
    } else if (lane == 0) {
        wcnt[wave] = 0;
    }
    lds_barrier();                                               // (2)
    LA_CLK(8);
    int m = 0;
    {
        const uint4* cv = reinterpret_cast<const uint4*>(wcnt);
        uint32_t base = 0;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const uint4 c = cv[q4];
            const uint32_t c0 = __builtin_amdgcn_readfirstlane(c.x), c1 = __builtin_amdgcn_readfirstlane(c.y),
                           c2 = __builtin_amdgcn_readfirstlane(c.z), c3 = __builtin_amdgcn_readfirstlane(c.w);
            base += (4 * q4 + 0 < wave ? c0 : 0u) + (4 * q4 + 1 < wave ? c1 : 0u) + (4 * q4 + 2 < wave ? c2 : 0u) +
                    (4 * q4 + 3 < wave ? c3 : 0u);
            m += (int)(c0 + c1 + c2 + c3);
        }
        off += base;
    }
    *moved_out = m;
    if (m == 0) return true;                                     // in order already
    if (m > kCap) return false;                                  // (workgroup-uniform)
    if (m <= 64) {
        if (wave == 0) {                                         // one wavefront sorts them
            P64 s = p64_from(lane < m ? comp[lane] : ~0ull);
            asm volatile("s_nop 1" : "+v"(s.lo), "+v"(s.hi));
            bitonic_sort_lanes_p64<64>(s);
            if (lane < m) comp[lane] = p64_value(s);
        }
        lds_barrier();
    } else if (__builtin_expect(m <= kCapN, 1)) {
        if (!moved_small_sort<CPT, 64>(comp, stage2, sup, sup1, cnt2, m, tid, bucket_limit LA_CLK_ARG)) return false;
    } else {
        if constexpr (kWide) {
            // more bins move than the narrow form holds, not more than twice as many (the dense bulk of a power-law topic of
            // 131 072 .. 262 144 or of ~2 M partitions over 8 192 consumers: 2 050 - 3 100 per round): the same sort with four bins
            // per thread and 128 buckets -- a round of 27 - 33 k cycles where the sample sort over all bins takes 51 k and the run
            // merge 55 - 59 k.  Decided per round from what the round's bins say (round 6's first wide form was chosen by the
            // host from the number of rounds, kept 64 buckets, and lost wherever ~4 000 bins moved).
            if (m > kWideMovedLimit * EC) return false;
            if (!moved_small_sort<2 * CPT, 128>(comp, stage2, sup, sup1, cnt2, m, tid, bucket_limit LA_CLK_ARG)) return false;
        } else {
            return false;
        }
    }
    // 3. back to the places the bins that move came from
    if (wave_moves) {
        uint32_t k = off;
#pragma unroll
        for (int r = 0; r < EC; ++r)
            if (mask & (1u << r)) rec[r] = p64_from(comp[k++]);
    }
    LA_CLK(15);
    return true;
}

template <int EC>
__device__ void greedy_rounds_packed(const LargeArgs& a, const uint64_t* key, int64_t P, int C, int64_t rounds,
                                     int idx_bits, void* smem, const uint32_t* lag32, uint16_t* idx16, const int64_t cpad,
                                     const bool zero_tail) {
    const int tid = threadIdx.x;
    const int n = EC * blockDim.x;
    constexpr int kSpan = 64 * EC;                       // elements of one wavefront
    const uint32_t idx_mask = (1u << idx_bits) - 1;
    uint64_t* s_bin = reinterpret_cast<uint64_t*>(smem);
    [[maybe_unused]] const SampleLds L = sample_lds_carve(smem, n);
    [[maybe_unused]] const bool use_sample = (EC >= 2) && blockDim.x == kSampleThreads && a.no_sample_sort != 1;
    if (use_sample && tid < kWalkPad) L.stage[n + tid] = make_ulonglong2(~0ull, 0);      // first read after many barriers
    P64 rec[EC];
    // raw sorted keys of the round's partitions, one round ahead.  The loads are UNCONDITIONAL (index clamped) and
    // issued back to back: a branch around a load makes hipcc wait for it before issuing the next one -- eight
    // serialized memory round trips per round here, 6k of a round's 52k cycles; the select happens at the use, a
    // whole round of sorting later.
    // lag[]: the lags themselves (the keys' flip is undone when they arrive, not when they are added).  narrow: the
    // 32-bit lags emit_ids_kernel left, a round's stretch `cpad` elements after the one before (rounds_io).
    const bool narrow = EC >= kRoundsNarrowEc && EC >= 4 && lag32 != nullptr;     // (workgroup-uniform; never for fewer bins per thread)
    const int64_t cap8 = (2 * P - 8) & ~(int64_t)3;                              // the last aligned place a 8-element read may start
    uint64_t lag[EC];
#pragma unroll
    for (int r = 0; r < EC; ++r) {
        const int i = tid * EC + r;
        // pads (slots beyond the C consumers) sort behind every bin and, like the bins, are all different
        rec[r] = p64_from(i < C ? (uint64_t)i : ((~0ull << idx_bits) | (uint64_t)i));
        if (narrow) lag[r] = lag32[i < cap8 ? i : cap8];                          // (round 0 starts at element 0)
        else lag[r] = key[i < P ? i : P - 1] ^ kLagKeyFlip;
    }
    [[maybe_unused]] int64_t next_look = 1;              // the next round that looks whether its bins are a few ascending runs
    [[maybe_unused]] int64_t next_moved = 2;             // the next round that looks whether few of its bins move (round 1 sorts
                                                         // what round 0 made of equal bins: every bin moves)
    [[maybe_unused]] int moved_wait = 0;
    [[maybe_unused]] int moved_calls = 0;                // (the moved-bins sort alternates between two sets of its first words)
    // The lags descend, so a round whose FIRST lag is zero hands out zeros only, and so does every round behind it: nothing is
    // added any more, the order the bins stand in when that round begins is final and the rounds behind it only write it down again
    // -- no order check, no barrier.  (A consumer group that has caught up on most partitions: the long tail of a big topic's
    // rounds.)  Which round that is, is found ONCE, before the loop -- 64 rounds probed per step by the lanes of every wavefront for
    // itself: two or three dependent loads -- because anything added to the loop for it cost every topic (a load of the next
    // round's first lag per round, scalar, vector or by one lane: cfg5 +7 %: one more instruction through the one compute unit's
    // address path per wavefront and round, or a memory round trip inside the next LDS barrier's lgkmcnt(0)).
    int64_t first_zero_round = rounds;                   // (workgroup-uniform)
    if (zero_tail) {                                     // (the topic's smallest lag is zero at all)
        const int lane = tid & 63;
        int64_t lo = 0, hi = rounds;                     // rounds below lo begin with a lag > 0; round hi (if any) with zero
        while (lo < hi) {
            const int64_t step = (hi - lo + 63) / 64;
            const int64_t r = lo + lane * step;
            uint64_t first = 0;
            if (r < hi) {
                if (narrow) { const int64_t f = r * cpad; first = lag32[f < cap8 ? f : cap8]; }
                else first = key[r * (int64_t)C] ^ kLagKeyFlip;
            }
            const uint64_t zeros = __builtin_amdgcn_ballot_w64(first == 0);      // (lanes beyond hi count as zero)
            if (zeros == 0) { lo = lo + 63 * step + 1; continue; }                // (cannot happen while 64 * step >= hi - lo; kept for safety)
            const int k = __builtin_ctzll(zeros);
            hi = lo + k * step < hi ? lo + k * step : hi;
            lo = k > 0 ? lo + (int64_t)(k - 1) * step + 1 : lo;
            if (k == 0) hi = lo;
        }
        first_zero_round = lo;
    }
    const int tid_fixed = tid;
    for (int64_t q = 0; q < rounds; ++q) {
        // The thread index, opaque once per round: everything a round derives from it (lane predicates, LDS addresses, masks)
        // is then computed in the round -- a few VALU instructions -- instead of once before the loop, where hipcc parks the
        // values in scratch memory (the kernel sits at its 128-register cap) and reloads them in the middle of the chain.
        int tid = tid_fixed;
        asm volatile("" : "+v"(tid));
        [[maybe_unused]] int path_ = 0, moved_ = 0;
        if (q > 0 && q <= first_zero_round) {
            bool sorted = false;
            if constexpr (EC >= 2) {
                // Round 0 handed the DESCENDING lags to the bins in index order (all totals were 0): where the lags differ the
                // bins stand in exactly the reverse of the order round 1 needs, and only runs of equal lags (index order = the
                // right order already) are out of place once the C bins are turned around.  So round 1 turns them around through
                // LDS and hands the result to the moved-bins sort (cfg5: 82 of 8 192 bins move then) instead of sorting 8 192
                // bins from scratch -- when most threads' bins descend; a topic of equal lags is in order as it stands.
                if (q == 1 && use_sample && a.no_moved_sort == 0 && a.no_sample_sort == 0) {
                    uint32_t* desc_threads = L.moved + 212;
                    if (tid == 0) *desc_threads = 0;
                    lds_barrier();
                    uint64_t v[EC];
                    bool desc = true;
#pragma unroll
                    for (int r = 0; r < EC; ++r) v[r] = p64_value(rec[r]);
#pragma unroll
                    for (int r = 1; r < EC; ++r) desc &= v[r - 1] > v[r];
                    desc &= tid * EC + EC <= C;
                    const uint64_t votes = __builtin_amdgcn_ballot_w64(desc);
                    if ((tid & 63) == 0 && votes) atomicAdd(desc_threads, (uint32_t)__builtin_popcountll(votes));
#pragma unroll
                    for (int r = 0; r < EC; ++r) s_bin[tid * EC + r] = v[r];
                    lds_barrier();
                    if (4u * *desc_threads >= 3u * (uint32_t)(C / EC)) {          // (workgroup-uniform)
#pragma unroll
                        for (int r = 0; r < EC; ++r) {
                            const int i = tid * EC + r;
                            if (i < C) rec[r] = p64_from(s_bin[C - 1 - i]);
                        }
                        next_moved = 1;
                    }
                    // (the moved-bins sort's first barrier stands between these reads and its writes to the same memory)
                }
            }
            if constexpr (EC >= 2) {
                // few bins move?  A topic that has the property has it round after round (the bulk of a power-law topic);
                // one that does not (lags spread like the totals) has every bin move in every round: after a look that
                // found more than twice what fits, the next one waits 1, 2, 4 .. 32 rounds.
                if (use_sample && a.no_moved_sort == 0 && q >= next_moved) {
                    int moved = 0;
                    sorted = moved_sort_bins<EC>(rec, L, tid, a.no_sample_sort == 2 ? 20u : kMovedBucket, &moved, moved_calls++);
                    moved_ = moved; if (sorted) path_ = 1;
                    if (sorted || moved <= 512 * EC) moved_wait = 0;
                    else moved_wait = moved_wait ? (moved_wait < 32 ? 2 * moved_wait : 32) : 1;
                    next_moved = q + 1 + moved_wait;
                }
                // few ascending runs?  The number of runs falls from round to round on the topics that have the property
                // and stays in the thousands on those that do not: look again after as many rounds as the last look
                // missed by (a factor of two per round is about what cfg5 does), every round once it has held.
                if (!sorted && use_sample && a.no_run_merge == 0 && q >= next_look) {
                    int runs = 0;
                    sorted = merge_runs_bins<EC>(rec, L, tid, &runs);
                    if (sorted) path_ = 2;
                    int wait = 0;
                    for (int x = runs; x > 2 * kMaxRuns && wait < 16; x >>= 1) ++wait;
                    next_look = q + 1 + wait;
                    if (!sorted) lds_barrier();              // (its LDS use ends before the sample sort's begins)
                }
                if (!sorted && use_sample) { sorted = sample_sort_bins<EC>(rec, L, tid, a.no_sample_sort == 2 ? 6u : kMaxBucket); if (sorted) path_ = 3; }
            }
            if (!sorted) {
                path_ = 4;
                // sort the n bins: inside every wavefront first, then merges across wavefronts
                // (workgroup_sort_p64 written out: called as the function, hipcc turns one branch of this kernel around)
                dpp_fence<EC>(rec);
                bitonic_sort_tile_p64<64, EC>(rec);
                ExchangeBufs xb{s_bin, n};
                for (int K = 2 * kSpan; K <= n; K <<= 1) {
                    cross_wave_step<EC>(rec, xb, tid, K - 1, K >> 1);                        // mirror: i <-> i ^ (K-1)
                    for (int j = K >> 2; j >= kSpan; j >>= 1) cross_wave_step<EC>(rec, xb, tid, j, j);
                    dpp_fence<EC>(rec);
                    clean_p64<64, EC, kSpan / 2, false>(rec);                                 // i <-> i ^ j, j < span
                }
                if (n > kSpan) lds_barrier();      // the last step's reads, before anything else goes over its buffer
            }
        }
        // position i of the sorted bins takes partition q*C + i; the next round's lags are fetched now
        LA_STAMP(q, path_, moved_);
        LA_CLK_START;
        // A thread's EC positions are consecutive (blocked layout), so are its keys and its results: 16 bytes per
        // instruction -- two keys per load, four results per store -- instead of one element each.  This kernel runs on
        // ONE CU, whose address path handled 16 narrow instructions per thread and round, 64 cache lines apiece.
        uint64_t next_lag[EC];
        if (narrow) {
            if constexpr (EC >= 4) {
                typedef uint32_t U32x4 __attribute__((ext_vector_type(4), aligned(16)));
                int64_t sb = (q + 1) * cpad + tid * EC;                          // a multiple of 4: 16-byte aligned
                sb = sb < cap8 ? sb : cap8;                                      // (past the topic: somewhere inside the buffer, never used)
#pragma unroll
                for (int r = 0; r < EC; r += 4) {
                    const U32x4 v = *reinterpret_cast<const U32x4*>(lag32 + sb + r);
                    next_lag[r] = v.x; next_lag[r + 1] = v.y; next_lag[r + 2] = v.z; next_lag[r + 3] = v.w;
                }
            }
        } else if constexpr (EC >= 2) {
            struct __attribute__((aligned(8))) U64x2 { uint64_t x, y; };
            // No branch around the loads, not even a uniform one (round 3 had `if (P >= 2)` here and hipcc put an
            // s_waitcnt vmcnt(0) between every two of them: four serialized round trips to L2 per round, ~2k cycles).  A
            // one-partition topic reads key[0 .. 1]: inside the buffer, whose size is rounded up to 256 bytes (sort_layout).
            const int64_t last_pair = P >= 2 ? P - 2 : 0;
#pragma unroll
            for (int r = 0; r < EC; r += 2) {
                const int64_t s = (q + 1) * C + tid * EC + r;
                const int64_t base = s < last_pair ? s : last_pair;              // the pair stays inside the array
                const U64x2 v = *reinterpret_cast<const U64x2*>(key + base);
                next_lag[r] = (base == s ? v.x : v.y) ^ kLagKeyFlip;        // s == P - 1: its key is the pair's second word
                next_lag[r + 1] = v.y ^ kLagKeyFlip;                        // (positions past P - 1 are never used)
            }
        } else {
            const int64_t s = (q + 1) * C + tid;
            next_lag[0] = key[s < P ? s : P - 1] ^ kLagKeyFlip;
        }
        int32_t who[EC];
        bool live[EC];
        if (EC >= 4 && C == n && (q + 1) * C <= P) {
            // a full round of a topic whose consumers fill every slot (cfg5: 127 of 128 rounds): every bin takes a partition
            // -- no predicates, no 64-bit position arithmetic, two 16-byte stores
#pragma unroll
            for (int r = 0; r < EC; ++r) {
                const uint64_t nb = p64_value(rec[r]) + (lag[r] << idx_bits);       // Main.java:265
                rec[r] = p64_from(nb);
                who[r] = (int32_t)((uint32_t)nb & idx_mask);
                lag[r] = next_lag[r];
            }
            if constexpr (EC >= 4) {
                if (narrow) {
                    // the thread's EC consumer indices as 16-bit words: one aligned store (two 16-byte stores of 32-bit words before)
                    typedef uint32_t U32xH __attribute__((ext_vector_type(EC / 2), aligned(2 * EC)));
                    U32xH v;
#pragma unroll
                    for (int r = 0; r < EC; r += 2) v[r / 2] = (uint32_t)who[r] | ((uint32_t)who[r + 1] << 16);
                    *reinterpret_cast<U32xH*>(idx16 + q * cpad + tid * EC) = v;
                } else {
                    typedef int I32x4 __attribute__((ext_vector_type(4), aligned(4)));
                    int32_t* dst = a.out_rank + a.p0 + q * C + tid * EC;
#pragma unroll
                    for (int r = 0; r < EC; r += 4) {
                        const I32x4 v4 = {who[r], who[r + 1], who[r + 2], who[r + 3]};
                        *reinterpret_cast<I32x4*>(dst + r) = v4;
                    }
                }
            }
            LA_CLK(6);
            continue;
        }
#pragma unroll
        for (int r = 0; r < EC; ++r) {
            const int i = tid * EC + r;
            const int64_t s = q * C + i;
            live[r] = i < C && s < P;
            const uint64_t nb = p64_value(rec[r]) + (lag[r] << idx_bits);       // Main.java:265
            if (live[r]) rec[r] = p64_from(nb);
            who[r] = (int32_t)((uint32_t)nb & idx_mask);    // consumer index; map_ranks_kernel turns it into the rank
            lag[r] = next_lag[r];
        }
        if (EC >= 4 && narrow) {
            if constexpr (EC >= 4) {
                uint16_t* dst = idx16 + q * cpad + tid * EC;
                if (live[EC - 1]) {                         // the last is live: so are all before it
                    typedef uint32_t U32xH __attribute__((ext_vector_type(EC / 2), aligned(2 * EC)));
                    U32xH v;
#pragma unroll
                    for (int r = 0; r < EC; r += 2) v[r / 2] = (uint32_t)who[r] | ((uint32_t)who[r + 1] << 16);
                    *reinterpret_cast<U32xH*>(dst) = v;
                } else {
#pragma unroll
                    for (int r = 0; r < EC - 1; ++r)
                        if (live[r]) dst[r] = (uint16_t)who[r];
                }
            }
        } else if constexpr (EC >= 4) {
            typedef int I32x4 __attribute__((ext_vector_type(4), aligned(4)));
#pragma unroll
            for (int r = 0; r < EC; r += 4) {
                int32_t* dst = a.out_rank + a.p0 + q * C + tid * EC + r;
                if (live[r + 3]) {                          // the fourth is live: so are the three before it
                    const I32x4 v = {who[r], who[r + 1], who[r + 2], who[r + 3]};
                    *reinterpret_cast<I32x4*>(dst) = v;
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (live[r + k]) dst[k] = who[r + k];
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < EC; ++r)
                if (live[r]) a.out_rank[a.p0 + q * C + tid * EC + r] = who[r];
        }
        LA_CLK(6);
    }
    LA_STAMP(rounds < 258 ? rounds : 258, 9, 0);
    if (a.out_total) {
#pragma unroll
        for (int r = 0; r < EC; ++r) {
            const uint64_t v = p64_value(rec[r]);
            const uint32_t who = (uint32_t)v & idx_mask;
            if (who < (uint32_t)C) a.out_total[a.c0 + who] = (int64_t)(v >> idx_bits);
        }
    }
}

// ---- kernel 3: round-structured greedy, one workgroup -----------------------------------------------
// n = EC * blockDim.x consumer slots (power of two >= C); slot i = tid*EC + r.
template <int EC>
__global__ __launch_bounds__(1024) void greedy_rounds_kernel(LargeArgs a0, SortBufs b0, const LargeItem* items, char* scratch,
                                                            const int32_t* order) {
    LA_PICK_ITEM(a, b, a0, b0, items, scratch, order[blockIdx.x])               // one workgroup per topic of this (EC, threads) class
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int tid = threadIdx.x;
    const int n = EC * blockDim.x;
    uint32_t* s_hi = smem;
    uint32_t* s_lo = smem + n;
    uint32_t* s_tb = smem + 2 * n;
    const uint64_t* key = key_buf(b, b.ctl->cur[kFinal]);
    const int64_t P = a.n_part;
    const int C = (int)a.n_cons;

    const int64_t rounds = (P + C - 1) / C;
    {
        // Packed bins (total << idx_bits) | index when nothing can overflow: the keys are sorted, so the
        // first one carries the largest lag and the last one the smallest (rounds_io).
        const RoundsIo io = rounds_io(a, key, P, C);
        if (io.idx_bits) {
            const uint32_t other = b.ctl->cur[kFinal] ^ 1u;
            greedy_rounds_packed<EC>(a, key, P, C, rounds, io.idx_bits, smem,
                                     io.narrow ? reinterpret_cast<const uint32_t*>(key_buf(b, other)) : nullptr,
                                     reinterpret_cast<uint16_t*>(val_buf(b, other)), io.cpad, io.zero_tail);
            return;
        }
    }
    Rec rec[EC];
#pragma unroll
    for (int r = 0; r < EC; ++r) {
        const int i = tid * EC + r;
        if (i < C) { rec[r].hi = (uint32_t)(kTotalBias >> 32); rec[r].lo = 0; rec[r].tb = (uint32_t)i; }
        else rec[r].hi = rec[r].lo = rec[r].tb = 0xFFFFFFFFu;
    }
    for (int64_t q = 0; q < rounds; ++q) {
        if (q > 0) {
            // bitonic sort of the n bins, ascending by (biased total, index)
            for (int k = 2; k <= n; k <<= 1) {
                for (int j = k >> 1; j >= 64 * EC; j >>= 1) {            // across waves: LDS
#pragma unroll
                    for (int r = 0; r < EC; ++r) {
                        const int i = tid * EC + r;
                        s_hi[i] = rec[r].hi; s_lo[i] = rec[r].lo; s_tb[i] = rec[r].tb;
                    }
                    __syncthreads();
#pragma unroll
                    for (int r = 0; r < EC; ++r) {
                        const int i = tid * EC + r;
                        Rec o;
                        o.hi = s_hi[i ^ j]; o.lo = s_lo[i ^ j]; o.tb = s_tb[i ^ j];
                        const bool keep_min = (((i & j) == 0) == ((i & k) == 0));
                        const bool take = (rec_less(o, rec[r]) == keep_min);
                        rec[r].hi = take ? o.hi : rec[r].hi;
                        rec[r].lo = take ? o.lo : rec[r].lo;
                        rec[r].tb = take ? o.tb : rec[r].tb;
                    }
                    __syncthreads();
                }
                for (int jl = 32; jl >= 1; jl >>= 1) {                    // across lanes: DPP
                    const int j = jl * EC;
                    if (j < k) {
#pragma unroll
                        for (int r = 0; r < EC; ++r) {
                            const int i = tid * EC + r;
                            cmpx_lanes_dyn(rec[r], jl, (((i & j) == 0) == ((i & k) == 0)));
                        }
                    }
                }
#pragma unroll
                for (int J = EC / 2; J >= 1; J >>= 1) {                   // inside the lane: registers
                    if (J < k) {
#pragma unroll
                        for (int r = 0; r < EC; ++r)
                            if ((r & J) == 0) cmpx_regs(rec[r], rec[r | J], ((tid * EC + r) & k) == 0);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < EC; ++r) {
            const int k = tid * EC + r;
            const int64_t s = q * C + k;
            if (k < C && s < P) {
                const uint64_t lag = key[s] ^ kLagKeyFlip;
                const uint64_t t = (((uint64_t)rec[r].hi << 32) | rec[r].lo) + lag;      // Main.java:265
                rec[r].hi = (uint32_t)(t >> 32);
                rec[r].lo = (uint32_t)t;
                a.out_rank[a.p0 + s] = (int32_t)rec[r].tb;                       // consumer index, as above
            }
        }
    }
    if (a.out_total) {
#pragma unroll
        for (int r = 0; r < EC; ++r)
            if (rec[r].tb < (uint32_t)C)
                a.out_total[a.c0 + rec[r].tb] = (int64_t)((((uint64_t)rec[r].hi << 32) | rec[r].lo) ^ kTotalBias);
    }
}

// ---- kernel 3, literal form: bins in LDS, wavefront argmin per partition ------------------------------
__global__ __launch_bounds__(1024) void greedy_argmin_kernel(LargeArgs a, SortBufs b) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int C = (int)a.n_cons;
    uint32_t* s_cnt = smem;                 // assigned count per bin
    uint32_t* s_hi = smem + C;              // biased assigned lag, high / low dword
    uint32_t* s_lo = smem + 2 * C;
    uint32_t* w_best = smem + 3 * C;        // [16 waves][4]
    const uint64_t* key = b.key[b.ctl->cur[kFinal]];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    for (int i = tid; i < C; i += blockDim.x) { s_cnt[i] = 0; s_hi[i] = (uint32_t)(kTotalBias >> 32); s_lo[i] = 0; }
    __syncthreads();
    for (int64_t s = 0; s < a.n_part; ++s) {
        uint32_t bc = 0xFFFFFFFFu;
        Rec best; best.hi = best.lo = best.tb = 0xFFFFFFFFu;
        for (int i = tid; i < C; i += blockDim.x) {          // comparator of Main.java:243-261
            Rec c; c.hi = s_hi[i]; c.lo = s_lo[i]; c.tb = (uint32_t)i;
            const uint32_t cc = s_cnt[i];
            const bool take = (cc < bc) | ((cc == bc) & rec_less(c, best));
            bc = take ? cc : bc; best.hi = take ? c.hi : best.hi; best.lo = take ? c.lo : best.lo;
            best.tb = take ? c.tb : best.tb;
        }
        for (int j = 1; j < 64; j <<= 1) {                   // wavefront argmin
            const Rec o = shfl_xor_dyn(best, j);
            const uint32_t oc = (uint32_t)__shfl_xor((int)bc, j);
            const bool take = (oc < bc) | ((oc == bc) & rec_less(o, best));
            bc = take ? oc : bc; best.hi = take ? o.hi : best.hi; best.lo = take ? o.lo : best.lo;
            best.tb = take ? o.tb : best.tb;
        }
        if (lane == 0) { w_best[wave * 4] = bc; w_best[wave * 4 + 1] = best.hi; w_best[wave * 4 + 2] = best.lo; w_best[wave * 4 + 3] = best.tb; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < nw; ++w) {
                Rec o; o.hi = w_best[w * 4 + 1]; o.lo = w_best[w * 4 + 2]; o.tb = w_best[w * 4 + 3];
                const uint32_t oc = w_best[w * 4];
                const bool take = (oc < bc) | ((oc == bc) & rec_less(o, best));
                if (take) { bc = oc; best = o; }
            }
            const uint32_t m = best.tb;
            const uint64_t t = (((uint64_t)s_hi[m] << 32) | s_lo[m]) + (key[s] ^ kLagKeyFlip);
            s_hi[m] = (uint32_t)(t >> 32);
            s_lo[m] = (uint32_t)t;
            s_cnt[m] += 1;
            a.out_rank[a.p0 + s] = a.cons_rank[a.c0 + m];
        }
        __syncthreads();
    }
    if (a.out_total)
        for (int i = tid; i < C; i += blockDim.x)
            a.out_total[a.c0 + i] = (int64_t)((((uint64_t)s_hi[i] << 32) | s_lo[i]) ^ kTotalBias);
}

// The rounds kernels store the chosen consumer's INDEX (position in the topic's rank-sorted list): looking the rank up
// there would put a dependent global load into every round of the one-workgroup chain (~6 us of 27 per round at
// 8 192 consumers).  This pass, over all CUs, turns the indices into member ranks.
__global__ __launch_bounds__(256) void map_ranks_kernel(LargeArgs a0, SortBufs b0, const LargeItem* items, char* scratch) {
    LA_PICK_ITEM(a, b, a0, b0, items, scratch, blockIdx.y)
    if (a.n_cons == 0) return;                                         // emit_ids_kernel wrote -1: no index to map
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint32_t fin = b.ctl->cur[kFinal];
    const RoundsIo io = rounds_io(a, key_buf(b, fin), a.n_part, a.n_cons, true);
    if (io.narrow) {
        // the rounds kernel left 16-bit consumer indices, every round's stretch on a multiple of 8 (rounds_io)
        const uint16_t* idx16 = reinterpret_cast<const uint16_t*>(val_buf(b, fin ^ 1u));
        const uint32_t C32 = (uint32_t)a.n_cons;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_part; i += stride) {
            const uint32_t q = (uint32_t)i / C32;
            a.out_rank[a.p0 + i] = a.cons_rank[a.c0 + idx16[(int64_t)q * io.cpad + ((uint32_t)i - q * C32)]];
        }
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_part; i += stride)
        a.out_rank[a.p0 + i] = a.cons_rank[a.c0 + a.out_rank[a.p0 + i]];
}

// `items` null: ONE topic (a, b).  Otherwise `count` topics of this (EC, threads) class, one workgroup each, side by side:
// the chain of rounds is serial inside a topic and independent across topics (Main.java:177-184).
template <int EC>
hipError_t launch_rounds(const LargeArgs& a, const SortBufs& b, int threads, hipStream_t stream, const LargeItem* items = nullptr,
                         char* scratch = nullptr, const int32_t* order = nullptr, int count = 1) {
    // packed bins: two exchange buffers of 8 B per bin; 96-bit bins: 12 B per bin; sample sort (EC >= 2): its own layout
    size_t lds = (size_t)4 * EC * threads * sizeof(uint32_t);
    if (EC >= 2 && sample_lds_bytes(EC) > lds) lds = sample_lds_bytes(EC);
    static PerDeviceOnce lds_opt_in;
    const hipError_t e = lds_opt_in.run([] {
        return hipFuncSetAttribute((const void*)greedy_rounds_kernel<EC>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   160 * 1024);
    });
    if (e != hipSuccess) return e;
    LA_LAUNCH((greedy_rounds_kernel<EC>), dim3(count), dim3(threads), lds, stream, a, b, items, scratch, order);
    if (!items)
        LA_LAUNCH(map_ranks_kernel, dim3(grid_256(a.n_part)), dim3(256), 0, stream, a, b, (const LargeItem*)nullptr, (char*)nullptr);
    return hipGetLastError();
}

// (EC, threads) of the rounds kernel for a topic with n_cons consumers (1 <= n_cons <= kLargeMaxConsumers)
__host__ __device__ inline void rounds_class(int64_t n_cons, int* ec, int* threads) {
    int cp2 = 64;
    while (cp2 < n_cons) cp2 <<= 1;
    if (cp2 <= 1024) { *ec = 1; *threads = cp2; }
    else { *ec = cp2 / 1024 >= 8 ? 8 : cp2 / 1024; *threads = 1024; }
}

inline hipError_t launch_rounds_class(int ec, int threads, const LargeArgs& a, const SortBufs& b, hipStream_t stream,
                                      const LargeItem* items = nullptr, char* scratch = nullptr, const int32_t* order = nullptr,
                                      int count = 1) {
    switch (ec) {
        case 1: return launch_rounds<1>(a, b, threads, stream, items, scratch, order, count);
        case 2: return launch_rounds<2>(a, b, threads, stream, items, scratch, order, count);
        case 4: return launch_rounds<4>(a, b, threads, stream, items, scratch, order, count);
        default: return launch_rounds<8>(a, b, threads, stream, items, scratch, order, count);
    }
}

}  // namespace

// no partition metadata: every subscribed consumer still reports a total of 0 (Main.java:216-225, :283-291)
static hipError_t zero_totals(const LargeArgs& a, hipStream_t stream) {
    if (a.n_cons > 0 && a.out_total) return hipMemsetAsync(a.out_total + a.c0, 0, (size_t)a.n_cons * sizeof(int64_t), stream);
    return hipSuccess;
}

// The phase events of the first large sort of a call that asked for them (LargeProfile): ev[0] at begin(), ev[1] and ev[2]
// where the launcher says, ev[3] on every way out.
struct ProfileScope {
    LargeProfile& pf;
    hipStream_t stream;
    bool on = false;
    hipError_t begin(int64_t n) {
        if (!pf.armed || pf.recorded) return hipSuccess;
        hipError_t e;
        for (hipEvent_t& ev : pf.ev)
            if (!ev && (e = hipEventCreate(&ev)) != hipSuccess) return e;
        pf.n = n;
        pf.recorded = true;
        on = true;
        mark(0);
        return hipSuccess;
    }
    hipEvent_t event(int i) const { return on ? pf.ev[i] : nullptr; }
    void mark(int i) { if (on) (void)hipEventRecord(pf.ev[i], stream); }
    ~ProfileScope() { mark(3); }
};

hipError_t large_topic_launch(LargeScratch& scratch, const LargeArgs& a, bool argmin, hipStream_t stream) {
    const int64_t n = a.n_part;
    if (n <= 0) return zero_totals(a, stream);
    if (n > 0x7FFFFFFF || a.n_cons > kLargeMaxConsumers) return hipErrorInvalidValue;
    SortBufs b{};
    hipError_t e;
    if ((e = sort_prepare(scratch, n, stream, &b, a.sort_multi_kernel != 0, true)) != hipSuccess) return e;
    ProfileScope prof{scratch.prof, stream};
    if ((e = prof.begin(n)) != hipSuccess) return e;
    if ((e = sort_launch(a, sort_job_single(b, bounds_pass_mask(a), a.status), stream, prof.event(1))) != hipSuccess) return e;
    prof.mark(2);
    LargeArgs al = a;
    al.rounds_follow = argmin ? 0 : 1;
    LA_LAUNCH(emit_ids_kernel, dim3(grid_256(n)), dim3(256), 0, stream, al, b, (const LargeItem*)nullptr, (char*)nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.n_cons == 0) return hipSuccess;

    if (argmin) {
        const int C = (int)a.n_cons;
        int threads = 64;
        while (threads < C && threads < 1024) threads <<= 1;
        const size_t lds = sizeof(uint32_t) * ((size_t)3 * C + 16 * 4);
        static PerDeviceOnce lds_opt_in;
        if ((e = lds_opt_in.run([] {
                 return hipFuncSetAttribute((const void*)greedy_argmin_kernel,
                                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
             })) != hipSuccess)
            return e;
        LA_LAUNCH(greedy_argmin_kernel, dim3(1), dim3(threads), lds, stream, a, b);
        return hipGetLastError();
    }
    int ec = 1, threads = 64;
    rounds_class(a.n_cons, &ec, &threads);
    return launch_rounds_class(ec, threads, al, b, stream);
}

hipError_t large_topics_launch(LargeScratch& scratch, const LargeArgs* args, int count, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipError_t e;
    std::vector<SortLayout> lay((size_t)count);
    bool serial = count == 1;
    for (int i = 0; i < count; ++i) {
        if (args[i].n_part <= 0 || args[i].n_part > 0x7FFFFFFF || args[i].n_cons > kLargeMaxConsumers) return hipErrorInvalidValue;
        lay[(size_t)i] = sort_layout(args[i].n_part, args[i].sort_multi_kernel != 0, true);
        serial = serial || lay[(size_t)i].multi_kernel;
    }
    if (serial) {
        for (int i = 0; i < count; ++i)
            if ((e = large_topic_launch(scratch, args[i], false, stream)) != hipSuccess) return e;
        return hipSuccess;
    }
    // items in tile-class order (every class a contiguous range for the pass launches; stable: the call's first large topic
    // of the first class sits at offset 0, where large_profile_read looks for a control block)
    std::vector<int> idx((size_t)count);
    for (int i = 0; i < count; ++i) idx[(size_t)i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return lay[(size_t)x].sweep_threads < lay[(size_t)y].sweep_threads; });
    size_t zero = 0, data = 0;
    std::vector<size_t> zoff((size_t)count), doff((size_t)count);
    for (int j = 0; j < count; ++j) {
        const SortLayout& L = lay[(size_t)idx[(size_t)j]];
        zoff[(size_t)j] = zero; zero += L.zero_bytes;
        doff[(size_t)j] = data; data += L.data_bytes;
    }
    if ((e = scratch_reserve(scratch, zero + data, stream)) != hipSuccess) return e;
    char* base = (char*)scratch.buf;

    // the argument blocks + the greedy's order list (topics grouped by the (EC, threads) class of their rounds kernel)
    const size_t items_bytes = align_up(sizeof(LargeItem) * (size_t)count, 256), bytes = items_bytes + sizeof(int32_t) * (size_t)count;
    LargeScratch::Stage& sg = scratch.stage[scratch.stage_next++ & 1u];
    if (sg.done) { if ((e = hipEventSynchronize(sg.done)) != hipSuccess) return e; }
    else if ((e = hipEventCreateWithFlags(&sg.done, hipEventDisableTiming)) != hipSuccess) return e;
    if (sg.cap < bytes) {
        if (sg.h) { (void)hipHostFree(sg.h); sg.h = nullptr; sg.cap = 0; }
        if ((e = hipHostMalloc(&sg.h, bytes + bytes / 2, hipHostMallocDefault)) != hipSuccess) return e;
        sg.cap = bytes + bytes / 2;
    }
    if (scratch.d_items_cap < bytes) {
        if (scratch.d_items) {
            if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
            (void)hipFree(scratch.d_items);
            scratch.d_items = nullptr; scratch.d_items_cap = 0;
        }
        if ((e = hipMalloc(&scratch.d_items, bytes + bytes / 2)) != hipSuccess) return e;
        scratch.d_items_cap = bytes + bytes / 2;
    }
    LargeItem* h_items = (LargeItem*)sg.h;
    int32_t* h_order = (int32_t*)((char*)sg.h + items_bytes);
    // job.b: what is common to a launch's items besides their buffers
    SortJob job{};
    job.b.atomic_rank = large_atomic_rank_supported();
    job.count = count;
    job.base = base;
    for (int j = 0; j < count; ++j) {
        const int i = idx[(size_t)j];
        const SortLayout& L = lay[(size_t)i];
        LargeItem& it = h_items[j];
        it.p0 = args[i].p0; it.n_part = args[i].n_part; it.c0 = args[i].c0; it.n_cons = args[i].n_cons;
        it.n = L.n; it.n_tiles = L.n_tiles; it.n_groups = L.n_groups;
        const uint64_t z = zoff[(size_t)j], d = zero + doff[(size_t)j];
        it.o_ctl = z + L.o_ctl; it.o_hist = z + L.o_hist; it.o_ticket = z + L.o_ticket; it.o_state = z + L.o_state;
        it.o_gbase = d + L.o_gbase; it.o_k0 = d + L.o_k0; it.o_k1 = d + L.o_k1; it.o_v0 = d + L.o_v0; it.o_v1 = d + L.o_v1;
        it.o_samp = L.keys_first ? z + L.o_samp : 0;               // (z + o_samp > 0: the control block comes first)
        it.o_flag = z + L.o_flag;
        it.samp_bits = L.samp_bits; it.pad = 0;
        job.keys_first = job.keys_first || L.keys_first != 0;
        if (L.keys_first == 2) job.b.keys_first_force = 1;
        if (L.n > job.max_n) job.max_n = L.n;
        if (job.n_cls == 0 || job.cls[job.n_cls - 1].sweep_threads != L.sweep_threads)
            job.cls[job.n_cls++] = SortClass{j, 0, L.sweep_threads, 0};
        SortClass& k = job.cls[job.n_cls - 1];
        ++k.n;
        if (L.n_tiles > k.max_tiles) k.max_tiles = L.n_tiles;
    }
    struct Cls { int ec, threads, first, n; };
    std::vector<Cls> cls;
    {
        std::vector<int> with;                                     // items that have consumers, by (EC, threads)
        for (int j = 0; j < count; ++j) if (h_items[j].n_cons > 0) with.push_back(j);
        auto key = [&](int j) { int ec, th; rounds_class(h_items[j].n_cons, &ec, &th); return ec * 2048 + th; };
        std::stable_sort(with.begin(), with.end(), [&](int x, int y) { return key(x) < key(y); });
        for (size_t k = 0; k < with.size(); ++k) {
            h_order[k] = with[k];
            int ec, th;
            rounds_class(h_items[with[k]].n_cons, &ec, &th);
            if (cls.empty() || cls.back().ec != ec || cls.back().threads != th) cls.push_back({ec, th, (int)k, 0});
            ++cls.back().n;
        }
    }
    if ((e = hipMemcpyAsync(scratch.d_items, sg.h, bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    (void)hipEventRecord(sg.done, stream);
    const LargeItem* d_items = (const LargeItem*)scratch.d_items;
    const int32_t* d_order = (const int32_t*)((const char*)scratch.d_items + items_bytes);
    if ((e = hipMemsetAsync(base, 0, zero, stream)) != hipSuccess) return e;

    ProfileScope prof{scratch.prof, stream};
    if ((e = prof.begin(h_items[0].n_part)) != hipSuccess) return e;
    // a0: the batch's arrays and flags, shared by every item (an item overrides the four segment fields)
    LargeArgs a0 = args[0];
    job.items = d_items;
    job.pass_mask = bounds_pass_mask(a0);
    job.status = a0.status;
    if ((e = sort_launch(a0, job, stream, prof.event(1))) != hipSuccess) return e;
    prof.mark(2);
    const SortBufs& b0 = job.b;
    const int gx = keys_grid(job.max_n);
    a0.rounds_follow = 1;
    LA_LAUNCH(emit_ids_kernel, dim3(gx, count), dim3(256), 0, stream, a0, b0, d_items, base);
    for (const Cls& c : cls)
        if ((e = launch_rounds_class(c.ec, c.threads, a0, b0, stream, d_items, base, d_order + c.first, c.n)) != hipSuccess) return e;
    if (!cls.empty()) LA_LAUNCH(map_ranks_kernel, dim3(gx, count), dim3(256), 0, stream, a0, b0, d_items, base);
    return hipGetLastError();
}

// ---- more consumers than one workgroup's registers hold (> kLargeMaxConsumers): bins in HBM -------------------------------
// Collections.min over the bins takes any C (Main.java:240-263).  The round structure still holds: in round r the k-th
// sorted partition of the round goes to the k-th bin in (total, member) order as of the round start -- so a round is ONE
// stable device sort of the C bins by total (payload = consumer index, ascending on input: ties keep member order) with the
// radix passes above, and one pass that hands the round's lags out in that order.  ceil(P / C) rounds of ~11 launches:
// slow next to the one-workgroup kernels (which stop at 8 192 bins), exact, and without a limit.
//   huge_round_kernel   position k of the current order: total += lag of the round's k-th partition, member rank out; the
//                       new total goes to slot `consumer index` of the next sort's input, with its digit histograms.
namespace {

__global__ __launch_bounds__(256) void huge_round_kernel(LargeArgs a, SortBufs parts, SortBufs cur, SortBufs next, int64_t round,
                                                         int first, int last) {
    __shared__ uint32_t h[8 * kRadix];
    for (int i = threadIdx.x; i < 8 * kRadix; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const int64_t C = a.n_cons, P = a.n_part;
    const uint64_t* lagkey = parts.key[parts.ctl->cur[kFinal]];
    const uint32_t fin = first ? 0u : cur.ctl->cur[kFinal];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < C; k += stride) {
        uint64_t total = kTotalBias;                                  // biased: unsigned order = Java's signed order
        uint32_t idx = (uint32_t)k;
        if (!first) { total = cur.key[fin][k]; idx = cur.val[fin][k]; }
        const int64_t s = round * C + k;
        if (s < P) {
            total += lagkey[s] ^ kLagKeyFlip;                         // Main.java:265, wrapping like a long
            a.out_rank[a.p0 + s] = a.cons_rank[a.c0 + idx];
        }
        if (last) {
            if (a.out_total) a.out_total[a.c0 + idx] = (int64_t)(total ^ kTotalBias);
        } else {
            next.key[0][idx] = total;
            next.val[0][idx] = idx;
#pragma unroll
            for (int d = 0; d < 8; ++d) atomicAdd(&h[d * kRadix + ((uint32_t)(total >> (8 * d)) & 0xFFu)], 1u);
        }
    }
    if (last) return;
    __syncthreads();
    for (int i = threadIdx.x; i < 8 * kRadix; i += blockDim.x)
        if (h[i]) atomicAdd(&next.hist[4 * kRadix + i], h[i]);
    // the id digits: the payload is ascending (slot = consumer index), the plan skips their passes
    if (blockIdx.x == 0 && threadIdx.x < 4) next.hist[threadIdx.x * kRadix] = (uint32_t)C;
}

}  // namespace

hipError_t huge_topic_launch(LargeScratch& scratch, const LargeArgs& a, hipStream_t stream) {
    const int64_t P = a.n_part, C = a.n_cons;
    if (P <= 0) return zero_totals(a, stream);
    if (P > 0x7FFFFFFF || C > 0x7FFFFFFF || C <= 0) return hipErrorInvalidValue;
    const SortLayout lp = sort_layout(P, a.sort_multi_kernel != 0, true), lc = sort_layout(C, false);
    hipError_t e;
    const size_t zero = lp.zero_bytes + 2 * lc.zero_bytes, data = lp.data_bytes + 2 * lc.data_bytes;
    if ((e = scratch_reserve(scratch, zero + data, stream)) != hipSuccess) return e;
    char* base = (char*)scratch.buf;
    const SortBufs bp = sort_bind(lp, base, base + zero);
    SortBufs bins[2] = {sort_bind(lc, base + lp.zero_bytes, base + zero + lp.data_bytes),
                        sort_bind(lc, base + lp.zero_bytes + lc.zero_bytes, base + zero + lp.data_bytes + lc.data_bytes)};
    if ((e = hipMemsetAsync(base, 0, lp.zero_bytes, stream)) != hipSuccess) return e;
    if ((e = sort_launch(a, sort_job_single(bp, kAllPasses, a.status), stream, nullptr)) != hipSuccess) return e;
    LA_LAUNCH(emit_ids_kernel, dim3(keys_grid(P)), dim3(256), 0, stream, a, bp, (const LargeItem*)nullptr, (char*)nullptr);
    const int cgrid = grid_256(C, 1024);
    const int64_t rounds = (P + C - 1) / C;
    for (int64_t r = 0; r < rounds; ++r) {
        const SortBufs& cur = bins[r & 1];
        const SortBufs& next = bins[(r + 1) & 1];
        const int last = r + 1 == rounds;
        if (!last && (e = hipMemsetAsync((char*)next.ctl, 0, lc.zero_bytes, stream)) != hipSuccess) return e;
        LA_LAUNCH(huge_round_kernel, dim3(cgrid), dim3(256), 0, stream, a, bp, cur, next, r, r == 0 ? 1 : 0, last);
        if (!last) sort_plan_and_passes(sort_job_single(next, 0xFF0u, a.status), stream, nullptr);   // the 8 digits of the totals; ids stay in order
    }
    return hipGetLastError();
}

// ---- lab builds: the rounds' instrumentation arrays (debug_read, la_launch.h) -------------------------------------------------
#ifdef LA_ROUND_CLOCKS
LA_DEBUG_EXPORT la_debug_round_stamps(unsigned long long* out) { return debug_read(g_round_stamp, out, 0); }
LA_DEBUG_EXPORT la_debug_round_clocks(unsigned long long* out, int reset) { return debug_read(g_round_clocks, out, reset); }
#endif

void large_scratch_release(LargeScratch& s) {
    if (s.buf) (void)hipFree(s.buf);
    s.buf = nullptr;
    s.cap = 0;
    for (LargeScratch::Stage& sg : s.stage) {
        if (sg.done) { (void)hipEventSynchronize(sg.done); (void)hipEventDestroy(sg.done); sg.done = nullptr; }
        if (sg.h) (void)hipHostFree(sg.h);
        sg.h = nullptr;
        sg.cap = 0;
    }
    if (s.d_items) (void)hipFree(s.d_items);
    s.d_items = nullptr;
    s.d_items_cap = 0;
    for (hipEvent_t& ev : s.prof.ev) {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
    }
}

hipError_t large_profile_read(LargeScratch& s, float* ms, int* passes, int64_t* n) {
    if (!s.prof.recorded || !s.buf) return hipErrorNotReady;
    hipError_t e;
    if ((e = hipEventSynchronize(s.prof.ev[3])) != hipSuccess) return e;
    for (int i = 0; i < 3; ++i)
        if ((e = hipEventElapsedTime(&ms[i], s.prof.ev[i], s.prof.ev[i + 1])) != hipSuccess) return e;
    SortCtl ctl;                                    // the control block sits at the start of the scratch
    if ((e = hipMemcpy(&ctl, s.buf, sizeof ctl, hipMemcpyDeviceToHost)) != hipSuccess) return e;
    passes[0] = passes[1] = 0;
    for (int p = 0; p < kSlots; ++p)
        if (!ctl.skip[p]) ++passes[p % kDigits < 4 ? 0 : 1];
    passes[2] = (int)ctl.keys_first;
    passes[3] = (int)ctl.redo;
    *n = s.prof.n;
    return hipSuccess;
}

}  // namespace la
