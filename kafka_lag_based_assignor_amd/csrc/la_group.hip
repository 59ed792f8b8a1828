// la_group.hip -- la_group_by_member: the assignment's entries as every member's list, a STABLE grouping by member rank in
// three size classes.  In file order:
//
//   one workgroup     group_small_kernel: up to kSmallGroupN entries, the counting sort of la_group_small.h in LDS.
//   several           group_mid_count_kernel / group_mid_place_kernel: up to kMidBlock x kMidMaxBlocks entries and few
//   workgroups        members, the same counting sort split over workgroups, two launches.
//   radix form        anything beyond: member_keys_kernel, the radix passes of la_radix.hip (sort_plan_and_passes) over the
//                     digits the member count leaves possible, member_emit_kernel.
//   host              group_by_member_launch picks the class.
//   read-outs         the lab builds' instrumentation array of the one-workgroup form (la_debug_group_clocks).
//
// Environment hooks, read at every call (tests set them around live contexts): LA_NO_SMALL_GROUP, LA_NO_MID_GROUP
// (group_by_member_launch).
#include "la_radix.h"
#include "la_device.h"
#include "la_group_small.h"

namespace la {

// ---- what a real rebalance is: up to a few thousand entries, ONE workgroup (la_group_small.h) --------------------------------
__global__ __launch_bounds__(1024) void group_small_kernel(int n, int32_t n_members, int64_t n_topics, const int64_t* part_off,
                                                           const int32_t* out_partition, const int32_t* member_rank,
                                                           int64_t* member_off, int32_t* grouped_topic,
                                                           int32_t* grouped_partition, int32_t* grouped_entry,
                                                           const uint32_t* fin_status, uint32_t* fin_flag) {
    __shared__ uint32_t start[kSmallGroupM];          // counts, then the groups' cursors
    __shared__ uint32_t wsum[1024 / kWave];
    __shared__ uint32_t turn;
    __shared__ int32_t s_in[7 * kSmallGroupN];        // ranks, ids, topics of the entries; the lists; the chunks' group leaders
    group_small_body_staged<1024, kSmallGroupM>(n, n_members, n_topics, part_off, out_partition, member_rank, member_off,
                                                grouped_topic, grouped_partition, grouped_entry, start, wsum, &turn, s_in,
                                                s_in + kSmallGroupN, s_in + 2 * kSmallGroupN, s_in + 3 * kSmallGroupN, s_in + 4 * kSmallGroupN,
                                                reinterpret_cast<uint32_t*>(s_in + 5 * kSmallGroupN),
                                                reinterpret_cast<uint32_t*>(s_in + 6 * kSmallGroupN));
    if (fin_flag) {
        // the last launch of a zero-copy call (la_host.hip, assign_small_zc): this ONE workgroup's stores into the host's memory
        // are out, then `done | status` goes where the calling thread is spinning -- no separate finishing launch
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(fin_flag, 0x80000000u | *fin_status, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- the same lists for a few thousand to 65 536 entries and FEW members: two launches -----------------------------------------
// Between the one-workgroup form (<= kSmallGroupN entries) and the radix form (five dependent launches, 17-25 us whatever the
// size) sits what a mid-size rebalance is: 3 000 - 65 000 partitions, a handful of members (10 000 entries: 85 -> 80 us per call).  With G = members + 2 <= kMidGroupM
// groups a table of per-block counts is small, and the stable counting sort splits over workgroups:
//   launch 1 (group_mid_count): block b = entries [b * kMidBlock, ...): the chunks' group leaders (ballots, as above) add their
//            peer counts into LDS counters; the block's G counts go to cnt[b][*];
//   launch 2 (group_mid_place): every block reads the whole table (blocks x G words), sums it per group (the groups' starts, an
//            exclusive scan) and over the blocks before it (its own first places), then places its entries exactly like the
//            one-workgroup form does -- ranks inside a chunk by ballots, cursors advanced chunk by chunk by in-order returning
//            LDS atomics -- and stores them straight to their places.  The topic of every entry: the block's first topic by a
//            256-ary search over part_off (two rounds up to 65 536 topics), the rest from the topic starts inside the block (+1
//            at a topic's first position, an inclusive scan).
// Stable by construction: blocks in order, chunks in order, lanes in order.
constexpr int kMidBlock = 2048;          // entries per workgroup
constexpr int kMidThreads = 256;
constexpr int kMidGroupM = 512;          // groups (members + 2) the table form holds
constexpr int kMidMaxBlocks = 32;        // 65 536 entries: every block sums the whole table (blocks x groups words); 125 blocks made it slower than the radix form

__device__ __forceinline__ void group_mid_chunk_ranks(int nb, uint32_t G, const int32_t* s_rank_in, int32_t* s_pk, uint32_t* lead,
                                                      uint32_t* counts, int lane, int wave) {
    constexpr int W = kMidThreads / kWave;
    const int nch = (nb + kWave - 1) / kWave;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (int c = wave; c < nch; c += W) {
        const int i = c * kWave + lane;
        const bool valid = i < nb;
        uint32_t gi = valid ? (uint32_t)(s_rank_in[i] + 1) : 0u;
        gi = gi < G ? gi : G;
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 10; ++bit) {                                // G <= kMidGroupM - 1 < 2^9 (+ the clamp value G itself)
            const bool one = (gi >> bit) & 1u;
            const uint64_t bal = __ballot(one);
            peers &= one ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & below), cnt = (uint32_t)__popcll(peers);
        const int leader = __ffsll((unsigned long long)peers) - 1;
        if (valid) {
            if (s_pk) s_pk[i] = (int32_t)(((uint32_t)leader << 16) | rank);
            if (lead) lead[i] = lane == leader ? ((gi << 8) | cnt) : 0u;
            if (lane == leader) atomicAdd(&counts[gi], cnt);
        }
    }
}

__global__ __launch_bounds__(kMidThreads) void group_mid_count_kernel(int n, int32_t n_members, const int32_t* member_rank, uint32_t* cnt) {
    __shared__ uint32_t counts[kMidGroupM];
    __shared__ int32_t s_rank[kMidBlock];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e0 = blockIdx.x * kMidBlock, nb = min(kMidBlock, n - e0);
    const uint32_t G = (uint32_t)n_members + 1;
    for (int k = tid; k < kMidGroupM; k += kMidThreads) counts[k] = 0;
    for (int i = tid; i < nb; i += kMidThreads) s_rank[i] = member_rank[e0 + i];
    __syncthreads();
    group_mid_chunk_ranks(nb, G, s_rank, nullptr, nullptr, counts, lane, wave);
    __syncthreads();
    for (uint32_t g = tid; g <= G; g += kMidThreads) cnt[(size_t)blockIdx.x * kMidGroupM + g] = counts[g];
    if (blockIdx.x == 0 && tid == 0) cnt[(size_t)gridDim.x * kMidGroupM] = 0;      // the place kernel's "blocks done" counter
}

__global__ __launch_bounds__(kMidThreads) void group_mid_place_kernel(int n, int32_t n_members, int64_t n_topics, const int64_t* part_off,
                                                                      const int32_t* out_partition, const int32_t* member_rank,
                                                                      uint32_t* cnt, int64_t* member_off, int32_t* grouped_topic,
                                                                      int32_t* grouped_partition, int32_t* grouped_entry,
                                                                      const uint32_t* status, uint32_t* fin_flag) {
    __shared__ uint32_t cursor[kMidGroupM];           // this block's first place of every group, then its cursors
    __shared__ uint32_t counts[kMidGroupM];           // (scratch of the chunk ranks: the block's own counts again)
    __shared__ uint32_t wsum[kMidThreads / kWave];
    __shared__ int32_t s_rank[kMidBlock], s_pk[kMidBlock], s_topic[kMidBlock];
    __shared__ uint32_t lead[kMidBlock], first[kMidBlock];
    __shared__ int s_t0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int W = kMidThreads / kWave;
    const int nblocks = gridDim.x;
    const int e0 = blockIdx.x * kMidBlock, nb = min(kMidBlock, n - e0), e1 = e0 + nb;
    const uint32_t G = (uint32_t)n_members + 1;
    // inputs (independent loads first), the table's column sums
    for (int i = tid; i < nb; i += kMidThreads) { s_rank[i] = member_rank[e0 + i]; s_topic[i] = 0; }
    for (int k = tid; k < kMidGroupM; k += kMidThreads) counts[k] = 0;
    uint32_t tot[kMidGroupM / kMidThreads], mine[kMidGroupM / kMidThreads];     // groups tid, tid + 256
#pragma unroll
    for (int r = 0; r < kMidGroupM / kMidThreads; ++r) {
        const uint32_t g = (uint32_t)(tid + r * kMidThreads);
        uint32_t all = 0, before = 0;
        if (g <= G)
            for (int b = 0; b < nblocks; ++b) {
                const uint32_t c = cnt[(size_t)b * kMidGroupM + g];
                all += c;
                before += b < (int)blockIdx.x ? c : 0u;
            }
        tot[r] = all;
        mine[r] = before;
    }
    // exclusive scan of the groups' totals over g (group g = tid + r * 256: scan the r = 0 half, then the r = 1 half behind it)
    uint32_t base_of[kMidGroupM / kMidThreads];
    uint32_t carry = 0;
#pragma unroll
    for (int r = 0; r < kMidGroupM / kMidThreads; ++r) {
        uint32_t incl = tot[r];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = carry, all = 0;
        for (int w = 0; w < W; ++w) { before += w < wave ? wsum[w] : 0u; all += wsum[w]; }
        base_of[r] = before + incl - tot[r];
        carry += all;
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < kMidGroupM / kMidThreads; ++r) {
        const uint32_t g = (uint32_t)(tid + r * kMidThreads);
        cursor[g] = base_of[r] + mine[r];
        // member m's list starts where the groups 0 .. m end: member_off[m] = start of group m + 1
        if (blockIdx.x == 0 && g >= 1 && g <= (uint32_t)n_members + 1) member_off[g - 1] = (int64_t)base_of[r];
    }
    // the block's first topic: the largest t with part_off[t] <= e0, by a 256-ary search
    if (grouped_topic) {
        int64_t lo = 0, hi = n_topics;                                       // invariant: part_off[lo] <= e0 (part_off[0] = 0), answer in [lo, hi)
        while (hi - lo > 1) {
            const int64_t step = (hi - lo + kMidThreads - 1) / kMidThreads;
            if (tid == 0) s_t0 = 0;
            __syncthreads();
            const int64_t at = lo + (int64_t)tid * step;
            if (at < hi && part_off[at] <= (int64_t)e0) atomicMax(&s_t0, tid);
            __syncthreads();
            const int64_t nlo = lo + (int64_t)s_t0 * step;
            hi = nlo + step < hi ? nlo + step : hi;
            lo = nlo;
            __syncthreads();
        }
        const int64_t t0 = lo;
        for (int64_t t = t0 + 1 + tid; t < n_topics; t += kMidThreads) {   // topic starts inside the block
            const int64_t at = part_off[t];
            if (at >= (int64_t)e1) break;
            atomicAdd((uint32_t*)&s_topic[at - e0], 1u);
        }
        __syncthreads();
        constexpr int PERT = kMidBlock / kMidThreads;
        uint32_t tv[PERT], trun = 0;
#pragma unroll
        for (int r = 0; r < PERT; ++r) {
            const int i = PERT * tid + r;
            tv[r] = i < nb ? (uint32_t)s_topic[i] : 0u;
            trun += tv[r];
        }
        uint32_t tincl = trun;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(tincl, o);
            if (lane >= o) tincl += y;
        }
        if (lane == 63) wsum[wave] = tincl;
        __syncthreads();
        uint32_t tbase = tincl - trun;
        for (int w = 0; w < wave; ++w) tbase += wsum[w];
#pragma unroll
        for (int r = 0; r < PERT; ++r) {
            const int i = PERT * tid + r;
            tbase += tv[r];
            if (i < nb) s_topic[i] = (int32_t)(t0 + tbase);
        }
    }
    __syncthreads();
    group_mid_chunk_ranks(nb, G, s_rank, s_pk, lead, counts, lane, wave);
    __syncthreads();
    {
        const int nch = (nb + kWave - 1) / kWave;
        constexpr int kAhead = 4;
        for (int c0 = 0; c0 < nch; c0 += kAhead) {
            uint32_t v[kAhead], f[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const int i = (c0 + u) * kWave + lane;
                v[u] = (c0 + u < nch && i < nb) ? lead[i] : 0u;
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const uint32_t c = v[u] & 0xFFu, g = v[u] >> 8;
                f[u] = 0;
                if (c != 0 && (g % W) == (uint32_t)wave) f[u] = atomicAdd(&cursor[g], c);
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const uint32_t c = v[u] & 0xFFu, g = v[u] >> 8;
                if (c != 0 && (g % W) == (uint32_t)wave) first[(c0 + u) * kWave + lane] = f[u];
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < nb; i += kMidThreads) {
        const uint32_t pk = (uint32_t)s_pk[i];
        const uint32_t pos = first[(i & ~(kWave - 1)) + (int)(pk >> 16)] + (pk & 0xFFFFu);
        grouped_partition[pos] = out_partition ? out_partition[e0 + i] : 0;
        if (grouped_topic) grouped_topic[pos] = s_topic[i];
        if (grouped_entry) grouped_entry[pos] = e0 + i;
    }
    if (fin_flag) {
        // a zero-copy call ends here (as in tile_tail): every block releases what it wrote -- the lists sit in host memory -- and
        // counts itself done; the last one stores `done | status` where the calling thread spins
        __threadfence_system();
        __syncthreads();
        if (tid == 0) {
            uint32_t* done = cnt + (size_t)gridDim.x * kMidGroupM;
            if (__hip_atomic_fetch_add(done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
                const uint32_t st = __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __threadfence_system();
                __hip_atomic_store(fin_flag, 0x80000000u | st, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

namespace {

// ---- the radix form: assignment -> per-member lists (the wrap step of Main.java:152-156, 171-174, 264) -------
// The reference appends to each member's list topic by topic, and inside a topic in assignment order: that is
// the order of the output arrays.  Grouping by member is therefore a STABLE sort of the entry indices by member
// rank: key = rank + 1 (0 = "topic had no consumers": those entries come first and are dropped), payload =
// entry index, already ascending, so only the key's ceil(log2(M+1)/8) digit passes run.
__global__ __launch_bounds__(256) void member_keys_kernel(const int32_t* member_rank, SortBufs b) {
    __shared__ uint32_t h[kDigits * kRadix];
    for (int i = threadIdx.x; i < kDigits * kRadix; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < b.n; base += stride) {
        const int64_t i = base + threadIdx.x;
        if (i < b.n) {
            const uint64_t key = (uint64_t)(uint32_t)(member_rank[i] + 1);
            b.key[0][i] = key;
            b.val[0][i] = (uint32_t)i;
#pragma unroll
            for (int p = 4; p < 8; ++p) atomicAdd(&h[p * kRadix + ((uint32_t)(key >> (8 * (p - 4))) & 0xFFu)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kDigits * kRadix; i += blockDim.x)
        if (h[i]) atomicAdd(&b.hist[i], h[i]);
    // digits the loop did not count: ids are ascending (skipped by the plan), key bits 32..63 are zero
    if (blockIdx.x == 0 && threadIdx.x < kDigits && (threadIdx.x < 4 || threadIdx.x >= 8))
        b.hist[threadIdx.x * kRadix] = (uint32_t)b.n;
}

// member_off[r] = first grouped position of member r (r = 0..M); grouped_* = the entries in grouped order
__global__ __launch_bounds__(256) void member_emit_kernel(SortBufs b, int32_t n_members, int64_t n_topics,
                                                          const int64_t* part_off, const int32_t* out_partition,
                                                          int64_t* member_off, int32_t* grouped_topic,
                                                          int32_t* grouped_partition, int32_t* grouped_entry, uint32_t* status) {
    const uint32_t fin = b.ctl->cur[kFinal];
    const uint64_t* key = b.key[fin];
    const uint32_t* val = b.val[fin];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= b.n; i += stride) {
        // boundaries: key k (= rank + 1) starts at the first i with key[i] >= k
        const int64_t k_prev = i > 0 ? (int64_t)key[i - 1] : 0;
        const int64_t k_here = i < b.n ? (int64_t)key[i] : (int64_t)n_members + 1;
        // the sort's result, checked on the way (see emit_ids_kernel): groups ascending, entry indices ascending inside a group
        if (i > 0 && i < b.n && status && (k_prev > k_here || (k_prev == k_here && val[i - 1] >= val[i])))
            atomicOr(status, kStatusOrder);
        for (int64_t k = k_prev + 1; k <= k_here; ++k)
            if (k >= 1 && k <= (int64_t)n_members + 1) member_off[k - 1] = i;
        if (i < b.n) {
            const uint32_t e = val[i];
            if (grouped_entry) grouped_entry[i] = (int32_t)e;
            if (grouped_partition) grouped_partition[i] = out_partition[e];
            if (grouped_topic) {
                int64_t lo = 0, hi = n_topics;                   // largest t with part_off[t] <= e
                while (hi - lo > 1) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (part_off[mid] <= (int64_t)e) lo = mid; else hi = mid;
                }
                grouped_topic[i] = (int32_t)lo;
            }
        }
    }
}

}  // namespace

hipError_t group_by_member_launch(LargeScratch& scratch, int64_t n, int32_t n_members, int64_t n_topics,
                                  const int64_t* part_off, const int32_t* out_partition, const int32_t* member_rank,
                                  int64_t* member_off, int32_t* grouped_topic, int32_t* grouped_partition,
                                  int32_t* grouped_entry, uint32_t* status, hipStream_t stream, uint32_t* fin_flag, bool* fin_done) {
    if (fin_done) *fin_done = false;
    if (n < 0 || n > 0x7FFFFFFF || n_members < 0) return hipErrorInvalidValue;
    hipError_t e;
    if (n == 0) return hipMemsetAsync(member_off, 0, sizeof(int64_t) * ((size_t)n_members + 1), stream);
    if (n <= kSmallGroupN && (int64_t)n_members + 2 <= kSmallGroupM && ((int64_t)n_members + 1) < ((int64_t)1 << (kSmallGroupBits + 1)) &&
        !getenv("LA_NO_SMALL_GROUP")) {
        LA_LAUNCH(group_small_kernel, dim3(1), dim3(1024), 0, stream, (int)n, n_members, n_topics, part_off, out_partition,
                           member_rank, member_off, grouped_topic, grouped_partition, grouped_entry, (const uint32_t*)status,
                           fin_flag);
        if (fin_done) *fin_done = fin_flag != nullptr;
        return hipGetLastError();
    }
    if (n <= (int64_t)kMidBlock * kMidMaxBlocks && (int64_t)n_members + 2 <= kMidGroupM && !getenv("LA_NO_MID_GROUP")) {
        // a mid-size rebalance with few members: the stable counting sort over several workgroups, two launches
        // instead of the radix form's five
        const int blocks = (int)((n + kMidBlock - 1) / kMidBlock);
        if ((e = scratch_reserve(scratch, ((size_t)blocks * kMidGroupM + 1) * sizeof(uint32_t), stream)) != hipSuccess) return e;
        uint32_t* cnt = (uint32_t*)scratch.buf;
        LA_LAUNCH(group_mid_count_kernel, dim3(blocks), dim3(kMidThreads), 0, stream, (int)n, n_members, member_rank, cnt);
        LA_LAUNCH(group_mid_place_kernel, dim3(blocks), dim3(kMidThreads), 0, stream, (int)n, n_members, n_topics, part_off, out_partition,
                  member_rank, cnt, member_off, grouped_topic, grouped_partition, grouped_entry, (const uint32_t*)status, fin_flag);
        if (fin_done) *fin_done = fin_flag != nullptr;
        return hipGetLastError();
    }
    SortBufs b{};
    if ((e = sort_prepare(scratch, n, stream, &b)) != hipSuccess) return e;
    const int grid = grid_256(n);
    LA_LAUNCH(member_keys_kernel, dim3(grid), dim3(256), 0, stream, member_rank, b);
    // key = rank + 1 <= n_members: only its low ceil(bits / 8) digits can differ; the payload (entry index) is ascending.
    // Launching just those passes matters for the small batches a real group leader sends: a skipped pass is still a
    // launch (four in the four-kernel form: ~50 launches, ~190 us, for a 100-partition rebalance).
    uint32_t mask = 0;
    for (int d = 0; d < 8 && ((uint64_t)n_members >> (8 * d)) != 0; ++d) mask |= 1u << (4 + d);
    sort_plan_and_passes(sort_job_single(b, mask, status), stream, nullptr);
    LA_LAUNCH(member_emit_kernel, dim3(grid), dim3(256), 0, stream, b, n_members, n_topics, part_off,
                       out_partition, member_off, grouped_topic, grouped_partition, grouped_entry, status);
    return hipGetLastError();
}

// ---- lab builds: the one-workgroup form's instrumentation array (la_group_small.h; debug_read, la_launch.h) -------------------
#ifdef LA_GROUP_CLOCKS
LA_DEBUG_EXPORT la_debug_group_clocks(unsigned long long* out, int reset) { return debug_read(g_group_clocks, out, reset); }
#endif

}  // namespace la
