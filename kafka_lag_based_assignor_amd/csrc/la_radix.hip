// la_radix.hip -- the device-wide radix sort of the large path, of the huge path's bins (la_large.hip) and of the grouping by
// member (la_group.hip); what its clients see of it is la_radix.h.  In file order:
//
//   keys and plan     build_keys_kernel: lag from offsets (Main.java:376-404), 64-bit sort key + 32-bit id, the 12 digit
//                     histograms of the 96-bit composite and a sample of the lags in one read; sample_scan_kernel: is some lag
//                     frequent?; plan_kernel: a pass whose digit is constant over the topic is skipped (lags < 2^40 with ids
//                     < 2^24 cost 8 passes, not 12; ids already ascending skip the 4 id passes), and whether the sort goes
//                     keys first.  The sort is an LSD radix sort, 8 bits per pass, stable, over (key64, id32): id digits, then
//                     key digits -> (lag desc, id asc), the comparator of Main.java:228-235.
//   two pass forms    four kernels per pass (tile_count, two scans, tile_scatter): n >= 2^30 and a test hook; ONE kernel per
//                     pass (onesweep_pass_kernel): stable scatter with decoupled look-back, ranks from returning LDS atomics
//                     where the device serves colliding lanes in lane order (lds_atomic_order_test_kernel), else by matching.
//   keys first        large topics with shuffled ids and no frequent lag sort by the key digits alone; tie_scan_kernel and
//                     tie_repair_kernel then put every run of equal lags in id order.  A run too long for one workgroup makes
//                     replan_kernel arm the redo slots: the same digits again, all in one launch (onesweep_redo_kernel);
//                     no-ops otherwise.
//   host              the atomic-rank check per device (large_init_device), sort layout and scratch, the pass launches
//                     (sort_passes), the tie repair (sort_repair_launch), the whole sort (sort_launch).
//   read-outs         the lab builds' instrumentation arrays (la_debug_sweep_clocks, la_debug_lookback_stats).
//
// Environment hooks.  Read at every call (tests set them around live contexts): LA_SORT_KEYS_FIRST, LA_SORT_MULTIKERNEL,
// LA_SWEEP_THREADS (sort_layout).  Read once per process: LA_SORT_RANK (large_init_device, per device).
#include "la_radix.h"
#include "la_device.h"
#include "la_sort64.h"

#include <type_traits>

namespace la {

namespace {

// Arrays that a kernel reads ONCE (the caller's inputs in build_keys_kernel, a pass's source buffers) as non-temporal loads
// (profiles/r06_ab_nt_loads.txt, profiles/r06_ad_nt_loads_large.txt).
template <typename T>
__device__ __forceinline__ T stream_load(const T* p) {
    return __builtin_nontemporal_load(p);
}

constexpr int kSortThreads = 256;
constexpr int kSortWaves = kSortThreads / kWave;
constexpr int kItems = 16;
constexpr int kTile = kSortThreads * kItems;     // 4096 elements per workgroup
constexpr int kScanRows = 32;                    // tiles per workgroup of the offset scan
constexpr uint32_t kSampleHeavy = 8;             // 1 in 256 keys is sampled: a counter at 8 ~ a lag shared by ~2 000 partitions
constexpr int kRepairThreads = 1024, kRepairEC = 8;        // tie_repair_kernel
constexpr int kRepairCap = kRepairThreads * kRepairEC;     // 8 192 positions a workgroup sorts at once
constexpr int kRepairWindow = kRepairCap / 2;              // so a run of up to 4 096 starting anywhere in a window fits

// bijection [0, n) -> [0, n): workgroups with equal (w % 8) get consecutive results
__device__ __forceinline__ int xcd_contiguous(int w, int n) {
    const int per = n / 8, rem = n % 8;                  // XCD x owns per (+1 if x < rem) values
    const int x = w % 8, k = w / 8;
    return x * per + (x < rem ? x : rem) + k;
}

__device__ __forceinline__ uint32_t digit_of(int pass, uint64_t key, uint32_t val) {
    return pass < 4 ? (val >> (8 * pass)) & 0xFFu : (uint32_t)(key >> (8 * (pass - 4))) & 0xFFu;
}

// ---- kernel 1: keys + all digit histograms ---------------------------------------------------
__global__ __launch_bounds__(256) void build_keys_kernel(LargeArgs a0, SortBufs b0, const LargeItem* items, char* scratch) {
    LA_PICK_ITEM(a, b, a0, b0, items, scratch, blockIdx.y)
    if ((int64_t)blockIdx.x * blockDim.x >= b.n) return;              // (a grid sized for the largest topic of the launch)
    __shared__ uint32_t h[kDigits * kRadix];
    for (int i = threadIdx.x; i < kDigits * kRadix; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const bool latest = a.reset_latest != 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t last_sample = 0;                                          // (lane 0 of a sampling wavefront)
    bool have_sample = false, sampling = true;
    bool out_of_bounds = false;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < b.n; base += stride) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < b.n;
        uint64_t key = 0;
        uint32_t val = 0;
        if (valid) {
            const int64_t g = a.p0 + i;
            int64_t lag;
            if (a.lag) lag = stream_load(a.lag + g);
            else lag = partition_lag(a.begin ? stream_load(a.begin + g) : 0, stream_load(a.end + g), stream_load(a.committed + g), latest);
            key = (uint64_t)lag ^ kLagKeyFlip;
            const int32_t id = a.pid[g];
            val = (uint32_t)id ^ kPidBias;
            b.key[0][i] = key;
            b.val[0][i] = val;
            // the caller's bounds decided which passes were launched at all (bounds_pass_mask): a partition outside them is an
            // error of the call (LA_EINVAL), never a differently sorted topic
            if (a.max_lag_hint >= 0 && ((uint64_t)lag > (uint64_t)a.max_lag_hint || (uint64_t)(int64_t)id > (uint64_t)a.max_id_hint))
                out_of_bounds = true;
            if (i + 1 < b.n && a.pid[g + 1] < id) b.ctl->unsorted_ids = 1;
        }
        const uint64_t vmask = __ballot(valid);
        if (b.samp) {
            // How frequent is the most frequent lag?  (keys-first sorts repair runs of equal keys inside one workgroup: a run
            // must fit.)  64 equal neighbours say "very"; otherwise every fourth wavefront counts its first key in a hash
            // table of n / 32 counters (n / 256 samples) with a FIRE-AND-FORGET atomic -- waiting for the counter's old value
            // put a ~2 us round trip into every fourth iteration, 70 us of a 300 us kernel -- and sample_scan_kernel looks for a
            // counter at kSampleHeavy afterwards (~ a lag that some thousand partitions share).  A wavefront that draws the same
            // key twice in a row says "frequent" at once and stops sampling: a hot counter sees a few atomics per wavefront, not
            // one per sample (reading the shared flag instead cost an L2 round trip per sample: 60 us of this kernel).
            const uint64_t k0 = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(key >> 32)) << 32) |
                                __builtin_amdgcn_readfirstlane((uint32_t)key);
            if (vmask == ~0ull && __ballot(key == k0) == ~0ull) {
                if (__lane_id() == 0) b.ctl->tie_heavy = 1;
            } else if (((base + (threadIdx.x & ~63)) >> 6) % 4 == 0 && (vmask & 1ull) && __lane_id() == 0 && sampling) {
                if (have_sample && k0 == last_sample) {
                    b.ctl->tie_heavy = 1;
                    sampling = false;                                  // (this wavefront has said what it had to say)
                } else {
                    const uint32_t h = (uint32_t)((k0 * 0x9E3779B97F4A7C15ull) >> (64 - b.samp_bits));
                    (void)__hip_atomic_fetch_add(&b.samp[h], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                last_sample = k0;
                have_sample = true;
            }
        }
#pragma unroll
        for (int p = 0; p < kDigits; ++p) {
            const uint32_t d = digit_of(p, key, val);
            // common case for the high digits: the whole wave agrees -> one add
            const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
            const uint64_t same = __ballot(valid && d == d0);
            if (same == vmask) {
                if (valid && (int)__lane_id() == __ffsll((unsigned long long)vmask) - 1)
                    atomicAdd(&h[p * kRadix + d0], (uint32_t)__popcll(vmask));
            } else if (valid) {
                atomicAdd(&h[p * kRadix + d], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kDigits * kRadix; i += blockDim.x)
        if (h[i]) atomicAdd(&b.hist[i], h[i]);
    if (__any(out_of_bounds) && (threadIdx.x & (kWave - 1)) == 0) atomicOr(a.status, kStatusBounds);
}

// ---- the sample of the lags: did any counter reach kSampleHeavy? ----------------------------------------------------------
__global__ __launch_bounds__(256) void sample_scan_kernel(SortBufs b0, const LargeItem* items, char* scratch) {
    LargeArgs unused{};
    SortBufs b = b0;
    if (items) bind_item(unused, b, items[blockIdx.y], scratch);
    if (!b.samp) return;
    const uint4* t = reinterpret_cast<const uint4*>(b.samp);
    const int64_t words = ((int64_t)1 << b.samp_bits) / 4, stride = (int64_t)gridDim.x * blockDim.x;
    bool heavy = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
        const uint4 v = t[i];
        heavy |= v.x >= kSampleHeavy || v.y >= kSampleHeavy || v.z >= kSampleHeavy || v.w >= kSampleHeavy;
    }
    if (__any(heavy) && (threadIdx.x & (kWave - 1)) == 0) b.ctl->tie_heavy = 1;
}

// ---- plan: which passes are no-ops, where the data lives before each pass --------------------
__global__ __launch_bounds__(kRadix) void plan_kernel(SortBufs b0, const LargeItem* items, char* scratch) {
    LargeArgs unused{};
    SortBufs b = b0;
    if (items) bind_item(unused, b, items[blockIdx.y], scratch);
    // block p: global first position of every digit of pass p (exclusive scan of its histogram): the single-kernel passes
    // add a tile's look-back result to it
    __shared__ uint32_t wsum[kRadix / kWave];
    {
        const int p = blockIdx.x, d = threadIdx.x, lane = d & 63, wave = d >> 6;
        const uint32_t h = b.hist[p * kRadix + d];
        uint32_t incl = h;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t run = incl - h;
        for (int w = 0; w < wave; ++w) run += wsum[w];
        b.gbase[p * kRadix + d] = run;
    }
    if (blockIdx.x != 0) return;
    // block 0: which passes are no-ops, where the data lives before each pass
    __shared__ uint32_t skip[kDigits];
    if (threadIdx.x < kDigits) skip[threadIdx.x] = 0;
    __syncthreads();
    for (int p = 0; p < kDigits; ++p)
        if (b.hist[p * kRadix + threadIdx.x] == (uint32_t)b.n) skip[p] = 1;   // one bin holds everything
    __syncthreads();
    if (threadIdx.x == 0) {
        // Keys first: the id passes only order partitions with EQUAL lags.  When the ids arrive shuffled and no lag is
        // frequent, sort by the key digits alone (stable: equal keys stay in input order) and let tie_repair_kernel put every
        // run of equal keys in id order afterwards -- for lags without long runs that is 5 scatter passes + one read where
        // the full LSD sort takes 9.  Frequent lags (the sample) keep the full order of passes: nothing changes for them.
        bool key_digits = false;
        for (int p = 4; p < kDigits; ++p) key_digits |= skip[p] == 0;
        const bool keys_first = b.samp != nullptr && b.ctl->unsorted_ids != 0 && key_digits &&
                                (b.keys_first_force || b.ctl->tie_heavy == 0);
        b.ctl->keys_first = keys_first ? 1u : 0u;
        uint32_t cur = 0;
        for (int p = 0; p < kDigits; ++p) {
            uint32_t s = skip[p];
            if (p < 4 && (b.ctl->unsorted_ids == 0 || keys_first)) s = 1;     // stable passes keep the input's id order
            b.ctl->skip[p] = s;
            b.ctl->cur[p] = cur;
            cur ^= (s ? 0u : 1u);
        }
        for (int p = kDigits; p < kSlots; ++p) {              // the redo slots: idle unless replan_kernel arms them
            b.ctl->skip[p] = 1;
            b.ctl->cur[p] = cur;
        }
        b.ctl->cur[kFinal] = cur;
    }
}

// After tie_repair_kernel: a run of equal keys that did not fit its workgroup (ctl->redo) sends the sort through the redo
// slots -- the full order of passes, ids first, from wherever the data stands; any permutation is a valid LSD input.
__global__ void replan_kernel(SortBufs b0, const LargeItem* items, char* scratch) {
    LargeArgs unused{};
    SortBufs b = b0;
    if (items) bind_item(unused, b, items[blockIdx.x], scratch);
    if (threadIdx.x != 0 || !b.ctl->keys_first || !b.ctl->redo) return;
    uint32_t cur = b.ctl->cur[kDigits];
    for (int p = 0; p < kDigits; ++p) {
        bool constant = false;
        for (int d = 0; d < kRadix; ++d) constant |= b.hist[p * kRadix + d] == (uint32_t)b.n;
        const uint32_t s = constant ? 1u : 0u;                 // (the ids are not ascending: keys first was chosen)
        b.ctl->skip[kDigits + p] = s;
        b.ctl->cur[kDigits + p] = cur;
        cur ^= (s ? 0u : 1u);
    }
    b.ctl->cur[kFinal] = cur;
}

// ---- per pass: tile digit counts ------------------------------------------------------------------
// A resident-sized grid walks the tiles; the next tile's loads (16 B per lane, whole tile) are issued before
// the current tile's histogram updates, one private histogram per wavefront (LDS atomics contend only inside
// a wavefront).  Only the array that carries the pass's digit is read: 8 B (key passes) or 4 B (id passes)
// per element.
template <bool IDS>
__device__ __forceinline__ void count_tiles(const SortBufs& b, int pass, uint32_t (*h)[kRadix]) {
    using Vec = typename std::conditional<IDS, uint4, ulonglong2>::type;
    constexpr int PER = IDS ? 4 : 2;                              // elements per 16-byte load
    constexpr int N = kTile / (PER * kSortThreads);
    const int wave = threadIdx.x >> 6;
    const uint32_t cur = b.ctl->cur[pass];
    const char* src = IDS ? (const char*)b.val[cur] : (const char*)b.key[cur];
    const int esz = IDS ? 4 : 8;
    const int sh = IDS ? 8 * pass : 8 * (pass - 4);
    auto digit = [&](const Vec& v, int k) -> uint32_t {
        if constexpr (IDS) return ((k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w) >> sh) & 0xFFu;
        else return (uint32_t)((k == 0 ? v.x : v.y) >> sh) & 0xFFu;
    };
    Vec v[N];
    auto load_tile = [&](int tile) {
        const int64_t t0 = (int64_t)tile * kTile;
        if (t0 + kTile <= b.n) {
#pragma unroll
            for (int k = 0; k < N; ++k)
                v[k] = *reinterpret_cast<const Vec*>(src + (t0 + PER * (k * kSortThreads + (int)threadIdx.x)) * esz);
        }
    };
    int tile = blockIdx.x;
    if (tile < b.n_tiles) load_tile(tile);
    for (; tile < b.n_tiles; tile += gridDim.x) {
        for (int i = threadIdx.x; i < kSortWaves * kRadix; i += kSortThreads) (&h[0][0])[i] = 0;
        __syncthreads();
        const int64_t t0 = (int64_t)tile * kTile;
        if (t0 + kTile <= b.n) {
            Vec w[N];
#pragma unroll
            for (int k = 0; k < N; ++k) w[k] = v[k];
            if (tile + (int)gridDim.x < b.n_tiles) load_tile(tile + gridDim.x);
#pragma unroll
            for (int k = 0; k < N; ++k)
#pragma unroll
                for (int e = 0; e < PER; ++e) atomicAdd(&h[wave][digit(w[k], e)], 1u);
        } else {
            for (int64_t i = t0 + threadIdx.x; i < b.n; i += kSortThreads) {
                const uint32_t d = IDS ? digit_of(pass, 0, b.val[cur][i]) : digit_of(pass, b.key[cur][i], 0);
                atomicAdd(&h[wave][d], 1u);
            }
        }
        __syncthreads();
        uint32_t c = 0;
#pragma unroll
        for (int w2 = 0; w2 < kSortWaves; ++w2) c += h[w2][threadIdx.x];
        b.tile_off[(int64_t)tile * kRadix + threadIdx.x] = c;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kSortThreads) void tile_count_kernel(SortBufs b, int pass) {
    if (b.ctl->skip[pass]) return;
    __shared__ uint32_t h[kSortWaves][kRadix];
    if (pass < 4) count_tiles<true>(b, pass, h);
    else count_tiles<false>(b, pass, h);
}

// ---- per pass: exclusive scan over the tiles of every digit's count, plus the digit's global base --------
// tile_off is [tile][digit]: the count kernel writes and the scatter kernel reads one contiguous 1 KB row
// per tile.  The scan walks columns: thread d owns digit d, a workgroup owns kScanRows consecutive tiles
// (every row access is a coalesced 1 KB).  Kernel A: the group's column sums.  Kernel B: every group adds up
// the sums of the groups before it (L2-resident, <= 256 KB per group) and rewrites its rows as offsets.
__global__ __launch_bounds__(kRadix) void scan_group_sums_kernel(SortBufs b, int pass) {
    if (b.ctl->skip[pass]) return;
    const int r0 = blockIdx.x * kScanRows;
    const int r1 = r0 + kScanRows < b.n_tiles ? r0 + kScanRows : b.n_tiles;
    uint32_t sum = 0;
    for (int r = r0; r < r1; ++r) sum += b.tile_off[(int64_t)r * kRadix + threadIdx.x];
    b.group_sum[(int64_t)blockIdx.x * kRadix + threadIdx.x] = sum;
}

__global__ __launch_bounds__(kRadix) void scan_offsets_kernel(SortBufs b, int pass) {
    if (b.ctl->skip[pass]) return;
    __shared__ uint32_t wsum[kRadix / kWave];
    const int d = threadIdx.x, lane = d & 63, wave = d >> 6;
    // global base of digit d = number of elements with a smaller digit (exclusive scan of the histogram)
    const uint32_t hcount = b.hist[pass * kRadix + d];
    uint32_t incl = hcount;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t run = incl - hcount;
    for (int w = 0; w < wave; ++w) run += wsum[w];
    // + this digit's elements in the groups before this one (independent loads: keep many in flight)
#pragma unroll 16
    for (int g = 0; g < (int)blockIdx.x; ++g) run += b.group_sum[(int64_t)g * kRadix + d];
    const int r0 = blockIdx.x * kScanRows;
    const int r1 = r0 + kScanRows < b.n_tiles ? r0 + kScanRows : b.n_tiles;
    for (int r = r0; r < r1; ++r) {
        uint32_t* p = b.tile_off + (int64_t)r * kRadix + d;
        const uint32_t x = *p;
        *p = run;
        run += x;
    }
}

// ---- rank of an element among the equal digits of its wavefront's share of a tile --------------------------------
// Order inside a tile = (wave, item, lane).  Two forms, same result:
//   * ATOMIC: ONE returning LDS atomic per element, `ds_add_rtn_u32 cnt[wave][digit], 1`.  The lanes of one DS instruction
//     that hit the same address are served in ascending lane order on gfx950, so the returned pre-values ARE the stable
//     ranks.  That order is what the hardware does, not something the ISA manual promises: la::large_init_device() checks
//     it once per device with lds_atomic_order_test_kernel (thousands of address patterns, several wavefronts at once) and
//     the launchers fall back to the other form if it ever fails.
//   * match: the wavefront finds every lane's peers (equal digits) with 8 ballots, the group's first lane advances the
//     counter.  ~100 VALU instructions per element more than the atomic form: with it the scatter kernels spend 2 190
//     VALU instructions per wavefront and tile and sit at 66 % VALU utilisation (profiles/archive/r03_sort_pmc_*.json).
template <bool ATOMIC>
__device__ __forceinline__ void rank_in_wave(const uint64_t (&key)[kItems], const uint32_t (&val)[kItems],
                                             uint32_t (&loc)[kItems], uint32_t* cnt_wave, int pass, int64_t w0, int64_t n,
                                             int lane) {
    if constexpr (ATOMIC) {
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const bool valid = w0 + it * kWave + lane < n;
            const uint32_t d = digit_of(pass, key[it], val[it]);
            uint32_t r = 0;
            if (valid) r = atomicAdd(&cnt_wave[d], 1u);
            loc[it] = (d << 16) | r;
        }
    } else {
        const uint64_t lt = ((uint64_t)1 << lane) - 1;
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const bool valid = w0 + it * kWave + lane < n;
            const uint32_t d = digit_of(pass, key[it], val[it]);
            uint64_t peers = __ballot(valid);
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool one = (d >> bit) & 1;
                const uint64_t bal = __ballot(one);
                peers &= one ? bal : ~bal;
            }
            uint32_t old = 0;
            if (valid) old = cnt_wave[d];                        // same address for all peers: broadcast
            wave_lds_fence();
            if (valid && (peers & lt) == 0) cnt_wave[d] = old + (uint32_t)__popcll(peers);   // group leader
            wave_lds_fence();
            loc[it] = (d << 16) | (old + (uint32_t)__popcll(peers & lt));
        }
    }
}

// One-off hardware check behind the ATOMIC form above: do the lanes of a returning LDS atomic that collide on an address
// get their pre-values in lane order?  4 wavefronts at once, each on its own counters, address sets of 1 .. 256 words,
// some lanes switched off, several atomics back to back as in the real loop.  *bad != 0: they do not.
__global__ __launch_bounds__(256) void lds_atomic_order_test_kernel(uint32_t* bad) {
    __shared__ uint32_t c[4][kRadix];              // counters the atomics advance
    __shared__ uint32_t shadow[4][kRadix];         // the same counters advanced by the match form: what a stable rank is
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lt = ((uint64_t)1 << lane) - 1;
    uint32_t wrong = 0;
    for (uint32_t pattern = 0; pattern < 384; ++pattern) {
        for (int i = lane; i < kRadix; i += kWave) { c[wave][i] = 0; shadow[wave][i] = 0; }
        wave_lds_fence();
        const uint32_t span = 1u << ((pattern + wave) % 9);                       // 1, 2, 4 .. 256 distinct addresses
        uint32_t got[4], want[4], addr[4];
        bool on[4];
#pragma unroll
        for (int rep = 0; rep < 4; ++rep) {
            uint32_t h = (uint32_t)lane * 2654435761u + pattern * 40503u + (uint32_t)rep * 97u + (uint32_t)wave * 7919u;
            h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
            addr[rep] = h & (span - 1);
            on[rep] = ((h >> 20) & 7u) != 0;
        }
#pragma unroll
        for (int rep = 0; rep < 4; ++rep) {
            uint64_t peers = __ballot(on[rep]);
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool one = (addr[rep] >> bit) & 1;
                const uint64_t bal = __ballot(one);
                peers &= one ? bal : ~bal;
            }
            uint32_t old = 0;
            if (on[rep]) old = shadow[wave][addr[rep]];
            wave_lds_fence();
            if (on[rep] && (peers & lt) == 0) shadow[wave][addr[rep]] = old + (uint32_t)__popcll(peers);
            wave_lds_fence();
            want[rep] = old + (uint32_t)__popcll(peers & lt);
        }
#pragma unroll
        for (int rep = 0; rep < 4; ++rep) {                  // back to back, as in rank_in_wave
            got[rep] = 0;
            if (on[rep]) got[rep] = atomicAdd(&c[wave][addr[rep]], 1u);
        }
#pragma unroll
        for (int rep = 0; rep < 4; ++rep) wrong |= (on[rep] && got[rep] != want[rep]) ? 1u : 0u;
        wave_lds_fence();
    }
    if (wrong) atomicOr(bad, 1u);
}

// ---- per pass: stable scatter ----------------------------------------------------------------------
// Order inside a tile = (wave, item, lane); elements are loaded wave-striped so every load is a
// 64-element contiguous run.  Rank among equal digits: wave-level match (8 ballots), running
// per-wave digit counters in LDS, then an exclusive scan of those counters over the waves (stable; no
// atomics on the data path).  The tile is then REORDERED IN LDS by digit, so that consecutive lanes write
// consecutive addresses of a digit's output run (a tile holds ~16 elements per digit: 128 B runs of keys,
// 64 B of ids) instead of 64 unrelated 8-byte writes per wavefront.
template <bool ATOMIC_RANK>
__global__ __launch_bounds__(kSortThreads) void tile_scatter_kernel(SortBufs b, int pass) {
    if (b.ctl->skip[pass]) return;
    static_assert(kSortThreads == kRadix, "one thread per digit in the offset phase");
    __shared__ uint32_t cnt[kSortWaves][kRadix];
    __shared__ uint32_t bin_start[kRadix];            // tile-local position of the digit's first element
    __shared__ uint32_t bin_base[kRadix];             // global position of it, minus bin_start
    __shared__ uint32_t wsum[kSortWaves];
    __shared__ uint64_t s_stage[kTile];               // the tile reordered by digit: one array at a time
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < kSortWaves * kRadix; i += kSortThreads) (&cnt[0][0])[i] = 0;
    __syncthreads();
    const uint32_t cur = b.ctl->cur[pass];
    const uint64_t* kin = b.key[cur];
    const uint32_t* vin = b.val[cur];
    uint64_t* kout = b.key[cur ^ 1];
    uint32_t* vout = b.val[cur ^ 1];
    // Workgroup w runs on XCD w % 8 (observed dispatch order; only speed depends on it).  Neighbouring tiles
    // write neighbouring runs of every digit's output: give each XCD a CONTIGUOUS range of tiles so that the
    // partial cache lines at the run boundaries meet in one L2 instead of being written back twice.
    const int tile = xcd_contiguous(blockIdx.x, gridDim.x);
    const int64_t t0 = (int64_t)tile * kTile;
    const int64_t w0 = t0 + (int64_t)wave * kItems * kWave;
    const int n_here = (int)((b.n - t0) < kTile ? (b.n - t0) : kTile);

    uint64_t key[kItems];
    uint32_t val[kItems];
    uint32_t loc[kItems];       // digit << 16 | rank inside (wave, digit)   (rank < 1024)
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const int64_t i = w0 + it * kWave + lane;
        const bool valid = i < b.n;
        key[it] = valid ? stream_load(kin + i) : 0;
        val[it] = valid ? stream_load(vin + i) : 0;
    }
    rank_in_wave<ATOMIC_RANK>(key, val, loc, cnt[wave], pass, w0, b.n, lane);
    __syncthreads();
    {   // thread d: exclusive scan of digit d's counters over the waves, then of the tile's digit counts
        const int d = threadIdx.x;
        uint32_t run = 0;
#pragma unroll
        for (int w = 0; w < kSortWaves; ++w) {
            const uint32_t c = cnt[w][d];
            cnt[w][d] = run;
            run += c;
        }
        uint32_t incl = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t woff = 0;
        for (int w = 0; w < wave; ++w) woff += wsum[w];
        const uint32_t start = woff + incl - run;
        bin_start[d] = start;
        bin_base[d] = b.tile_off[(int64_t)tile * kRadix + d] - start;
    }
    __syncthreads();
    // tile-local sorted position of every element
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const uint32_t d = loc[it] >> 16;
        loc[it] = bin_start[d] + cnt[wave][d] + (loc[it] & 0xFFFFu);
    }
    // The array that carries the pass's digit goes through the staging buffer first: the global position of
    // tile-local position j is bin_base[digit of the element at j] + j.
    uint32_t* s_val = reinterpret_cast<uint32_t*>(s_stage);
    uint32_t gpos[kItems];
    if (pass < 4) {
#pragma unroll
        for (int it = 0; it < kItems; ++it)
            if (w0 + it * kWave + lane < b.n) s_val[loc[it]] = val[it];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int j = it * kSortThreads + threadIdx.x;
            if (j < n_here) {
                const uint32_t v = s_val[j];
                gpos[it] = bin_base[digit_of(pass, 0, v)] + (uint32_t)j;
                vout[gpos[it]] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kItems; ++it)
            if (w0 + it * kWave + lane < b.n) s_stage[loc[it]] = key[it];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int j = it * kSortThreads + threadIdx.x;
            if (j < n_here) kout[gpos[it]] = s_stage[j];
        }
    } else {
#pragma unroll
        for (int it = 0; it < kItems; ++it)
            if (w0 + it * kWave + lane < b.n) s_stage[loc[it]] = key[it];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int j = it * kSortThreads + threadIdx.x;
            if (j < n_here) {
                const uint64_t k = s_stage[j];
                gpos[it] = bin_base[digit_of(pass, k, 0)] + (uint32_t)j;
                kout[gpos[it]] = k;
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kItems; ++it)
            if (w0 + it * kWave + lane < b.n) s_val[loc[it]] = val[it];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int j = it * kSortThreads + threadIdx.x;
            if (j < n_here) vout[gpos[it]] = s_val[j];
        }
    }
}

// ---- per pass, single-kernel form: stable scatter with decoupled look-back ----------------------------------------
// One launch per pass instead of four (count, two scans, scatter): the count kernel's re-read of the digit array
// (4-8 B per element) and the offset matrix are gone.  The global digit histograms come from build_keys_kernel
// (b.gbase = their exclusive scans, plan_kernel); what a tile still needs is how many elements of each digit the tiles
// BEFORE it hold.  Every tile publishes its 256 digit counts as granules {tag, count} -- ONE naturally aligned 8-byte
// relaxed agent-scope store each, the data is its own flag (cdna_hip_programming.md section 6, Guideline 16, form R2:
// the per-XCD L2s are not coherent, a plain store/load pair would go stale) -- first as an AGGREGATE (its own count),
// then, after walking back over its predecessors until it meets an INCLUSIVE one, as the inclusive prefix.  tag =
// (pass + 1) << 2 | status, so the state array is zeroed once per sort, not per pass.
//
// Which tile a workgroup takes is decided by an arrival ticket, never by blockIdx: tile = arrival number, so a tile only
// ever waits for tiles whose workgroups are already running, and the walk cannot deadlock whatever the dispatch order is
// (a bounded spin turns anything unforeseen into kStatusInternal instead of a hung device).  Tried and measured without
// effect on this kernel (profiles/archive/r03_sort_*): giving every XCD 4-32 consecutive tiles at a time (arrival- or
// blockIdx-based) -- what made the four-kernel scatter 20 % faster -- and polling 4, 8 or 16 predecessors per hop.
#ifdef LA_LOOKBACK_STATS   // development build: how far the walks go (tools/lookback_probe.py)
__device__ unsigned long long g_lookback_stats[8];      // walks, hops, polls that found nothing, longest walk, cycles in walks
#endif
#ifdef LA_SWEEP_CLOCKS     // development build: thread 0 of every tile adds the time of each phase (tools/lookback_probe.py)
__device__ unsigned long long g_sweep_clocks[12];
#define LA_SCLK(i)                                                                      \
    do {                                                                                \
        if (threadIdx.x == 0) {                                                         \
            const unsigned long long now_ = wall_clock64();                             \
            atomicAdd(&g_sweep_clocks[i], now_ - sclk_);                                \
            sclk_ = now_;                                                               \
        }                                                                               \
    } while (0)
#define LA_SCLK_START unsigned long long sclk_ = wall_clock64(); if (threadIdx.x == 0) atomicAdd(&g_sweep_clocks[11], 1ull)
#else
#define LA_SCLK(i) do {} while (0)
#define LA_SCLK_START do {} while (0)
#endif
constexpr uint32_t kStateAggregate = 1u, kStateInclusive = 2u;
constexpr int kLookWindow = 2;           // predecessors a walk polls at once
constexpr uint32_t kLookbackSpinLimit = 1u << 22;     // polls of one granule (~1 us each with the sleep) before giving up

// One tile of one pass: the body of onesweep_pass_kernel (one tile per workgroup, taken by arrival) and of onesweep_redo_kernel
// (workgroups that loop over tickets and passes).  s_ticket: the tile's number, written by thread 0 of the caller BEFORE
// the call and read here after the first barrier.
template <bool ATOMIC_RANK, int THREADS>
__device__ __forceinline__ void onesweep_tile(const SortBufs& b, const int slot, uint32_t* status, const uint32_t* s_ticket) {
    const int pass = slot >= kDigits ? slot - kDigits : slot;   // the digit the slot sorts by (the redo slots repeat the digits)
    static_assert(THREADS >= kRadix && THREADS % kWave == 0, "one thread per digit in the look-back");
    constexpr int WAVES = THREADS / kWave, TILE = THREADS * kItems;
    __shared__ uint32_t cnt[WAVES][kRadix];
    __shared__ uint32_t bin_start[kRadix];            // tile-local position of the digit's first element
    __shared__ uint32_t bin_base[kRadix];             // global position of it, minus bin_start
    __shared__ uint32_t wsum[kRadix / kWave];
    __shared__ uint64_t s_stage[TILE];                // the tile reordered by digit: one array at a time
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool digit_thread = threadIdx.x < kRadix;   // (whole wavefronts: 0 .. 3)
    LA_SCLK_START;
    for (int i = threadIdx.x; i < WAVES * kRadix; i += THREADS) (&cnt[0][0])[i] = 0;
    __syncthreads();
    const uint32_t cur = b.ctl->cur[slot];
    const uint64_t* kin = key_buf(b, cur);
    const uint32_t* vin = val_buf(b, cur);
    uint64_t* kout = key_buf(b, cur ^ 1u);
    uint32_t* vout = val_buf(b, cur ^ 1u);
    const int tile = (int)*s_ticket;
    const int64_t t0 = (int64_t)tile * TILE;
    const int64_t w0 = t0 + (int64_t)wave * kItems * kWave;
    const int n_here = (int)((b.n - t0) < TILE ? (b.n - t0) : TILE);
    const uint32_t epoch = (uint32_t)(slot + 1) << 2;
    unsigned long long* my_state = b.tile_state + (int64_t)tile * kRadix + (threadIdx.x & (kRadix - 1));

    uint64_t key[kItems];
    uint32_t val[kItems];
    uint32_t loc[kItems];       // digit << 16 | rank inside (wave, digit)   (rank < 1024)
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const int64_t i = w0 + it * kWave + lane;
        const bool valid = i < b.n;
        key[it] = valid ? stream_load(kin + i) : 0;
        val[it] = valid ? stream_load(vin + i) : 0;
    }
    LA_SCLK(0);                                       // ticket, counters, loads issued
    rank_in_wave<ATOMIC_RANK>(key, val, loc, cnt[wave], pass, w0, b.n, lane);
    LA_SCLK(1);                                       // loads landed + ranks (this wavefront)
    __syncthreads();
    LA_SCLK(2);                                       // ... of the slowest wavefront
    // thread d: digit d's count in this tile; published at once, so that later tiles never wait for this tile's walk
    uint32_t count = 0, incl = 0;
    unsigned long long win[kLookWindow];
    if (digit_thread) {
        const int d = threadIdx.x;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t c = cnt[w][d];
            cnt[w][d] = count;
            count += c;
        }
        __hip_atomic_store(my_state, ((unsigned long long)(epoch | (tile == 0 ? kStateInclusive : kStateAggregate)) << 32) | count,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the first window of the walk is in flight while the tile is staged below
#pragma unroll
        for (int i = 0; i < kLookWindow; ++i)
            win[i] = i < tile ? __hip_atomic_load(my_state - (i + 1) * kRadix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        incl = count;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
    }
    __syncthreads();
    if (digit_thread) {
        uint32_t woff = 0;
        for (int w = 0; w < wave; ++w) woff += wsum[w];
        bin_start[threadIdx.x] = woff + incl - count;
    }
    __syncthreads();
    // tile-local sorted position of every element; the array that carries the pass's digit goes to the staging buffer
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const uint32_t d = loc[it] >> 16;
        loc[it] = bin_start[d] + cnt[wave][d] + (loc[it] & 0xFFFFu);
    }
    uint32_t* s_val = reinterpret_cast<uint32_t*>(s_stage);
    if (pass < 4) {
#pragma unroll
        for (int it = 0; it < kItems; ++it)
            if (w0 + it * kWave + lane < b.n) s_val[loc[it]] = val[it];
    } else {
#pragma unroll
        for (int it = 0; it < kItems; ++it)
            if (w0 + it * kWave + lane < b.n) s_stage[loc[it]] = key[it];
    }
    LA_SCLK(3);                                       // counts published, bin starts, first array staged
    if (digit_thread)
    {   // The walk: thread d adds up digit d's counts of the tiles before this one, nearest first, until it meets an
        // inclusive prefix.  A hop costs a trip to the fabric (the granules are write-through, the per-XCD L2s are not
        // coherent) behind this CU's own streaming loads and stores -- about 1 us -- and a walk passes ~28 tiles that have
        // published only their aggregate (measured: tools/lookback_probe.py), so kLookWindow predecessors are polled at once.
        const int d = threadIdx.x;
        uint32_t excl = 0;
        if (tile > 0) {
            int next = tile - 1;                                 // the nearest tile not yet added
            uint32_t spins = 0;
#ifdef LA_LOOKBACK_STATS
            unsigned long long hops = 0, empty = 0;
            const unsigned long long clk0 = clock64();
#endif
            for (;;) {
                bool done = false;
                int used = 0;
#pragma unroll
                for (int i = 0; i < kLookWindow; ++i) {
                    const uint32_t tag = (uint32_t)(win[i] >> 32);
                    const bool ready = (tag & ~3u) == epoch && i < next + 1 && used == i && !done;
                    if (ready) {
                        excl += (uint32_t)win[i];
                        used = i + 1;
                        done = (tag & 3u) == kStateInclusive;
                    }
                }
#ifdef LA_LOOKBACK_STATS
                hops += (unsigned long long)used;
                empty += used == 0 ? 1 : 0;
#endif
                if (done) break;
                next -= used;                                    // tile 0 is always inclusive: next never drops below 0 here
                if (used == 0) {
                    if (++spins > kLookbackSpinLimit) { atomicOr(status, kStatusInternal); break; }
                    __builtin_amdgcn_s_sleep(2);
                } else {
                    spins = 0;
                }
                const unsigned long long* look = b.tile_state + (int64_t)next * kRadix + d;
#pragma unroll
                for (int i = 0; i < kLookWindow; ++i)
                    win[i] = i <= next ? __hip_atomic_load(look - i * kRadix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            }
#ifdef LA_LOOKBACK_STATS
            if (d == 0) {
                atomicAdd(&g_lookback_stats[0], 1ull);
                atomicAdd(&g_lookback_stats[1], hops);
                atomicAdd(&g_lookback_stats[2], empty);
                atomicMax(&g_lookback_stats[3], hops);
                atomicAdd(&g_lookback_stats[4], (unsigned long long)(clock64() - clk0));
            }
#endif
            __hip_atomic_store(my_state, ((unsigned long long)(epoch | kStateInclusive) << 32) | (excl + count),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        bin_base[d] = b.gbase[pass * kRadix + d] + excl - bin_start[d];
    }
    LA_SCLK(4);                                       // this wavefront's walk
    __syncthreads();
    LA_SCLK(5);                                       // ... the slowest walk
    // the global position of tile-local position j is bin_base[digit of the element at j] + j
    uint32_t gpos[kItems];
    if (pass < 4) {
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int j = it * THREADS + threadIdx.x;
            if (j < n_here) {
                const uint32_t v = s_val[j];
                gpos[it] = bin_base[digit_of(pass, 0, v)] + (uint32_t)j;
                vout[gpos[it]] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kItems; ++it)
            if (w0 + it * kWave + lane < b.n) s_stage[loc[it]] = key[it];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int j = it * THREADS + threadIdx.x;
            if (j < n_here) kout[gpos[it]] = s_stage[j];
        }
    } else {
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int j = it * THREADS + threadIdx.x;
            if (j < n_here) {
                const uint64_t k = s_stage[j];
                gpos[it] = bin_base[digit_of(pass, k, 0)] + (uint32_t)j;
                kout[gpos[it]] = k;
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kItems; ++it)
            if (w0 + it * kWave + lane < b.n) s_val[loc[it]] = val[it];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int j = it * THREADS + threadIdx.x;
            if (j < n_here) vout[gpos[it]] = s_val[j];
        }
    }
    LA_SCLK(6);                                       // both scatters issued (stores still in flight)
}

template <bool ATOMIC_RANK, int THREADS>
__global__ __launch_bounds__(THREADS, 4) void onesweep_pass_kernel(SortBufs b0, int pass, uint32_t* status, const LargeItem* items,
                                                                   char* scratch) {
    LargeArgs unused{};
    SortBufs b = b0;
    if (items) bind_item(unused, b, items[blockIdx.y], scratch);
    // several topics per launch: the grid is as wide as the launch's largest topic, and only workgroups that have a tile to
    // sort may draw a ticket (tiles are taken by arrival, so exactly n_tiles workgroups of a topic must arrive)
    if ((int)blockIdx.x >= b.n_tiles) return;
    const int slot = pass;                            // control-block slot (skip / cur / ticket / tag of the granules)
    if (b.ctl->skip[slot]) return;
    __shared__ uint32_t s_ticket;
    if (threadIdx.x == 0) s_ticket = atomicAdd(&b.ticket[slot], 1u);
    onesweep_tile<ATOMIC_RANK, THREADS>(b, slot, status, &s_ticket);
}

// ---- the redo slots of a keys-first sort as ONE launch -------------------------------------------------------------------------
// A keys-first sort whose tie repair met a run of equal lags longer than a workgroup holds (ctl->redo: the sample said there
// was none, or a test forced keys first) is sorted again in full, ids first.  Rounds 4-5 kept a second set of pass launches
// for that -- up to twelve kernels that return at once in every ordinary sort, 4.4 us apiece: 50 us of a 1.15 ms sort of 33.5 M
// partitions, a fifth of the sort of a 5 M-partition topic.  Now: ONE kernel whose workgroups return at once unless ctl->redo
// is set, and otherwise run all the redo passes themselves -- tiles by ticket as in the pass kernel (a workgroup that holds
// ticket t walks back over tiles that running workgroups hold: the look-back cannot wait for a workgroup that has not
// started), an agent-scope barrier over the launch's workgroups between passes.  The grid is small enough to be resident at
// once (a workgroup keeps its CU until the last pass is done).
template <bool ATOMIC_RANK, int THREADS>
__global__ __launch_bounds__(THREADS, 4) void onesweep_redo_kernel(SortBufs b0, uint32_t pass_mask, uint32_t* status, const LargeItem* items,
                                                                   char* scratch) {
    LargeArgs unused{};
    SortBufs b = b0;
    if (items) bind_item(unused, b, items[blockIdx.y], scratch);
    if (!b.ctl->keys_first || !b.ctl->redo) return;   // (every workgroup of the topic reads the same words: replan_kernel ran before)
    __shared__ uint32_t s_ticket;
    uint32_t passes_done = 0;
    for (int d = 0; d < kDigits; ++d) {
        const int slot = kDigits + d;
        if (!((pass_mask >> d) & 1u) || b.ctl->skip[slot]) continue;          // (uniform over the topic's workgroups)
        for (;;) {
            if (threadIdx.x == 0) s_ticket = atomicAdd(&b.ticket[slot], 1u);
            __syncthreads();
            const bool more = (int)s_ticket < b.n_tiles;
            if (!more) break;                          // (uniform: one shared word; nobody writes it before the barrier below)
            onesweep_tile<ATOMIC_RANK, THREADS>(b, slot, status, &s_ticket);
            __syncthreads();                           // the tile's last reads of the staging buffer and of s_ticket
        }
        // every workgroup's stores of this pass, visible to every other before the next pass reads them
        ++passes_done;
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) {
            __hip_atomic_fetch_add(&b.ctl->redo_arrived, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t want = passes_done * gridDim.x;
            while (__hip_atomic_load(&b.ctl->redo_arrived, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < want) __builtin_amdgcn_s_sleep(2);
        }
        __syncthreads();
    }
}

// ---- keys-first sorts: every run of equal keys into id order ------------------------------------------------------------------
// After the key passes of a keys-first sort the partitions are in (lag desc) order and partitions with EQUAL lags stand in
// input order; the comparator wants them in id order (Main.java:228-235).  Windows of kRepairWindow positions, one workgroup
// per window (grid-stride): a window without two equal neighbours -- nearly all of them when lags are wide -- cost its 8 B
// per partition of reading in tie_scan_kernel and is skipped here.  Otherwise the workgroup takes the runs that START in its window, whole, up to kRepairCap
// positions: (index of the run) << 32 | id into registers, the block-wide bitonic network of the greedy's bins (la_sort64.h
// inside a wavefront, LDS exchanges across), ids back in place.  A window writes only the runs that start in it and reads no
// ids but theirs, so windows do not interfere.  A run that reaches beyond the capacity is left alone and raises ctl->redo:
// the sample said there was no such run (or the test hook forced keys first), and the redo slots then sort in full.

// First a plain streaming read of the sorted keys at full occupancy (the repair kernel below keeps 128 KB of LDS per workgroup
// -- one workgroup per CU -- and would read them at a sixth of the bandwidth).  The thread that meets the START of a run of
// equal keys settles it on the spot when the run has at most four members -- with wide lags nearly every tie is a pair: four
// ids into registers, a five-step network, back -- and otherwise marks the window the run starts in for tie_repair_kernel.
__device__ __forceinline__ void tie_run_start(const uint64_t* key, uint32_t* val, int64_t p, int64_t n, uint32_t* tie_flag) {
    const uint64_t k = key[p];
    int len = 2;                                                            // (key[p + 1] == k is why we are here)
    while (len < 5 && p + len < n && key[p + len] == k) ++len;
    if (len > 4) { tie_flag[p / kRepairWindow] = 1; return; }
    uint32_t v0 = val[p], v1 = val[p + 1], v2 = len > 2 ? val[p + 2] : 0xFFFFFFFFu, v3 = len > 3 ? val[p + 3] : 0xFFFFFFFFu;
    auto cx = [](uint32_t& a, uint32_t& b) { const uint32_t lo = a < b ? a : b, hi = a < b ? b : a; a = lo; b = hi; };
    cx(v0, v1); cx(v2, v3); cx(v0, v2); cx(v1, v3); cx(v1, v2);             // (pads are the largest value: they stay behind)
    val[p] = v0; val[p + 1] = v1;
    if (len > 2) val[p + 2] = v2;
    if (len > 3) val[p + 3] = v3;
}

__global__ __launch_bounds__(256) void tie_scan_kernel(SortBufs b0, const LargeItem* items, char* scratch) {
    LargeArgs unused{};
    SortBufs b = b0;
    if (items) bind_item(unused, b, items[blockIdx.y], scratch);
    if (!b.ctl->keys_first) return;
    const uint32_t fin = b.ctl->cur[kDigits];
    const uint64_t* key = key_buf(b, fin);
    uint32_t* val = val_buf(b, fin);
    const int64_t n = b.n, pairs = (n + 1) / 2;
    struct __attribute__((aligned(16))) U64x2 { uint64_t x, y; };
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < pairs; j += stride) {
        const int64_t i = 2 * j;                                            // positions i, i + 1 (one 16-byte load) and their neighbours
        uint64_t km = 0, k0, k1 = 0, k2 = 0;
        if (i + 1 < n) { const U64x2 v = *reinterpret_cast<const U64x2*>(key + i); k0 = v.x; k1 = v.y; }
        else k0 = key[i];
        if (i > 0) km = key[i - 1];
        if (i + 2 < n) k2 = key[i + 2];
        if (i + 1 < n && k0 == k1 && (i == 0 || km != k0)) tie_run_start(key, val, i, n, b.tie_flag);
        if (i + 2 < n && k1 == k2 && k0 != k1) tie_run_start(key, val, i + 1, n, b.tie_flag);
    }
}

__global__ __launch_bounds__(kRepairThreads) void tie_repair_kernel(SortBufs b0, const LargeItem* items, char* scratch) {
    extern __shared__ __attribute__((aligned(16))) uint64_t s_x[];        // two exchange buffers of kRepairCap words
    __shared__ int s_first, s_last, s_end;
    __shared__ uint32_t s_wsum[kRepairThreads / kWave];
    LargeArgs unused{};
    SortBufs b = b0;
    if (items) bind_item(unused, b, items[blockIdx.y], scratch);
    if (!b.ctl->keys_first) return;
    constexpr int EC = kRepairEC, NT = kRepairThreads, W = kRepairWindow, CAP = kRepairCap;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t fin = b.ctl->cur[kDigits];                               // (the data after the sort's own slots)
    const uint64_t* key = key_buf(b, fin);
    uint32_t* val = val_buf(b, fin);
    const int64_t n = b.n;
    for (int64_t w0 = (int64_t)blockIdx.x * W; w0 < n; w0 += (int64_t)gridDim.x * W) {
        const int64_t w1 = w0 + W < n ? w0 + W : n;
        if (b.tie_flag[w0 / W] == 0) continue;                              // (uniform) no run of more than four starts here
        // the first and the last run start inside the window; where the last run ends (searched up to the capacity)
        __syncthreads();                                                    // (the window before this one is done with s_*)
        if (tid == 0) { s_first = 0x7FFFFFFF; s_last = -1; s_end = 0x7FFFFFFF; }
        __syncthreads();
        {
            int lo = 0x7FFFFFFF, hi = -1;
            for (int64_t p = w0 + tid; p < w1; p += NT)
                if (p == 0 || key[p] != key[p - 1]) { const int o = (int)(p - w0); lo = o < lo ? o : lo; hi = o > hi ? o : hi; }
            if (lo != 0x7FFFFFFF) { atomicMin(&s_first, lo); atomicMax(&s_last, hi); }
        }
        __syncthreads();
        if (s_last < 0) continue;                                           // the whole window lies inside an earlier run (uniform)
        const int64_t first = w0 + s_first;
        {
            int e = 0x7FFFFFFF;
            for (int64_t p = w1 + tid; p <= first + CAP && p <= n; p += NT)
                if (p == n || key[p] != key[p - 1]) { const int o = (int)(p - first); e = o < e ? o : e; }
            if (e != 0x7FFFFFFF) atomicMin(&s_end, e);
        }
        __syncthreads();
        int len;
        if (s_end != 0x7FFFFFFF) {
            len = s_end;                                                    // every run that starts in the window, whole
        } else {
            len = (int)(w0 + s_last - first);                               // the last run does not fit: without it,
            if (tid == 0) b.ctl->redo = 1;                                  // and the sort is redone in full
        }
        __syncthreads();                                                    // (s_* are rewritten by the next window)
        if (len <= 1) continue;
        // composites: (index of the run in the region) << 32 | biased id; slots beyond the region sort last
        P64 rec[EC];
        uint32_t flags = 0, own = 0;
        uint64_t prev = first + (int64_t)tid * EC > 0 && tid * EC < len ? key[first + (int64_t)tid * EC - 1] : 0;
        uint32_t v[EC];
#pragma unroll
        for (int r = 0; r < EC; ++r) {
            const int i = tid * EC + r;
            const bool valid = i < len;
            const uint64_t k = valid ? key[first + i] : 0;
            v[r] = valid ? val[first + i] : 0;
            const bool start = valid && (i == 0 || k != prev);
            flags |= start ? 1u << r : 0u;
            own += start ? 1u : 0u;
            prev = k;
        }
        uint32_t incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        uint32_t run = incl - own;                                          // runs that start before this thread's positions
        for (int x = 0; x < wave; ++x) run += s_wsum[x];
#pragma unroll
        for (int r = 0; r < EC; ++r) {
            run += (flags >> r) & 1u;
            rec[r] = p64_from(tid * EC + r < len ? ((uint64_t)run << 32) | v[r] : ~0ull);
        }
        workgroup_sort_p64<EC>(rec, s_x, CAP, tid);                          // the network of greedy_rounds_packed's bins
        lds_barrier();
#pragma unroll
        for (int r = 0; r < EC; ++r) {
            const int i = tid * EC + r;
            if (i < len) val[first + i] = (uint32_t)p64_value(rec[r]);
        }
        __syncthreads();
    }
}

}  // namespace

// ---- host: the device check, layout and scratch, the launch sequences (declared in la_radix.h) -------------------------------
// Per device, once (la_create_multi; synchronous): are the pre-values of colliding lanes of a returning LDS atomic in lane
// order (rank_in_wave)?  The launchers rank with the match form where they are not (or the check could not run).
static std::atomic<int> g_atomic_rank_ok[32];       // 0 = not checked, 1 = no, 2 = yes

hipError_t large_init_device() {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 32 || g_atomic_rank_ok[dev].load(std::memory_order_acquire) != 0) return hipSuccess;
    int verdict = 1;
    const char* env = getenv("LA_SORT_RANK");                  // "match": never the atomic form (A/B, tests)
    if (!(env && env[0] == 'm')) {
        uint32_t* d_bad = nullptr;
        uint32_t h_bad = 1;
        if ((e = hipMalloc((void**)&d_bad, sizeof(uint32_t))) != hipSuccess) return e;
        if ((e = hipMemset(d_bad, 0, sizeof(uint32_t))) == hipSuccess) {
            LA_LAUNCH(lds_atomic_order_test_kernel, dim3(8), dim3(256), 0, nullptr, d_bad);
            e = hipMemcpy(&h_bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost);
        }
        (void)hipFree(d_bad);
        if (e != hipSuccess) return e;
        verdict = h_bad == 0 ? 2 : 1;
    }
    g_atomic_rank_ok[dev].store(verdict, std::memory_order_release);
    return hipSuccess;
}

int large_atomic_rank_supported() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return 0;
    return g_atomic_rank_ok[dev].load(std::memory_order_acquire) == 2 ? 1 : 0;
}

// Keys-first sorts (plan_kernel): worth their extra launches from a few million partitions on; LA_SORT_KEYS_FIRST=0 never,
// =2 always and whatever the sample says (test hook: small topics, long runs through the redo slots).
static int keys_first_mode(int64_t n, bool multi_kernel) {
    int mode = 1;
    if (const char* env = getenv("LA_SORT_KEYS_FIRST")) mode = atoi(env);
    if (multi_kernel || mode <= 0) return 0;
    if (mode >= 2) return 2;
    return n >= ((int64_t)1 << 22) ? 1 : 0;
}

SortLayout sort_layout(int64_t n, bool multi_kernel, bool may_sort_keys_first) {
    SortLayout L;
    L.n = n;
    if (n >= ((int64_t)1 << 30)) multi_kernel = true;
    if (const char* env = getenv("LA_SORT_MULTIKERNEL")) multi_kernel = multi_kernel || atoi(env) != 0;
    L.multi_kernel = multi_kernel;
    // Tiles of 16 elements per thread: the larger the workgroup, the fewer tiles publish and walk (the look-back costs a
    // tile ~10 us whatever its size) and the longer the runs a tile writes per digit -- 33.5 M partitions: 2.25 / 2.02 / 1.93 ms
    // with 256 / 512 / 1 024 threads on the same box, four-kernel passes 2.56; but a 1 M-partition topic (cfg5) has only 64
    // tiles of 16 384: 0.136 / 0.125 / 0.144 ms (profiles/archive/r03_sort_tile_sizes.txt)
    int sweep_threads = n >= (3 << 20) ? 1024 : (n >= (1 << 17) ? 512 : 256);
    if (const char* env = getenv("LA_SWEEP_THREADS")) { const int w = atoi(env); sweep_threads = w == 256 || w == 1024 ? w : 512; }
    L.sweep_threads = sweep_threads;
    const int64_t tile = multi_kernel ? kTile : (int64_t)sweep_threads * kItems;
    L.n_tiles = (int)((n + tile - 1) / tile);
    L.n_groups = (L.n_tiles + kScanRows - 1) / kScanRows;
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    L.o_ctl = carve(sizeof(SortCtl));
    L.o_hist = carve(sizeof(uint32_t) * kDigits * kRadix);
    L.o_ticket = carve(sizeof(uint32_t) * kSlots);
    L.o_state = carve(multi_kernel ? 0 : sizeof(unsigned long long) * kRadix * (size_t)L.n_tiles);
    L.keys_first = may_sort_keys_first ? keys_first_mode(n, multi_kernel) : 0;
    if (L.keys_first) {
        L.samp_bits = 10;                                           // n / 32 counters for n / 256 samples (at least 1 024)
        while (((int64_t)1 << L.samp_bits) < n / 32 && L.samp_bits < 28) ++L.samp_bits;
        L.o_samp = carve(sizeof(uint32_t) << L.samp_bits);
        L.o_flag = carve(sizeof(uint32_t) * (size_t)((n + kRepairWindow - 1) / kRepairWindow));
    }
    L.zero_bytes = off;
    off = 0;
    L.o_gbase = carve(sizeof(uint32_t) * kDigits * kRadix);
    L.o_k0 = carve(sizeof(uint64_t) * n); L.o_k1 = carve(sizeof(uint64_t) * n);
    L.o_v0 = carve(sizeof(uint32_t) * n); L.o_v1 = carve(sizeof(uint32_t) * n);
    L.o_to = carve(multi_kernel ? sizeof(uint32_t) * kRadix * (size_t)L.n_tiles : 0);
    L.o_gs = carve(multi_kernel ? sizeof(uint32_t) * kRadix * (size_t)L.n_groups : 0);
    L.data_bytes = off;
    return L;
}

SortBufs sort_bind(const SortLayout& L, char* zero, char* data) {
    SortBufs b{};
    b.ctl = (SortCtl*)(zero + L.o_ctl);
    b.hist = (uint32_t*)(zero + L.o_hist);
    b.ticket = (uint32_t*)(zero + L.o_ticket);
    b.tile_state = L.multi_kernel ? nullptr : (unsigned long long*)(zero + L.o_state);
    b.gbase = (uint32_t*)(data + L.o_gbase);
    b.key[0] = (uint64_t*)(data + L.o_k0);
    b.key[1] = (uint64_t*)(data + L.o_k1);
    b.val[0] = (uint32_t*)(data + L.o_v0);
    b.val[1] = (uint32_t*)(data + L.o_v1);
    b.tile_off = (uint32_t*)(data + L.o_to);
    b.group_sum = (uint32_t*)(data + L.o_gs);
    b.n = L.n;
    b.n_tiles = L.n_tiles;
    b.n_groups = L.n_groups;
    b.atomic_rank = large_atomic_rank_supported();
    b.sweep_threads = L.sweep_threads;
    b.samp = L.keys_first ? (uint32_t*)(zero + L.o_samp) : nullptr;
    b.tie_flag = (uint32_t*)(zero + L.o_flag);
    b.samp_bits = L.samp_bits;
    b.keys_first_force = L.keys_first == 2 ? 1 : 0;
    return b;
}

hipError_t scratch_reserve(LargeScratch& scratch, size_t bytes, hipStream_t stream) {
    if (bytes <= scratch.cap) return hipSuccess;
    hipError_t e;
    if (scratch.buf) {
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        if ((e = hipFree(scratch.buf)) != hipSuccess) return e;
        scratch.buf = nullptr;
        scratch.cap = 0;
    }
    const size_t want = bytes + bytes / 4;
    if ((e = hipMalloc(&scratch.buf, want)) != hipSuccess) return e;
    scratch.cap = want;
    return hipSuccess;
}

hipError_t sort_prepare(LargeScratch& scratch, int64_t n, hipStream_t stream, SortBufs* out, bool multi_kernel,
                        bool may_sort_keys_first) {
    const SortLayout L = sort_layout(n, multi_kernel, may_sort_keys_first);
    hipError_t e;
    if ((e = scratch_reserve(scratch, L.zero_bytes + L.data_bytes, stream)) != hipSuccess) return e;
    char* base = (char*)scratch.buf;
    *out = sort_bind(L, base, base + L.zero_bytes);
    return hipMemsetAsync(base, 0, L.zero_bytes, stream);
}

// The passes a caller's bounds (LA_FLAG_BOUNDS: 0 <= lag <= max_lag, 0 <= id <= max_id) leave possible: a key digit above the
// lag's bits holds the same value in every record (key = lag ^ 0x7FFF..., so the bits above are all ones), an id digit above the
// id's bits likewise (val = id ^ 0x80000000) -- the device-side plan would find them constant and skip them, but each skipped
// pass is still a launch (3-4.5 us apiece: cfg5 launches 6 such, a 33.5 M-partition keys-first sort 3 + 3 redo slots).
// build_keys_kernel raises kStatusBounds on a partition outside the bounds.
uint32_t bounds_pass_mask(const LargeArgs& a) {
    uint32_t mask = kAllPasses;
    if (a.max_lag_hint < 0 || a.max_id_hint < 0) return mask;
    const int lag_bits = a.max_lag_hint > 0 ? 64 - __builtin_clzll((unsigned long long)a.max_lag_hint) : 0;
    const int id_bits = a.max_id_hint > 0 ? 64 - __builtin_clzll((unsigned long long)a.max_id_hint) : 0;
    mask = 0;
    for (int d = 0; d < 4; ++d) if (8 * d < id_bits) mask |= 1u << d;
    for (int d = 0; d < 8; ++d) if (8 * d < lag_bits) mask |= 1u << (4 + d);
    return mask;
}

// (b.sweep_threads, b.atomic_rank) as compile-time values: f(std::bool_constant<atomic rank>, std::integral_constant<int, threads>)
template <typename F>
static void with_sweep_class(const SortBufs& b, F&& f) {
    auto with_rank = [&](auto threads) {
        if (b.atomic_rank) f(std::true_type{}, threads);
        else f(std::false_type{}, threads);
    };
    if (b.sweep_threads == 1024) with_rank(std::integral_constant<int, 1024>{});
    else if (b.sweep_threads == 512) with_rank(std::integral_constant<int, 512>{});
    else with_rank(std::integral_constant<int, 256>{});
}

SortJob sort_job_single(const SortBufs& b, uint32_t pass_mask, uint32_t* status) {
    return SortJob{b, nullptr, 1, nullptr, {{0, 1, b.sweep_threads, b.n_tiles}}, 1, b.samp != nullptr, b.n, pass_mask, status};
}

// The launched passes of every tile class.  slot0 = 0: the sort's own slots; kDigits: the redo slots of a keys-first sort (the
// same digits again, see tie_repair_kernel).  A pass is ONE launch (onesweep_pass_kernel) -- or four, when the sort was
// prepared for the multi-kernel form; the redo slots of a class are one launch altogether.
static void sort_passes(const SortJob& j, hipStream_t stream, int slot0) {
    for (int c = 0; c < j.n_cls; ++c) {
        const SortClass& k = j.cls[c];
        SortBufs b = j.b;
        const LargeItem* items = nullptr;
        if (j.items) {
            items = j.items + k.first;
            b.sweep_threads = k.sweep_threads;
            b.tile_state = (unsigned long long*)j.base;            // (non-null: the single-kernel passes; items carry the real one)
        }
        if (slot0 == kDigits && b.tile_state) {
            // onesweep_redo_kernel needs a grid that is resident at once -- at most 64 workgroups over all the launch's topics (a
            // workgroup of 1 024 threads keeps 130 KB of LDS: one per CU; the lanes of a host-buffer call may run up to four such
            // launches side by side on their streams: 4 x 64 = the chip's 256 CUs, so every launch's workgroups become resident
            // whatever the others do -- a workgroup waiting for a CU behind spinning ones of ANOTHER launch would otherwise be
            // a deadlock in the making)
            const int per_topic = 64 / (k.n < 64 ? k.n : 64);
            const dim3 grid(k.max_tiles < per_topic ? k.max_tiles : per_topic, k.n);
            with_sweep_class(b, [&](auto atomic, auto threads) {
                LA_LAUNCH((onesweep_redo_kernel<atomic(), threads()>), grid, dim3(threads()), 0, stream, b, j.pass_mask, j.status, items, j.base);
            });
            continue;
        }
        for (int d = 0; d < kDigits; ++d) {
            if (!((j.pass_mask >> d) & 1u)) continue;
            const int p = slot0 + d;
            if (b.tile_state) {
                with_sweep_class(b, [&](auto atomic, auto threads) {
                    LA_LAUNCH((onesweep_pass_kernel<atomic(), threads()>), dim3(k.max_tiles, k.n), dim3(threads()), 0, stream, b, p, j.status, items, j.base);
                });
                continue;
            }
            LA_LAUNCH(tile_count_kernel, dim3(b.n_tiles < 2048 ? b.n_tiles : 2048), dim3(kSortThreads), 0, stream, b, p);
            LA_LAUNCH(scan_group_sums_kernel, dim3(b.n_groups), dim3(kRadix), 0, stream, b, p);
            LA_LAUNCH(scan_offsets_kernel, dim3(b.n_groups), dim3(kRadix), 0, stream, b, p);
            if (b.atomic_rank) LA_LAUNCH(tile_scatter_kernel<true>, dim3(b.n_tiles), dim3(kSortThreads), 0, stream, b, p);
            else LA_LAUNCH(tile_scatter_kernel<false>, dim3(b.n_tiles), dim3(kSortThreads), 0, stream, b, p);
        }
    }
}

void sort_plan_and_passes(const SortJob& j, hipStream_t stream, hipEvent_t planned) {
    LA_LAUNCH(plan_kernel, dim3(kDigits, j.count), dim3(kRadix), 0, stream, j.b, j.items, j.base);
    if (planned) (void)hipEventRecord(planned, stream);
    sort_passes(j, stream, 0);
}

// The tail of sorts that may have gone keys first: ties into id order, then a new plan for the redo slots.
static hipError_t sort_repair_launch(const SortJob& j, hipStream_t stream) {
    static PerDeviceOnce lds_opt_in;
    const hipError_t e = lds_opt_in.run([] {
        // (exactly what the launch asks for: the kernel also has static LDS, and dynamic + static must fit the CU's 160 KB)
        return hipFuncSetAttribute((const void*)tie_repair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(2 * kRepairCap * sizeof(uint64_t)));
    });
    if (e != hipSuccess) return e;
    int64_t gs = (j.max_n / 2 + 255) / 256;
    if (gs > 4096) gs = 4096;
    LA_LAUNCH(tie_scan_kernel, dim3((unsigned)(gs < 1 ? 1 : gs), j.count), dim3(256), 0, stream, j.b, j.items, j.base);
    int64_t gx = (j.max_n + kRepairWindow - 1) / kRepairWindow;
    if (gx > 1024) gx = 1024;                                   // (128 KB of LDS each: one per CU at a time; windows grid-stride)
    LA_LAUNCH(tie_repair_kernel, dim3((unsigned)gx, j.count), dim3(kRepairThreads), (size_t)2 * kRepairCap * sizeof(uint64_t), stream,
              j.b, j.items, j.base);
    LA_LAUNCH(replan_kernel, dim3(j.count), dim3(64), 0, stream, j.b, j.items, j.base);
    return hipGetLastError();
}

hipError_t sort_launch(const LargeArgs& a, const SortJob& j, hipStream_t stream, hipEvent_t planned) {
    LA_LAUNCH(build_keys_kernel, dim3(keys_grid(j.max_n), j.count), dim3(256), 0, stream, a, j.b, j.items, j.base);
    if (j.keys_first) LA_LAUNCH(sample_scan_kernel, dim3(j.items ? 64 : 256, j.count), dim3(256), 0, stream, j.b, j.items, j.base);
    sort_plan_and_passes(j, stream, planned);
    if (!j.keys_first) return hipSuccess;
    const hipError_t e = sort_repair_launch(j, stream);
    if (e != hipSuccess) return e;
    sort_passes(j, stream, kDigits);
    return hipSuccess;
}

// ---- lab builds: the sweeps' instrumentation arrays (debug_read, la_launch.h) -------------------------------------------------
#ifdef LA_SWEEP_CLOCKS
LA_DEBUG_EXPORT la_debug_sweep_clocks(unsigned long long* out, int reset) { return debug_read(g_sweep_clocks, out, reset); }
#endif
#ifdef LA_LOOKBACK_STATS
LA_DEBUG_EXPORT la_debug_lookback_stats(unsigned long long* out, int reset) { return debug_read(g_lookback_stats, out, reset); }
#endif

}  // namespace la
