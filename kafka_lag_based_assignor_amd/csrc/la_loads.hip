// la_loads.hip -- per-member roll-up of an assignment (la_member_loads_device, lagassign.h).
//
// Nothing in the reference computes it: the reference balances every topic on its own and prints one debug summary per topic
// (Main.java:279-306).  Over all topics of a rebalance, per member rank r:
//
//     partitions[r] = #{ i : out_member_rank[i] == r }         unassigned = #{ i : out_member_rank[i] == -1 }  (Main.java:211-213)
//     lag[r]        = sum of out_total_lag[k] over cons_rank[k] == r, Java long arithmetic (wraps)
//
// Two input streams with different keys -- N x 4 B of ranks to count, K x 12 B of (rank, total) pairs to sum -- are reduced by
// ONE launch: the first workgroups of the grid take the ranks, the rest the pairs.  A wrapping integer sum does not depend on
// the order of its adds, so atomics give the same bits on every run.
//
//   few members  (M <= kLoadsLdsMaxMembers): per-workgroup bins in LDS (32-bit counts, bin 0 = rank -1; 64-bit sums), one table
//                per lane while 64 tables fit (64 lanes on a handful of addresses would serialise), folded after the workgroup's
//                last element into one 64-bit global atomic add per non-zero bin.  The grid is what is resident, or less.
//   many members (beyond that, any M up to 2^31 - 1): 64-bit global atomic adds straight to the outputs -- with that many bins
//                two lanes rarely meet; rank -1 (one address for every topic without consumers) is counted in registers.
//
// Loads are 16-byte non-temporal accesses between a scalar head and tail, so a view that starts at any element of a larger
// buffer takes the same path.  Nothing is stored through a rank: a rank outside [-1, M) / [0, M) is skipped and raises
// kStatusLoads.  The outputs are zeroed on the stream before the launch (member_loads_launch).
#include <algorithm>

#include "la_kernels.h"
#include "la_device.h"

namespace la {

namespace {

constexpr int kLoadsThreads = 256;
constexpr int kLoadsLdsBytes = 32 * 1024;       // bins of one workgroup: 8192 counts or 4096 sums
constexpr int kLoadsMaxTables = kWave;          // one table per lane; waves share them (their adds are separate instructions)
constexpr int64_t kLoadsMaxPerBlock = 1ll << 31;   // ranks one workgroup counts before its flush: a 32-bit LDS counter cannot wrap
static_assert((int64_t)kLoadsLdsMaxMembers + 1 <= kLoadsLdsBytes / 8, "the sums of M members and the counts of M + 1 bins fit the LDS budget");

typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));     // one 16-byte access

struct LoadsArgs {
    // counts half: workgroups [0, grid_p)
    const int32_t* member_rank;     // [n]
    int64_t head_p, nvec_p, n;      // scalar head, 16-byte vectors behind it, all elements
    int64_t* member_partitions;     // [M]
    int64_t* unassigned;            // [1] or null
    // sums half: workgroups [grid_p, gridDim.x)
    const int32_t* cons_rank;       // [k]
    const int64_t* total_lag;       // [k]
    int64_t head_k, nvec_k, k;
    int64_t* member_lag;            // [M]
    uint32_t* status;
    int32_t n_members;
    int32_t grid_p;
    int32_t tables_p, stride_p;     // LDS form: tables (a power of two) and their stride in bins (odd: lanes spread over the banks)
    int32_t tables_k, stride_k;
    int32_t total16;                // total_lag + head_k is 16-byte aligned
};

template <bool LDS>
__global__ __launch_bounds__(kLoadsThreads) void member_loads_kernel(LoadsArgs a) {
    extern __shared__ uint64_t loads_bins[];
    const int tid = (int)threadIdx.x;
    const bool counts = (int)blockIdx.x < a.grid_p;
    bool bad = false;
    if (counts) {
        const uint32_t nbins = (uint32_t)a.n_members + 1u;              // bin 0 = rank -1, bin r + 1 = member r
        uint32_t* bins = reinterpret_cast<uint32_t*>(loads_bins);
        uint32_t* mine = bins + (size_t)(tid & (a.tables_p - 1)) * a.stride_p;
        uint64_t none = 0;                                              // many-member form: this thread's rank -1 entries
        if (LDS) {
            for (int i = tid; i < a.tables_p * a.stride_p; i += kLoadsThreads) bins[i] = 0;
            __syncthreads();
        }
        auto add = [&](uint32_t rank) {
            const uint32_t b = rank + 1u;
            if (b >= nbins) { bad = true; return; }
            if (LDS) __hip_atomic_fetch_add(mine + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else if (b == 0) ++none;
            else global_add(a.member_partitions + (b - 1u), 1);
        };
        auto add4 = [&](const U32x4& v) { add(v.x); add(v.y); add(v.z); add(v.w); };
        const U32x4* vec = reinterpret_cast<const U32x4*>(a.member_rank + a.head_p);
        const int64_t stride = (int64_t)a.grid_p * kLoadsThreads;
        int64_t v = (int64_t)blockIdx.x * kLoadsThreads + tid;
        for (; v + stride < a.nvec_p; v += 2 * stride) {               // two loads in flight per thread
            const U32x4 x0 = __builtin_nontemporal_load(vec + v);
            const U32x4 x1 = __builtin_nontemporal_load(vec + v + stride);
            add4(x0);
            add4(x1);
        }
        if (v < a.nvec_p) add4(__builtin_nontemporal_load(vec + v));
        if (blockIdx.x == 0) {                                          // the elements before and behind the vectors (<= 3 each)
            const int64_t tail0 = a.head_p + 4 * a.nvec_p;
            if (tid < a.head_p) add((uint32_t)a.member_rank[tid]);
            if (tail0 + tid < a.n) add((uint32_t)a.member_rank[tail0 + tid]);
        }
        if (LDS) {
            __syncthreads();
            for (uint32_t b = (uint32_t)tid; b < nbins; b += kLoadsThreads) {
                uint64_t s = 0;
                for (int t = 0; t < a.tables_p; ++t) s += bins[(size_t)t * a.stride_p + b];
                if (s == 0) continue;
                if (b > 0) global_add(a.member_partitions + (b - 1u), s);
                else if (a.unassigned) global_add(a.unassigned, s);
            }
        } else {
            none = wave_sum_u64(none);
            if (none != 0 && a.unassigned && (tid & (kWave - 1)) == 0) global_add(a.unassigned, none);
        }
    } else {
        const uint32_t nbins = (uint32_t)a.n_members;                   // bin r = member r
        uint64_t* bins = loads_bins;
        uint64_t* mine = bins + (size_t)(tid & (a.tables_k - 1)) * a.stride_k;
        if (LDS) {
            for (int i = tid; i < a.tables_k * a.stride_k; i += kLoadsThreads) bins[i] = 0;
            __syncthreads();
        }
        auto add = [&](uint32_t rank, uint64_t total) {
            if (rank >= nbins) { bad = true; return; }
            if (LDS) __hip_atomic_fetch_add(mine + rank, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else global_add(a.member_lag + rank, total);
        };
        const int grid_k = (int)gridDim.x - a.grid_p;
        const U32x4* vec = reinterpret_cast<const U32x4*>(a.cons_rank + a.head_k);
        const int64_t* tot = a.total_lag + a.head_k;
        const int64_t stride = (int64_t)grid_k * kLoadsThreads;
        for (int64_t v = (int64_t)((int)blockIdx.x - a.grid_p) * kLoadsThreads + tid; v < a.nvec_k; v += stride) {
            const U32x4 r = __builtin_nontemporal_load(vec + v);
            union { U32x4 q[2]; uint64_t e[4]; } t;
            if (a.total16) {
                const U32x4* tv = reinterpret_cast<const U32x4*>(tot + 4 * v);
                t.q[0] = __builtin_nontemporal_load(tv);
                t.q[1] = __builtin_nontemporal_load(tv + 1);
            } else {                                                    // the totals sit 8 bytes off the ranks' 16-byte grid
#pragma unroll
                for (int j = 0; j < 4; ++j) t.e[j] = (uint64_t)__builtin_nontemporal_load(tot + 4 * v + j);
            }
            add(r.x, t.e[0]); add(r.y, t.e[1]); add(r.z, t.e[2]); add(r.w, t.e[3]);
        }
        if ((int)blockIdx.x == a.grid_p) {
            const int64_t tail0 = a.head_k + 4 * a.nvec_k;
            if (tid < a.head_k) add((uint32_t)a.cons_rank[tid], (uint64_t)a.total_lag[tid]);
            if (tail0 + tid < a.k) add((uint32_t)a.cons_rank[tail0 + tid], (uint64_t)a.total_lag[tail0 + tid]);
        }
        if (LDS) {
            __syncthreads();
            for (uint32_t b = (uint32_t)tid; b < nbins; b += kLoadsThreads) {
                uint64_t s = 0;
                for (int t = 0; t < a.tables_k; ++t) s += bins[(size_t)t * a.stride_k + b];
                if (s != 0) global_add(a.member_lag + b, s);
            }
        }
    }
    if (__any(bad) && (tid & (kWave - 1)) == 0) atomicOr(a.status, kStatusLoads);
}

// elements before the first 16-byte boundary of an int32 array, at most n
inline int64_t head_elems(const int32_t* p, int64_t n) {
    const int64_t h = (int64_t)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / 4u);
    return h < n ? h : n;
}

}  // namespace

hipError_t member_loads_launch(int64_t n, const int32_t* member_rank, int64_t k, const int32_t* cons_rank,
                               const int64_t* total_lag, int32_t n_members, int64_t* member_partitions, int64_t* member_lag,
                               int64_t* unassigned, uint32_t* status, hipStream_t stream) {
    hipError_t e;
    const size_t out_bytes = (size_t)n_members * sizeof(int64_t);
    if (member_partitions && out_bytes && (e = hipMemsetAsync(member_partitions, 0, out_bytes, stream)) != hipSuccess) return e;
    if (member_lag && out_bytes && (e = hipMemsetAsync(member_lag, 0, out_bytes, stream)) != hipSuccess) return e;
    if (unassigned && (e = hipMemsetAsync(unassigned, 0, sizeof(int64_t), stream)) != hipSuccess) return e;
    if (!member_rank) n = 0;
    if (!cons_rank) k = 0;
    if (n <= 0 && k <= 0) return hipSuccess;

    LoadsArgs a{};
    a.n_members = n_members;
    a.status = status;
    a.member_rank = member_rank;
    a.n = n;
    a.head_p = n > 0 ? head_elems(member_rank, n) : 0;
    a.nvec_p = (n - a.head_p) / 4;
    a.member_partitions = member_partitions;
    a.unassigned = unassigned;
    a.cons_rank = cons_rank;
    a.total_lag = total_lag;
    a.k = k;
    a.head_k = k > 0 ? head_elems(cons_rank, k) : 0;
    a.nvec_k = (k - a.head_k) / 4;
    a.member_lag = member_lag;
    a.total16 = k > 0 && ((uintptr_t)(total_lag + a.head_k) & 15u) == 0;

    const bool lds = n_members <= kLoadsLdsMaxMembers;
    size_t lds_bytes = 0;
    a.tables_p = a.tables_k = 1;
    a.stride_p = a.stride_k = 1;
    if (lds) {
        tables_for((int64_t)n_members + 1, kLoadsLdsBytes / 4, kLoadsMaxTables, &a.tables_p, &a.stride_p);
        tables_for((int64_t)n_members, kLoadsLdsBytes / 8, kLoadsMaxTables, &a.tables_k, &a.stride_k);
        const size_t bp = n > 0 ? (size_t)a.tables_p * a.stride_p * 4 : 0, bk = k > 0 ? (size_t)a.tables_k * a.stride_k * 8 : 0;
        lds_bytes = bp > bk ? bp : bk;
    }
    int resident = 0;
    e = lds ? resident_workgroups<member_loads_kernel<true>>(kLoadsThreads, lds_bytes, &resident)
            : resident_workgroups<member_loads_kernel<false>>(kLoadsThreads, 0, &resident);
    if (e != hipSuccess) return e;

    // Workgroups per half: what its vectors need (two per thread and pass for the ranks, one for the pairs), at least one where
    // the half has an element at all; beyond what is resident the grid is shared out by the bytes each half reads.
    auto ceil_div = [](int64_t x, int64_t y) { return (x + y - 1) / y; };
    int64_t gp = n > 0 ? std::max<int64_t>(1, ceil_div(a.nvec_p, 2 * kLoadsThreads)) : 0;
    int64_t gk = k > 0 ? std::max<int64_t>(1, ceil_div(a.nvec_k, kLoadsThreads)) : 0;
    if (gp + gk > resident) {
        if (gp > 0 && gk > 0) {
            const double share = 4.0 * (double)n / (4.0 * (double)n + 12.0 * (double)k);
            int64_t want_p = (int64_t)(share * resident);
            want_p = std::min<int64_t>(std::max<int64_t>(want_p, 1), std::max(resident - 1, 1));
            const int64_t want_k = std::max<int64_t>(resident - want_p, 1);
            gp = std::min(gp, want_p);
            gk = std::min(gk, want_k);
        } else {
            gp = std::min<int64_t>(gp, resident);
            gk = std::min<int64_t>(gk, resident);
        }
    }
    gp = std::max(gp, ceil_div(n, kLoadsMaxPerBlock));                  // (only a buffer of terabytes gets here)
    if (gp + gk > 0x7FFFFFFF) return hipErrorInvalidValue;
    a.grid_p = (int32_t)gp;
    return lds ? launch_grid<member_loads_kernel<true>>(gp + gk, kLoadsThreads, lds_bytes, stream, a)
               : launch_grid<member_loads_kernel<false>>(gp + gk, kLoadsThreads, 0, stream, a);
}

}  // namespace la
