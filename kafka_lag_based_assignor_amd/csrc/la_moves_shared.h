// la_moves_shared.h -- what the two compile units of la_assignment_moves_device share: la_moves.hip (both assignments over ONE
// layout) and la_moves_layouts.hip (a layout each).  Constants, the mapping of a previous rank, the insert of a previous entry,
// the gained / lost bins and the launchers' host arithmetic.  No kernel lives here.
#pragma once
#include <algorithm>

#include "la_kernels.h"
#include "la_device.h"
#include "la_join.h"

namespace la {

namespace {

constexpr int kMovesThreads = 256;
constexpr int kMovesChunk = 4 * kMovesThreads;      // global form: entries of one workgroup step
constexpr int kMovesMaxTables = 16;                 // copies of the bins ...
constexpr int kMovesFewBins = 2048;                 // ... while all of them stay within this many counters (8 KiB)
constexpr int64_t kMovesMaxBinned = 1ll << 32;      // entries of a call whose moves 32-bit bins can count without wrapping
static_assert((kMovesLdsMaxPartitions & (kMovesLdsMaxPartitions - 1)) == 0, "2 x the limit is the table of the largest topic");
static_assert(2 * kMovesLdsMaxMembers + 1 >= kMovesFewBins, "one copy of the widest bins is the largest bin area");

__device__ __forceinline__ void global_add(int64_t* p, uint64_t v) {
    __hip_atomic_fetch_add((unsigned long long*)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

// previous rank -> that owner in today's ranks; false: a rank out of range (nothing is read or stored through it)
__device__ __forceinline__ bool owner_today(const MovesCall& c, int32_t p, int32_t* q) {
    const int32_t n_prev = c.map ? c.n_prev_members : c.n_members;
    if (p < -1 || p >= n_prev) return false;
    const int32_t r = p < 0 ? -1 : (c.map ? c.map[p] : p);
    if (r < -1 || r >= c.n_members) return false;
    *q = r;
    return true;
}

// one previous entry into its topic's table; returns status bits
template <int SCOPE>
__device__ __forceinline__ uint32_t insert_entry(const MovesCall& c, uint64_t* table, int bits, int64_t i) {
    const int32_t id = __builtin_nontemporal_load(c.prev_partition + i);
    const int32_t p = __builtin_nontemporal_load(c.prev_member_rank + i);
    int32_t q;
    if (!owner_today(c, p, &q)) return kStatusMoves;
    return table_insert<SCOPE>(table, bits, id, q);
}

// ARGS: a kernel's argument struct with the call `c` and the bins' geometry `tables` / `stride`
template <typename ARGS>
__device__ __forceinline__ void clear_bins(const ARGS& a, uint32_t* bins, int tid) {
    for (int i = tid; i < a.tables * a.stride; i += kMovesThreads) bins[i] = 0;
}

// the workgroup's bins into the outputs: one 64-bit global atomic per non-zero bin (behind a barrier)
template <typename ARGS>
__device__ __forceinline__ void flush_bins(const ARGS& a, const uint32_t* bins, int tid) {
    const uint32_t m = (uint32_t)a.c.n_members;
    for (uint32_t b = (uint32_t)tid; b < 2 * m; b += kMovesThreads) {
        uint64_t s = 0;
        for (int t = 0; t < a.tables; ++t) s += bins[(size_t)t * a.stride + b];
        if (s == 0) continue;
        if (b < m) { if (a.c.member_gained) global_add(a.c.member_gained + b, s); }
        else if (a.c.member_lost) global_add(a.c.member_lost + (b - m), s);
    }
}

// copies of `bins` counters (stride: bins made odd, so that the copies start on different banks): as many as stay within
// kMovesFewBins, a power of two up to kMovesMaxTables
inline void tables_for(int64_t bins, int32_t* tables, int32_t* stride) {
    const int64_t s = (bins < 1 ? 1 : bins) | 1;
    int t = 1;
    while (t * 2 <= kMovesMaxTables && (int64_t)t * 2 * s <= kMovesFewBins) t *= 2;
    *tables = t;
    *stride = (int32_t)s;
}

// Resident workgroups of a kernel for its dynamic LDS, per device; one word per (device, kernel): LDS bytes << 32 | workgroups.
// It remembers the last LDS size only (a caller that alternates between hints asks the runtime again: host arithmetic).
template <typename K>
hipError_t moves_resident(K kernel, int form, size_t lds, int* out) {
    static std::atomic<uint64_t> s_cache[32][8];
    int dev = 0, cus = 0, per_cu = 0;
    hipError_t e;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    const bool cached = dev >= 0 && dev < 32;
    if (cached) {
        const uint64_t c = s_cache[dev][form].load(std::memory_order_relaxed);
        if ((uint32_t)c != 0 && (c >> 32) == lds) { *out = (int)(uint32_t)c; return hipSuccess; }
    }
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kMovesThreads, lds)) != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    if (cus < 1) cus = 1;
    *out = cus * per_cu;
    if (cached) s_cache[dev][form].store(((uint64_t)lds << 32) | (uint32_t)*out, std::memory_order_relaxed);
    return hipSuccess;
}

inline int ceil_log2(int64_t x) {                  // smallest b with 2^b >= x, at least 1
    int b = 1;
    while (((int64_t)1 << b) < x) ++b;
    return b;
}

inline hipError_t grow_device(void** p, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return hipSuccess;
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    const size_t want = bytes + bytes / 4 + 256;
    const hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess) { *p = nullptr; return e; }
    *cap = want;
    return hipSuccess;
}

// The pinned list of a global form's topics and its device copy, `bytes` each; waits for the last call's copy out of h_items.
inline hipError_t moves_items_reserve(MovesScratch& s, size_t bytes) {
    hipError_t e;
    if (s.copied && (e = hipEventSynchronize(s.copied)) != hipSuccess) return e;
    if (bytes > s.h_items_cap) {
        if (s.h_items) { (void)hipHostFree(s.h_items); s.h_items = nullptr; s.h_items_cap = 0; }
        const size_t want = bytes + bytes / 4 + 256;
        if ((e = hipHostMalloc(&s.h_items, want, hipHostMallocDefault)) != hipSuccess) { s.h_items = nullptr; return e; }
        s.h_items_cap = want;
    }
    if ((e = grow_device(&s.d_items, &s.d_items_cap, bytes)) != hipSuccess) return e;
    if (!s.copied && (e = hipEventCreateWithFlags(&s.copied, hipEventDisableTiming)) != hipSuccess) return e;
    return hipSuccess;
}

}  // namespace

}  // namespace la
