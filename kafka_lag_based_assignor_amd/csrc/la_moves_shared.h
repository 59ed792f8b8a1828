// la_moves_shared.h -- what the two compile units of la_assignment_moves_device share: la_moves.hip (both assignments over ONE
// layout) and la_moves_layouts.hip (a layout each).  Constants, the mapping of a previous rank, the insert of a previous entry
// and the gained / lost bins (la_coop.hip counts in bins of the same geometry).  No kernel lives here; the launchers' plumbing
// is la_launch.h's.
#pragma once
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

}  // namespace

}  // namespace la
