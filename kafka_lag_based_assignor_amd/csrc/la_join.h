// la_join.h -- the per-topic hash join on a partition id, shared by la_moves.hip, la_moves_layouts.hip, la_verify.hip, la_sticky.hip and
// la_sticky_large.hip.
//
// An open-addressing table keyed by the id:
//
//     slot (one 64-bit word) = mark << 63 | (payload + 2) << 32 | (uint32) id        empty = 0
//
// (payload + 2 >= 1, so no live slot is 0; a payload below 2^30 keeps bit 63 free for the mark.)  INSERT is a 64-bit
// compare-and-swap on an empty slot, walking on from an occupied one -- an equal id on the way is a duplicate.  LOOKUP walks the
// same chain and sets the mark of its hit with an atomic OR: a hit that was marked already is a second lookup of that id.  A
// table that is at most half full (2^ceil(log2(2 P)) slots) ends every walk at a hit or an empty slot; every walk is bounded by
// the slot count all the same and returns kStatusInternal when it runs out.  No thread ever waits for another.
// SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP for a table in LDS, __HIP_MEMORY_SCOPE_AGENT for one in device memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "la_kernels.h"

namespace la {

constexpr uint64_t kSlotMark = 1ull << 63;

__device__ __forceinline__ uint64_t first_slot(int32_t id, int bits) {      // Fibonacci hashing: strided ids spread out
    return ((uint64_t)(uint32_t)id * 0x9E3779B97F4A7C15ull) >> (64 - bits);
}

// 0: inserted; kStatusMoves: the id is there already; kStatusInternal: no empty slot within the table (never expected)
template <int SCOPE>
__device__ __forceinline__ uint32_t table_insert(uint64_t* table, int bits, int32_t id, int32_t owner) {
    const uint64_t mask = (1ull << bits) - 1;
    const uint64_t word = ((uint64_t)(uint32_t)(owner + 2) << 32) | (uint32_t)id;
    uint64_t h = first_slot(id, bits);
    for (uint64_t n = 0; n <= mask; ++n) {
        unsigned long long seen = 0;
        if (__hip_atomic_compare_exchange_strong((unsigned long long*)(table + h), &seen, (unsigned long long)word,
                                                 __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE))
            return 0;
        if ((uint32_t)seen == (uint32_t)id) return kStatusMoves;
        h = (h + 1) & mask;
    }
    return kStatusInternal;
}

// 0: *owner <- the id's payload, its slot marked; kStatusMoves: no such id, or marked before (a duplicate)
template <int SCOPE>
__device__ __forceinline__ uint32_t table_lookup(uint64_t* table, int bits, int32_t id, int32_t* owner) {
    const uint64_t mask = (1ull << bits) - 1;
    uint64_t h = first_slot(id, bits);
    for (uint64_t n = 0; n <= mask; ++n) {
        const uint64_t w = __hip_atomic_load((unsigned long long*)(table + h), __ATOMIC_RELAXED, SCOPE);
        if (w == 0) return kStatusMoves;
        if ((uint32_t)w == (uint32_t)id) {
            const uint64_t old = __hip_atomic_fetch_or((unsigned long long*)(table + h), (unsigned long long)kSlotMark,
                                                       __ATOMIC_RELAXED, SCOPE);
            if (old & kSlotMark) return kStatusMoves;
            *owner = (int32_t)((uint32_t)(old >> 32) & 0x7FFFFFFFu) - 2;
            return 0;
        }
        h = (h + 1) & mask;
    }
    return kStatusInternal;
}

}  // namespace la
