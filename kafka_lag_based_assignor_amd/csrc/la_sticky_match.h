// la_sticky_match.h -- device code the two sticky re-matchings share: la_sticky.hip (one workgroup per topic) and
// la_coop_sticky_small.hip (the whole cooperative round with sticky ties in one workgroup).  The layout of a sort key, the
// workgroup scan over one value per thread and the bisection of a sorted key array.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "la_device.h"

namespace la {

// key = run start << 44 | (uint32) member << 12 | position: 12 bits of position, 32 of member, the top bits free so that no key
// is kNoKey.  kNoPos: a 16-bit index that is no position.
constexpr uint16_t kNoPos = 0xFFFF;
constexpr uint64_t kNoKey = ~0ull;
constexpr int kKeyRunShift = 44, kKeyMemberShift = 12;
constexpr uint64_t kKeyPosMask = (1ull << kKeyMemberShift) - 1;
static_assert(kKeyRunShift == kKeyMemberShift + 32 && kKeyRunShift + kKeyMemberShift < 64, "run | member | position, the top bits free: no key is kNoKey");

// Exclusive scan of one value per thread over the workgroup, every thread calling: MAX = the maximum (of unsigned values, so 0
// is the identity), otherwise the sum.  *total <- over all threads.  wave_tot: one LDS word per wavefront, free on return.
template <bool MAX>
__device__ __forceinline__ uint32_t workgroup_excl_scan(uint32_t v, uint32_t* wave_tot, int tid, int nt, uint32_t* total) {
    const int lane = tid & (kWave - 1), wave = tid / kWave, n_waves = nt / kWave;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= d) incl = MAX ? (o > incl ? o : incl) : incl + o;
    }
    if (lane == kWave - 1) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < n_waves; ++w) {
        const uint32_t x = wave_tot[w];
        if (w < wave) before = MAX ? (x > before ? x : before) : before + x;
        all = MAX ? (x > all ? x : all) : all + x;
    }
    __syncthreads();
    uint32_t excl = (uint32_t)__shfl_up((int)incl, 1);
    if (lane == 0) excl = 0;
    *total = all;
    return MAX ? (excl > before ? excl : before) : before + excl;
}

// first index in [0, n) whose key is not below x (n when there is none); the interval shrinks whatever the keys hold
__device__ __forceinline__ int first_not_below(const uint64_t* keys, int n, uint64_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace la
