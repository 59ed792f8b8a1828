// la_pinned_sort.h -- device code the two forms of the pinned assignment share: la_pinned.hip (one workgroup holds a topic in its
// LDS) and la_pinned_large.hip (the levels of a topic of any size).  The workgroup sort of LDS arrays both use for the active set
// of a level; the LDS form sorts its partitions with it too.
#pragma once
#include "la_coop.h"

namespace la {

// ascending by (key, tb) over the first n entries of LDS arrays (pay rides along); every thread of a workgroup of kPinnedThreads
// calls it with the same n, behind a barrier; ends behind one.  The direction-free bitonic network in plain HIP: the lower index
// of every pair keeps the smaller record, so the positions from n on, which no pair touches, stand for +infinity and any n sorts
// without padding.
template <bool PAYLOAD>
__device__ __forceinline__ void pinned_sort(uint64_t* key, uint32_t* tb, int32_t* pay, int n, int tid) {
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const bool mirror = j == (k >> 1);
            for (int t = tid; t < (np2 >> 1); t += kPinnedThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // bit j clear
                const int l = mirror ? (i ^ (k - 1)) : (i | j);           // i < l
                if (l < n) {
                    const uint64_t ki = key[i], kl = key[l];
                    const uint32_t ti = tb[i], tl = tb[l];
                    if (kl < ki || (kl == ki && tl < ti)) {
                        key[i] = kl; key[l] = ki;
                        tb[i] = tl; tb[l] = ti;
                        if (PAYLOAD) {
                            const int32_t pi = pay[i];
                            pay[i] = pay[l];
                            pay[l] = pi;
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace la
