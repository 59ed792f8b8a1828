// la_launch.h -- how the library launches a kernel and keeps its scratch: the launch counter, the per-device opt-in to large
// dynamic LDS, the resident-grid launcher of the report kernels (la_loads / la_moves / la_moves_layouts / la_verify / la_coop / la_sticky),
// their growable device buffer and staged list, the launchers' host arithmetic, and the read-out of a lab build's counters
// (la_radix / la_large / la_group).  Host code only: no kernel lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

namespace la {

// Kernel launches of the whole library, counted where they are issued: la_last_launches (lagassign.h) reports the difference
// over one call -- how a test asserts "one launch" for a batch whose bounds prove that every tile packs.  Process-wide (the
// lanes of a host-buffer call launch from their own threads), relaxed: a diagnostic, not a synchronisation point.
inline std::atomic<uint64_t> g_kernel_launches{0};
#define LA_LAUNCH(...)                                                        \
    do {                                                                      \
        ::la::g_kernel_launches.fetch_add(1, std::memory_order_relaxed);      \
        hipLaunchKernelGGL(__VA_ARGS__);                                      \
    } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device, and a process may hold contexts
// on several: one bit per device id remembers where a kernel has been opted in (ids >= 32: set on every launch).
// Calls may come from several host threads (one per shard lane), hence the atomic.
struct PerDeviceOnce {
    std::atomic<uint32_t> mask{0};
    template <typename F>
    hipError_t run(F&& set) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const uint32_t bit = (dev >= 0 && dev < 32) ? (1u << dev) : 0u;
        if (bit && (mask.load(std::memory_order_acquire) & bit)) return hipSuccess;
        if ((e = set()) != hipSuccess) return e;
        if (bit) mask.fetch_or(bit, std::memory_order_release);
        return hipSuccess;
    }
};

// Kernel may ask for up to MAX_LDS bytes of dynamic LDS on the current device (once per device and kernel)
template <auto Kernel, size_t MAX_LDS>
hipError_t opt_in_lds() {
    static PerDeviceOnce once;
    return once.run([] {
        return hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MAX_LDS);
    });
}

// compute units of the current device, at least 1 (asked once per device; ids >= 32: on every call)
inline hipError_t device_cus(int* out) {
    static std::atomic<int> s_cus[32];
    int dev = 0, cus = 0;
    hipError_t e;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    const bool cached = dev >= 0 && dev < 32;
    if (cached && (cus = s_cus[dev].load(std::memory_order_relaxed)) > 0) { *out = cus; return hipSuccess; }
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    if (cus < 1) cus = 1;
    if (cached) s_cus[dev].store(cus, std::memory_order_relaxed);
    *out = cus;
    return hipSuccess;
}

// Resident workgroups of Kernel on the current device for a workgroup size and its dynamic LDS (two gfx950 devices need not
// expose the same number of CUs).  The cache belongs to the kernel ITSELF -- every instantiation has its own -- one word per
// device: LDS bytes << 40 | threads << 24 | workgroups; several lanes may ask at once.  It remembers the LAST request only: a
// caller that alternates between two asks the runtime again on every call (host arithmetic, a few microseconds; a rebalance
// has one member count and one hint).
template <auto Kernel>
hipError_t resident_workgroups(int threads, size_t lds, int* out) {
    static std::atomic<uint64_t> s_cache[32];
    int dev = 0, cus = 0, per_cu = 0;
    hipError_t e;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    const bool cached = dev >= 0 && dev < 32;
    const uint64_t key = ((uint64_t)lds << 40) | ((uint64_t)threads << 24);
    if (cached) {
        const uint64_t w = s_cache[dev].load(std::memory_order_relaxed);
        if ((w & 0xFFFFFFu) != 0 && (w & ~(uint64_t)0xFFFFFFu) == key) { *out = (int)(w & 0xFFFFFFu); return hipSuccess; }
    }
    if ((e = device_cus(&cus)) != hipSuccess) return e;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, threads, lds)) != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    *out = (int)std::min<int64_t>((int64_t)cus * per_cu, 0xFFFFFF);
    if (cached) s_cache[dev].store(key | (uint32_t)*out, std::memory_order_relaxed);
    return hipSuccess;
}

// `grid` workgroups of Kernel, counted by la_last_launches; grid <= 0: nothing to do, nothing launched
template <auto Kernel, typename Args>
hipError_t launch_grid(int64_t grid, int threads, size_t lds, hipStream_t stream, const Args& a) {
    if (grid <= 0) return hipSuccess;
    LA_LAUNCH(Kernel, dim3((unsigned)grid), dim3((unsigned)threads), lds, stream, a);
    return hipGetLastError();
}

// `want` workgroups of a kernel whose workgroups walk their share of the work, or as many as are resident at once
template <auto Kernel, typename Args>
hipError_t launch_resident(int64_t want, int threads, size_t lds, hipStream_t stream, const Args& a) {
    if (want <= 0) return hipSuccess;
    int resident = 0;
    const hipError_t e = resident_workgroups<Kernel>(threads, lds, &resident);
    if (e != hipSuccess) return e;
    return launch_grid<Kernel>(std::min<int64_t>(want, resident), threads, lds, stream, a);
}

// the same for a kernel whose request may exceed the LDS it gets without asking: up to MAX_LDS bytes
template <auto Kernel, size_t MAX_LDS, typename Args>
hipError_t launch_resident_lds(int64_t want, int threads, size_t lds, hipStream_t stream, const Args& a) {
    const hipError_t e = opt_in_lds<Kernel, MAX_LDS>();
    if (e != hipSuccess) return e;
    return launch_resident<Kernel>(want, threads, lds, stream, a);
}

// ---- the launchers' host arithmetic ------------------------------------------------------------------------------------------
// a x b and a + b in size_t; false: the result does not fit
inline bool mul_ok(size_t a, size_t b, size_t* out) { return !__builtin_mul_overflow(a, b, out); }
inline bool add_ok(size_t a, size_t b, size_t* out) { return !__builtin_add_overflow(a, b, out); }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline int ceil_log2(int64_t x) {                  // smallest b with 2^b >= x, at least 1
    int b = 1;
    while (((int64_t)1 << b) < x) ++b;
    return b;
}

inline int64_t ceil_sqrt(int64_t x) {               // smallest r >= 1 with r r >= x
    int64_t r = (int64_t)__builtin_sqrt((double)x);
    if (r < 1) r = 1;
    while (r * r < x) ++r;
    while (r > 1 && (r - 1) * (r - 1) >= x) --r;
    return r;
}

// copies of `bins` LDS bins (stride: bins made odd, so that the copies start on different banks): as many as stay within
// `slots` bins, a power of two up to max_tables
inline void tables_for(int64_t bins, int64_t slots, int max_tables, int32_t* tables, int32_t* stride) {
    const int64_t s = (bins < 1 ? 1 : bins) | 1;
    int t = 1;
    while (t * 2 <= max_tables && (int64_t)t * 2 * s <= slots) t *= 2;
    *tables = t;
    *stride = (int32_t)s;
}

// ---- scratch that grows -------------------------------------------------------------------------------------------------------
// bytes + a quarter + 256, so that a slowly growing request does not allocate on every call; false: it does not fit
inline bool grown_size(size_t bytes, size_t* want) { return add_ok(bytes, bytes / 4 + 256, want); }

// A device buffer of at least `bytes` (the old content is gone when it grows).  hipErrorOutOfMemory, with the buffer empty and no
// sticky error left, when it cannot be had -- whatever the allocator's own reason.
inline hipError_t grow_device(void** p, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return hipSuccess;
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    size_t want = 0;
    if (!grown_size(bytes, &want)) return hipErrorOutOfMemory;
    if (hipMalloc(p, want) != hipSuccess) { *p = nullptr; (void)hipGetLastError(); return hipErrorOutOfMemory; }
    *cap = want;
    return hipSuccess;
}

// A list the host builds per call for a kernel to read: built in `h` (pinned), copied to `d` on the call's stream.  `copied` is
// the last copy out of `h`: the next call waits for it before it writes the list again.
struct StagedList {
    void* d = nullptr;
    void* h = nullptr;
    size_t d_cap = 0, h_cap = 0;
    hipEvent_t copied = nullptr;

    // room for `bytes` in both; waits for the last call's copy.  hipErrorOutOfMemory as grow_device.
    hipError_t reserve(size_t bytes) {
        hipError_t e;
        if (copied && (e = hipEventSynchronize(copied)) != hipSuccess) return e;
        if (bytes > h_cap) {
            if (h) { (void)hipHostFree(h); h = nullptr; h_cap = 0; }
            size_t want = 0;
            if (!grown_size(bytes, &want)) return hipErrorOutOfMemory;
            if (hipHostMalloc(&h, want, hipHostMallocDefault) != hipSuccess) {
                h = nullptr;
                (void)hipGetLastError();
                return hipErrorOutOfMemory;
            }
            h_cap = want;
        }
        if ((e = grow_device(&d, &d_cap, bytes)) != hipSuccess) return e;
        if (!copied && (e = hipEventCreateWithFlags(&copied, hipEventDisableTiming)) != hipSuccess) return e;
        return hipSuccess;
    }
    // the first `bytes` of h to d on `stream` (behind a reserve of at least as many)
    hipError_t upload(size_t bytes, hipStream_t stream) {
        const hipError_t e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, stream);
        return e != hipSuccess ? e : hipEventRecord(copied, stream);
    }
    void release() {
        if (copied) { (void)hipEventSynchronize(copied); (void)hipEventDestroy(copied); }
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        *this = StagedList{};
    }
};

// ---- lab builds: the kernels' instrumentation arrays (tools/*_probe.py find the exports with hasattr) -------------------------
// Reads a __device__ array of counters into `out` and, with `reset`, zeroes it.
template <typename T>
int debug_read(const T& symbol, unsigned long long* out, int reset) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(symbol), sizeof(T));
    if (e == hipSuccess && reset) {
        const T zero{};
        e = hipMemcpyToSymbol(HIP_SYMBOL(symbol), &zero, sizeof(T));
    }
    return e == hipSuccess ? 0 : -3;
}
#define LA_DEBUG_EXPORT extern "C" __attribute__((visibility("default"))) int

}  // namespace la
