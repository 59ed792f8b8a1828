// la_radix.h -- the device-wide radix sort (la_radix.hip) as its clients see it: the large path and the huge path's bins
// (la_large.hip) and the radix form of the grouping by member (la_group.hip).  An LSD radix sort, 8 bits per pass, stable, over
// (key64, id32): id digits, then key digits.  In file order:
//
//   device side       the digit and slot counts, the sort's control block and buffers (SortCtl, SortBufs), one topic of a
//                     batched launch (LargeItem, bind_item, LA_PICK_ITEM) and the grids of the kernels that walk a topic's
//                     elements (keys_grid, grid_256): what a client's own kernels and launches need around a sort.
//   host side         layout and scratch of a sort (SortLayout, sort_layout, sort_bind, scratch_reserve, sort_prepare), what one
//                     set of sort launches covers (SortClass, SortJob, sort_job_single) and the launch sequences (sort_launch:
//                     the whole sort; sort_plan_and_passes: of keys a client's kernel wrote; bounds_pass_mask).
//
// Environment hook read here, once per process: LA_KEYS_GRID (keys_grid).
#pragma once
#include <stdlib.h>

#include "la_kernels.h"

namespace la {

constexpr int kDigits = 12;            // 4 id digits + 8 key digits
constexpr uint32_t kAllPasses = (1u << kDigits) - 1;       // pass mask (bit p = digit p) of a sort whose caller knows no bounds
constexpr int kRadix = 256;

// Pass slots: 0 .. kDigits-1 are the sort's passes (digit = slot); kDigits .. 2*kDigits-1 are the same digits again, for the one
// case in which a keys-first sort has to be redone in full (see tie_repair_kernel); they are no-ops otherwise.
constexpr int kSlots = 2 * kDigits;
constexpr int kFinal = kSlots;         // ctl->cur[kFinal]: the buffer that holds the sorted data

struct SortCtl {
    uint32_t skip[kSlots];
    uint32_t cur[kSlots + 1];          // which buffer (0/1) holds the data before pass slot s; [kFinal]: after the last
    uint32_t unsorted_ids;             // != 0: input ids are not ascending
    uint32_t tie_heavy;                // build_keys: a key came up often in the sample (or filled a whole wavefront): many equal lags
    uint32_t keys_first;               // plan: the id passes are skipped, ties are put in id order by tie_repair_kernel
    uint32_t redo;                     // tie_repair: a run of equal keys did not fit its workgroup -> the redo slots sort in full
    uint32_t redo_arrived;             // onesweep_redo_kernel's grid barrier: workgroups that finished a redo pass (zeroed with ctl)
    uint32_t pad[10];
};

struct SortBufs {
    SortCtl* ctl;
    uint32_t* hist;                    // [kDigits][256]
    uint64_t* key[2];
    uint32_t* val[2];
    uint32_t* tile_off;                // [n_tiles][256] (a tile's 256 digit counts / offsets are one 1 KB row)
    uint32_t* group_sum;               // [n_groups][256] digit counts of kScanRows consecutive tiles
    // single-kernel passes (decoupled look-back): zeroed per sort together with ctl and hist
    uint32_t* ticket;                  // [kSlots] arrival counter of every pass slot
    uint32_t* gbase;                   // [kDigits][256] exclusive scan of hist: global first position of every digit
    unsigned long long* tile_state;    // [n_tiles][256] granules {tag = (pass + 1) << 2 | status, count}; null: multi-kernel passes
    int64_t n;
    int n_tiles;
    int n_groups;
    int atomic_rank;                   // ranks from returning LDS atomics (the device passed lds_atomic_order_test_kernel)
    int sweep_threads;                 // workgroup size of the single-kernel passes: 512 (tiles of 8 192) or 256 (4 096)
    // keys-first sorts (large n, shuffled ids): a hash table of SAMPLED keys (zeroed with ctl) tells whether some lag is so
    // frequent that its run could not be repaired in one workgroup; null: this sort never goes keys first
    uint32_t* samp;
    uint32_t samp_bits;                // table of 2^samp_bits counters
    uint32_t* tie_flag;                // [ceil(n / kRepairWindow)] != 0: a run of more than four equal keys starts in the window
    int keys_first_force;              // test hook: keys first whatever the sample says (long runs then take the redo slots)
};

// One large topic of a batched launch (large_topics_launch): kernels launched over SEVERAL topics at once read where their
// topic's partitions / consumers are and where its sort lives from a device array -- blockIdx.y (or an order list) picks the
// item -- instead of from the kernel arguments.  `items == nullptr` is the single-topic form: the arguments are the kernel's own.
// An item holds NO pointers: the per-partition arrays are the batch's (the kernel's own LargeArgs, shared by every item) and
// the sort's buffers are byte offsets into the scratch block, whose base is a kernel argument.  A pointer LOADED from memory
// is a generic pointer to the compiler -- every access through it a flat_* instruction (tests/test_isa_hazards.py) -- while
// one derived from a kernel argument is known to be global.
struct LargeItem {
    int64_t p0, n_part, c0, n_cons;
    int64_t n;
    int32_t n_tiles, n_groups;
    uint64_t o_ctl, o_hist, o_ticket, o_state, o_gbase, o_k0, o_k1, o_v0, o_v1;
    uint64_t o_samp;                   // 0: no sample table (this topic never sorts keys first)
    uint64_t o_flag;
    uint32_t samp_bits, pad;
};

// b.key[x] / b.val[x] with a run-time x, as a select: indexing the pointer pair of a LOCAL SortBufs dynamically would put the
// struct in scratch memory and bring the pointers back generic (flat_* accesses)
__device__ __forceinline__ uint64_t* key_buf(const SortBufs& b, uint32_t x) { return x ? b.key[1] : b.key[0]; }
__device__ __forceinline__ uint32_t* val_buf(const SortBufs& b, uint32_t x) { return x ? b.val[1] : b.val[0]; }

__device__ __forceinline__ void bind_item(LargeArgs& a, SortBufs& b, const LargeItem& it, char* scratch) {
    a.p0 = it.p0; a.n_part = it.n_part; a.c0 = it.c0; a.n_cons = it.n_cons;
    b.ctl = (SortCtl*)(scratch + it.o_ctl);
    b.hist = (uint32_t*)(scratch + it.o_hist);
    b.ticket = (uint32_t*)(scratch + it.o_ticket);
    b.tile_state = (unsigned long long*)(scratch + it.o_state);
    b.gbase = (uint32_t*)(scratch + it.o_gbase);
    b.key[0] = (uint64_t*)(scratch + it.o_k0);
    b.key[1] = (uint64_t*)(scratch + it.o_k1);
    b.val[0] = (uint32_t*)(scratch + it.o_v0);
    b.val[1] = (uint32_t*)(scratch + it.o_v1);
    b.samp = it.o_samp ? (uint32_t*)(scratch + it.o_samp) : nullptr;
    b.tie_flag = (uint32_t*)(scratch + it.o_flag);
    b.samp_bits = it.samp_bits;
    b.n = it.n;
    b.n_tiles = it.n_tiles;
    b.n_groups = it.n_groups;
}

// (a0 / b0 of a batched launch: the batch's arrays and flags; atomic_rank / sweep_threads of the launch's tile class)
#define LA_PICK_ITEM(a, b, a0, b0, items, scratch, which)  \
    LargeArgs a = a0;                                       \
    SortBufs b = b0;                                        \
    if (items) bind_item(a, b, (items)[which], scratch);

// grid of build_keys_kernel.  Every block ends by adding its non-zero digit counters (up to 12 x 256) to the global histograms with
// atomics, so beyond 512 blocks a block takes 2 048 partitions instead of 256 (grid stride), up to 1 024 blocks (2 048 from 16 M
// partitions on, where the flush is noise and the loads want every CU several times over).  1 M partitions (cfg5): 0.057 ->
// 0.040 ms; 4 M: 0.079 -> 0.074 ms (profiles/r05_aa_keys_grid.txt).
inline int keys_grid(int64_t n) {
    static const int forced = [] { const char* e = getenv("LA_KEYS_GRID"); return e ? atoi(e) : 0; }();   // (lab)
    const int64_t fine = (n + 255) / 256;
    if (forced > 0) return (int)(fine > forced ? forced : fine);
    if (fine <= 512) return (int)fine;
    const int64_t cap = n >= ((int64_t)16 << 20) ? 2048 : 1024;
    const int64_t coarse = (n + 2047) / 2048;
    const int64_t g = coarse > cap ? cap : coarse;
    return (int)(g < 512 ? 512 : g);
}

// grid of the grid-stride kernels of 256 threads: a thread per element, up to `cap` workgroups
inline int grid_256(int64_t n, int cap = 2048) {
    const int64_t g = (n + 255) / 256;
    return (int)(g > cap ? cap : g);
}

// ---- host side (defined in la_radix.hip) -----------------------------------------------------------------------------------------
// The sort's working set for n elements, in two parts: what a sort expects zeroed (ctl, hist and -- single-kernel passes --
// the arrival tickets and the look-back granules) and the rest.  Several topics sorted side by side put all their zero parts
// first, so that ONE memset clears them.
// `multi_kernel`: the four-kernel passes (count, scans, scatter) instead of the single-kernel ones; also taken when a
// digit count would not fit a granule's 32-bit count with room for the tag arithmetic (n >= 2^30).
struct SortLayout {
    int64_t n = 0;
    bool multi_kernel = false;
    int sweep_threads = 256, n_tiles = 0, n_groups = 0;
    size_t o_ctl = 0, o_hist = 0, o_ticket = 0, o_state = 0, o_samp = 0, o_flag = 0, zero_bytes = 0;  // offsets into the zero part
    int keys_first = 0;                                                                             // 0 never, 1 by the sample, 2 forced
    uint32_t samp_bits = 0;
    size_t o_gbase = 0, o_k0 = 0, o_k1 = 0, o_v0 = 0, o_v1 = 0, o_to = 0, o_gs = 0, data_bytes = 0;   // ... into the data part
};

SortLayout sort_layout(int64_t n, bool multi_kernel, bool may_sort_keys_first = false);
SortBufs sort_bind(const SortLayout& L, char* zero, char* data);
// grow-only; earlier work on `stream` may still use the old block
hipError_t scratch_reserve(LargeScratch& scratch, size_t bytes, hipStream_t stream);
// layout, scratch, bind and the memset of the zero part for ONE sort of n elements that has the scratch to itself
hipError_t sort_prepare(LargeScratch& scratch, int64_t n, hipStream_t stream, SortBufs* out, bool multi_kernel = false,
                        bool may_sort_keys_first = false);

// One tile class of a set of sort launches: `n` topics from item `first` on whose passes run `sweep_threads` wide -- grid.y
// picks the topic, grid.x is as wide as the class's largest topic (max_tiles).
struct SortClass {
    int first, n, sweep_threads, max_tiles;
};

// What one set of sort launches covers.  `items == nullptr`: ONE topic, its buffers b's own, one class of one topic
// (sort_job_single).  Otherwise `count` topics side by side, in tile-class order: b holds what they share (atomic_rank,
// keys_first_force), an item its topic's buffers as offsets from `base`.
struct SortJob {
    SortBufs b;
    const LargeItem* items;
    int count;
    char* base;
    SortClass cls[3];                  // (a sweep is 256, 512 or 1 024 threads wide)
    int n_cls;
    bool keys_first;                   // some topic may sort keys first: sample scan, tie repair and redo slots are launched
    int64_t max_n;                     // elements of the largest topic
    // passes the HOST knows can matter (bit p = digit p); the kernels of the others are not even launched.  The device-side
    // plan still decides among the launched ones (a launched pass whose digit turns out constant returns at once), and it marks
    // every pass outside the mask as skipped by itself -- the caller guarantees those digits are constant (key bits that cannot
    // be set) or the ids ascending.
    uint32_t pass_mask;
    uint32_t* status;
};

SortJob sort_job_single(const SortBufs& b, uint32_t pass_mask, uint32_t* status);
// plan + the sort's passes; keys, payloads, histograms and the unsorted-ids flag must already be in buffer 0.  `planned`
// (may be null) is recorded after the plan.
void sort_plan_and_passes(const SortJob& j, hipStream_t stream, hipEvent_t planned);
// A whole sort of the job's topics by (lag desc, id asc): keys, sample scan, plan, passes and -- where a topic may sort keys
// first -- the tie repair and the redo slots (no-ops unless a run of equal lags did not fit its workgroup).
hipError_t sort_launch(const LargeArgs& a, const SortJob& j, hipStream_t stream, hipEvent_t planned);
// the passes a caller's bounds (LA_FLAG_BOUNDS) leave possible
uint32_t bounds_pass_mask(const LargeArgs& a);

}  // namespace la
