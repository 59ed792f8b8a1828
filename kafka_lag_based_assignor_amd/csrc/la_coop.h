// la_coop.h -- host-visible declarations of la_cooperative_adjust_device (la_coop.hip), of la_cooperative_round[_device]
// (la_coop_small.hip) and of la_assign_pinned_device (la_pinned.hip, la_pinned_large.hip): the scratch, the call structs, the launchers (the status bit, kStatusCoop, stands with the others in
// la_kernels.h).  The entry points of lagassign.h over them, and the checks that make these call structs, are la_api_coop.hip.
#pragma once
#include "la_kernels.h"
#include "la_group_small.h"

namespace la {

// ---- cooperative rebalance: withhold what changes owner (la_coop.hip) -----------------------------------------------------------
// ONE table over the whole call, keyed by (topic, partition id): a key array (8 B per slot) and a payload array (4 B per slot,
// the claiming member) side by side in one allocation, 2^ceil(log2(2 n_owned)) slots.  Up to kMovesLdsMaxMembers members the
// insert launch bisects the owned offsets in LDS and the lookup launch counts in LDS bins; beyond it both go to device memory.
constexpr int kCoopLaunches = 2;            // insert | lookup: what la_last_launches reports at most (lagassign.h)
constexpr int64_t kCoopMaxOwned = 1ll << 40;      // beyond it the table is not even asked for (hipErrorOutOfMemory)

// ---- device code both compile units share: the key, its first slot, the bisection of an offset array --------------------------
__device__ __forceinline__ uint64_t coop_key(int32_t topic, int32_t id) {
    return ((uint64_t)(uint32_t)(topic + 1) << 32) | (uint32_t)id;
}

__device__ __forceinline__ uint64_t coop_first_slot(uint64_t key, int bits) {       // Fibonacci hashing over both halves of the key
    return (key * 0x9E3779B97F4A7C15ull) >> (64 - bits);
}

// largest r in [lo, hi) with off[r] <= x, for lo < hi; with offsets that do not ascend some r of that range all the same
__device__ __forceinline__ int64_t last_not_above(const int64_t* off, int64_t lo, int64_t hi, int64_t x) {
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The table as a kernel sees it: keys null = nobody owns anything.  la_coop.hip fills it; la_pinned.hip reads it too.
struct CoopTable {
    uint64_t* keys;
    uint32_t* owners;
    int32_t bits;               // 1 << bits slots
};

// the member that claimed (topic, id), or -1; *st |= kStatusInternal when the walk ran out (never expected: at most half full)
__device__ __forceinline__ int32_t coop_table_lookup(const CoopTable& t, int32_t topic, int32_t id, uint32_t* st) {
    if (!t.keys) return -1;
    const uint64_t mask = (1ull << t.bits) - 1;
    const uint64_t key = coop_key(topic, id);
    uint64_t h = coop_first_slot(key, t.bits);
    for (uint64_t w = 0; w <= mask; ++w) {
        const uint64_t seen = t.keys[h];
        if (seen == 0) return -1;
        if (seen == key) return (int32_t)t.owners[h];
        h = (h + 1) & mask;
    }
    *st |= kStatusInternal;
    return -1;
}

struct CoopScratch {            // of one shard, grown lazily: never the assign scratch (results kept on the device stay valid)
    void* table = nullptr;      // keys, then payloads
    size_t table_cap = 0;
    void* ranks = nullptr;      // la_cooperative_round_device, general form, without d_coop_member_rank: the adjusted ranks
    size_t ranks_cap = 0;
    void* prev = nullptr;       // la_cooperative_round_sticky_device, general form: the previous owners of the TARGET order
    size_t prev_cap = 0;
    void* stage_h = nullptr;    // la_cooperative_round (host buffers): inputs and outputs of a call, pinned ...
    size_t stage_h_cap = 0;
    void* stage_d = nullptr;    // ... and on the device: one copy each way
    size_t stage_d_cap = 0;
};

struct CoopCall {               // la_coop_args (lagassign.h), validated
    int32_t n_topics, n_members;
    int64_t n_partitions, n_owned;
    const int64_t* part_off;
    const int32_t *out_partition, *out_member_rank;
    const int64_t* owned_off;   // [M + 1]; null with n_owned == 0
    const int32_t *owned_topic, *owned_partition;
    int32_t *prev_owner, *coop_rank;      // outputs, each may be null
    int64_t *member_kept, *member_fresh, *member_pending, *member_release, *topic_withheld, *summary;
};

// Zeroes the counting outputs and the table's keys on `stream`, then at most kCoopLaunches launches (insert: skipped without
// owned entries; lookup: skipped without entries of today).  hipErrorOutOfMemory, with nothing enqueued, when the table cannot
// be had.  Sets kStatusCoop / kStatusShape / kStatusInternal.
hipError_t cooperative_adjust_launch(CoopScratch& s, const CoopCall& c, uint32_t* status, hipStream_t stream);
void coop_scratch_release(CoopScratch& s);

// The two halves of the table's making, for a caller that joins against it with a kernel of its own (la_pinned.hip).  reserve:
// the shard's table grown for n_owned entries, nothing enqueued (n_owned == 0: the empty table, keys null); hipErrorOutOfMemory when
// it cannot be had.  insert: the keys zeroed on `stream`, then the insert launch over c's owned arrays (n_topics, n_members,
// n_owned and the three owned pointers are all it reads of `c`); the number of claims, topic -1 entries included, is ADDED to
// *claimed (null: not wanted).  Nothing is enqueued with n_owned == 0.  Sets kStatusCoop / kStatusShape / kStatusInternal.
hipError_t coop_table_reserve(CoopScratch& s, int64_t n_owned, CoopTable* out);
hipError_t coop_table_insert_launch(const CoopTable& t, const CoopCall& c, int64_t* claimed, uint32_t* status, hipStream_t stream);

// ---- the pinned assignment: owned partitions stay, only the others are dealt out (la_pinned.hip) ---------------------------------
// One workgroup of kPinnedThreads per topic holds the topic in its LDS: up to kPinnedMaxPartitions partitions and
// kPinnedMaxConsumers consumers (the budget is proved by the static_asserts of la_pinned.hip).
constexpr int kPinnedMaxPartitions = 4096;
constexpr int kPinnedMaxConsumers = 2048;
constexpr int kPinnedThreads = 1024;
constexpr int kPinnedLaunches = 2;          // insert | topics: what la_last_launches reports at most (lagassign.h)

struct PinnedCall {             // la_device_batch + la_pinned_args (lagassign.h), validated
    int32_t n_topics, n_members, reset_latest;
    int64_t n_partitions, n_consumers, n_owned;
    const int64_t *part_off, *cons_off;
    const int32_t *pid, *cons_rank;
    const int64_t *begin, *end, *committed, *lag;      // as StickyCall
    const int64_t* owned_off;
    const int32_t *owned_topic, *owned_partition;
    int32_t *out_pid, *out_rank;
    int64_t* out_total;         // [K] or null
    int64_t* topic_free;        // [T] or null
    int64_t* summary;           // [4] or null
};

// ---- the pinned assignment of topics beyond the LDS limit (la_pinned_large.hip, LA_FLAG_PINNED_LARGE) ---------------------------
// The large form: all topics of a call with more than kPinnedMaxPartitions partitions (and at most kPinnedMaxConsumers consumers)
// side by side.  The order is the radix sort's of la_radix.h, a LargeItem per topic; the phases of the LDS kernel behind it are
// launches over regions in device memory, the levels one workgroup per topic with the bins in LDS.
constexpr int64_t kPinnedLargeMaxPartitions = (1 << 30) - 2;      // of one topic, and of a call's large topics together
// keys | plan | 12 digit passes for each of the sort's three tile classes | classify | chunk scan | compact | levels
constexpr int kPinnedLargeLaunches = 2 + 3 * 12 + 4;
constexpr int64_t kPinnedLargeStep = 1024;      // positions of a workgroup step = the chunk of the device-wide scan

struct PinnedBig {              // one large topic; every offset and size is the HOST's, inside [0, N] / [0, K]
    int64_t p0, np, c0, nc;     // its segments of the batch
    int64_t q0;                 // its first position in the concatenated list of all large topics' positions
    int64_t step0;              // its first workgroup step, numbered through the topics
    int64_t k0;                 // its first bin in the concatenated list of all large topics' consumers
    uint64_t o_ctl, o_k0, o_k1, o_v0, o_v1;      // its sort: control block and buffers, bytes from the working memory's base
    int32_t topic, pad;
};

struct PinnedLargeWork {        // the large form's device memory, as the kernels see it (every pointer a kernel argument)
    char* base;                 // the working memory: the sorts live at offsets from it
    const PinnedBig* big;       // ascending in topic; null: the call has no large topic
    int32_t n_big;
    int64_t n_pos, n_steps;
    uint8_t* flag;              // [L] 1: the position is free
    uint32_t* fpos;             // [L] the free positions (inside their topic), ascending, topic after topic
    uint32_t* cfree;            // [n_steps] free positions of every chunk; the scan makes it exclusive
    unsigned long long* tot;    // [1] all free positions
    unsigned long long* ctr;    // [4 n_big] pinned | foreign | unused | unused, of every large topic
    unsigned long long* btotal; // [consumers of the large topics] the bins' seeds
    uint32_t* bcount;
};

struct PinnedLargeScratch {     // of one shard, grown lazily: never the assign scratch (results kept on the device stay valid)
    void* work = nullptr;       // the sorts' buffers, per-position arrays and bins, one allocation carved into regions
    size_t work_cap = 0;
    StagedList list;            // the topic list and the sort's items
    // what pinned_large_reserve found for the call it was made for (host arithmetic only)
    int64_t n_big = 0, n_pos = 0, n_steps = 0, n_bins = 0;
};

// Lists the large topics from the host's offsets (validated by the caller: ascending inside [0, N] / [0, K]) into s.list and
// grows s.work for them.  Enqueues nothing; s.n_big == 0 afterwards: the batch holds no such topic and nothing was touched.
// hipErrorOutOfMemory when the memory cannot be had or the large topics hold more than kPinnedLargeMaxPartitions together.
hipError_t pinned_large_reserve(PinnedLargeScratch& s, const PinnedCall& c, const int64_t* h_part_off, const int64_t* h_cons_off);
// The large form behind a reserve for the same call and behind the table's insert launch: at most kPinnedLargeLaunches launches.
// *out: the list the LDS kernel skips.  Sets kStatusUnsorted / kStatusShape / kStatusOrder / kStatusInternal.
hipError_t pinned_large_enqueue(PinnedLargeScratch& s, const PinnedCall& c, const CoopTable& table, uint32_t* status,
                                hipStream_t stream, PinnedLargeWork* out);
void pinned_large_scratch_release(PinnedLargeScratch& s);

// Zeroes topic_free, summary and the table's keys on `stream`, then at most kPinnedLaunches launches (insert: skipped without
// owned entries; topics: skipped without topics).  hipErrorOutOfMemory, with nothing enqueued, when the table cannot be had.
// Sets kStatusUnsorted / kStatusCoop / kStatusShape / kStatusInternal.
// With `large` (LA_FLAG_PINNED_LARGE; h_part_off / h_cons_off validated by the caller) the topics over the partition limit are
// assigned by the large form between the two launches: at most kPinnedLargeLaunches more, its memory grown before anything is
// enqueued.  Without a large topic the flagged call enqueues what the unflagged one does and touches no scratch.
hipError_t pinned_launch(CoopScratch& s, const PinnedCall& c, uint32_t* status, hipStream_t stream, PinnedLargeScratch* large = nullptr,
                         const int64_t* h_part_off = nullptr, const int64_t* h_cons_off = nullptr);

// ---- the round in one call: the adjusted assignment AND every member's list of it (la_coop_small.hip) ---------------------------
// A call within ALL four limits is ONE launch of ONE workgroup that holds the (topic, id) table, the counters and the lists in
// its LDS (coop_round_small_kernel: no memset, no allocation, nothing in device memory beside the caller's arrays).  Any other
// call, or one with LA_COOP_FORCE_TABLE, is cooperative_adjust_launch followed by group_by_member_launch on the adjusted ranks.
// The LDS budget of every phase is proved by the static_asserts of la_coop_small.hip.
constexpr int kCoopSmallEntries = 2048;                 // N: the staged target (ids, ranks, topics) and the lists' seven arrays
constexpr int kCoopSmallOwned = 2048;                   // n_owned: 2 x this many slots of 12 B are the table
constexpr int kCoopSmallMembers = kTailGroupM - 2;      // M: the groups of the list builder are the members, "nobody" and the clamp
constexpr int kCoopSmallTopics = 2048;                  // T: T + 1 part offsets and T withheld counters
constexpr int kCoopSmallThreads = 1024;

struct CoopRoundCall {          // la_coop_round_args (lagassign.h), validated
    CoopCall c;
    int64_t* member_off;        // [M + 1]
    int32_t *grouped_topic, *grouped_partition;      // [N]; grouped_topic may be null
};

inline bool coop_round_is_small(const CoopCall& c) {
    return c.n_partitions <= kCoopSmallEntries && c.n_owned <= kCoopSmallOwned && c.n_members <= kCoopSmallMembers &&
           c.n_topics <= kCoopSmallTopics;
}

// The one-workgroup form (coop_round_is_small) unless force_table; otherwise at most kCoopLaunches launches and then those of
// group_by_member_launch on `large`, the adjusted ranks in s.ranks when the caller wants none (grown, like the table, before
// anything is enqueued: hipErrorOutOfMemory then).  Sets kStatusCoop / kStatusShape / kStatusInternal.
hipError_t cooperative_round_launch(CoopScratch& s, LargeScratch& large, const CoopRoundCall& r, bool force_table, uint32_t* status,
                                    hipStream_t stream);

// The round as the LAST launch of a zero-copy host call (la_assign_batch_cooperative, fused form): the one-workgroup kernel in its
// finishing form.  `r` must be within coop_round_is_small; r.c.out_partition / out_member_rank are the target in DEVICE memory,
// every other pointer of `r`, target_partition / target_rank (both or neither: the target as the caller wants it) and fin_flag lie
// in the call's mapped staging buffer.  The kernel reads `status` (the lane's device word, where the assignment kernels left their
// bits), adds the round's own, puts the word back to zero and stores `0x80000000 | bits` into fin_flag after everything else.
// Exactly one launch; hipErrorInvalidValue, with nothing enqueued, for a call outside the limits.
hipError_t cooperative_round_finish_launch(const CoopRoundCall& r, int32_t* target_partition, int32_t* target_rank,
                                           uint32_t* status, uint32_t* fin_flag, hipStream_t stream);

// ---- the round with sticky ties in one call (la_coop_sticky_small.hip) -----------------------------------------------------------
// la_cooperative_round_sticky_device: cooperative_adjust_launch for the previous owners, sticky_ties_launch, then
// cooperative_round_launch on the sticky order -- or, within ALL four limits below and without force_table, ONE launch of ONE
// workgroup that does the three in its LDS (coop_sticky_small_kernel; the LDS budget of every phase is proved by the
// static_asserts of la_coop_sticky_small.hip).  The limits are the round's.
constexpr int kCoopStickyEntries = kCoopSmallEntries;   // N: positions in 12 bits of a sort key, two key arrays of N in the table's LDS
constexpr int kCoopStickyOwned = kCoopSmallOwned;       // n_owned
constexpr int kCoopStickyMembers = kCoopSmallMembers;   // M
constexpr int kCoopStickyTopics = kCoopSmallTopics;     // T: T + 1 part offsets, four counters per topic

struct CoopStickyCall {         // la_device_batch + la_coop_sticky_args (lagassign.h), validated
    StickyCall s;               // the batch as la_sticky_ties_device reads it and its four outputs; prev_owner is not looked at
    CoopRoundCall r;            // the round; r.c's target (n_topics, n_partitions, part_off, out_partition, out_member_rank) is s's
    const int64_t* h_part_off = nullptr;      // non-null: LA_FLAG_STICKY_LARGE, the host's offsets (validated) for sticky_ties_launch
};

inline bool coop_sticky_is_small(const CoopCall& c) {
    return c.n_partitions <= kCoopStickyEntries && c.n_owned <= kCoopStickyOwned && c.n_members <= kCoopStickyMembers &&
           c.n_topics <= kCoopStickyTopics;
}

// The one-workgroup form (coop_sticky_is_small) unless force_table: exactly one launch, a topic over the batch's hint is passed
// through by the kernel itself (kStatusShape).  Otherwise the three launchers in turn, the previous owners in s.prev and, when
// the caller wants no adjusted ranks, s.ranks -- both, and with k.h_part_off the sticky scratch of the large topics, grown before
// anything is enqueued (hipErrorOutOfMemory then).  Sets kStatusCoop / kStatusSticky / kStatusShape / kStatusInternal.
hipError_t cooperative_round_sticky_launch(CoopScratch& s, StickyScratch& sticky, LargeScratch& large, const CoopStickyCall& k, bool force_table,
                                           uint32_t* status, hipStream_t stream);

// The sticky round as the LAST launch of a zero-copy host call (la_assign_batch_cooperative_sticky, fused form): the one-workgroup
// kernel in its finishing form.  `k` must be within coop_sticky_is_small; the target (k.r.c.out_partition / out_member_rank) lies
// in DEVICE memory, every other pointer of `k` -- part offsets, input ids, the lag source, the owned arrays, every output, each
// optional one null or not, k.s.sticky included -- target_partition / target_rank (both or neither: the target as the caller wants
// it) and fin_flag lie in the call's mapped staging buffer.  The lag source is read once, by index; k.h_part_off is not looked at.
// The kernel reads `status` (the lane's device word), adds the round's own bits, puts the word back to zero and stores
// `0x80000000 | bits` into fin_flag after everything else.  Exactly one launch; hipErrorInvalidValue, with nothing enqueued, for
// a call outside the limits, without fin_flag or with one target pointer alone.
hipError_t cooperative_round_sticky_finish_launch(const CoopStickyCall& k, int32_t* target_partition, int32_t* target_rank,
                                                  uint32_t* status, uint32_t* fin_flag, hipStream_t stream);

}  // namespace la
