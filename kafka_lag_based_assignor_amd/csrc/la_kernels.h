// la_kernels.h -- host-visible declarations of the kernel launchers (internal to the library).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "la_launch.h"

namespace la {

// device status word bits (la_ctx::d_status)
constexpr uint32_t kStatusShape = 1u;      // a topic exceeded the shape hint
constexpr uint32_t kStatusUnsorted = 2u;   // a topic's cons_rank segment is not strictly ascending
constexpr uint32_t kStatusInternal = 4u;   // a look-back walk of the radix sort gave up waiting (never expected: a bounded spin
                                           // exists so that a scheduling surprise ends as an error, not as a hung device)

constexpr uint32_t kStatusOrder = 8u;      // the radix sort's result is not in order (emit_ids_kernel / member_emit_kernel compare neighbours
                                           // on their way through): the lane-order property the atomic ranking relies on did not
                                           // hold under load.  Never expected; a checked error instead of a silently wrong assignment

constexpr uint32_t kStatusWire = 16u;      // la_pack_results_on: a partition id or member rank does not fit the wire format it was given

constexpr uint32_t kStatusSparse = 32u;    // la_assign_batch_sparse: none_index is not ascending, or points outside the batch

constexpr uint32_t kStatusBounds = 64u;    // LA_FLAG_BOUNDS: a lag or a partition id lies outside the bounds the caller guaranteed

constexpr uint32_t kStatusLoads = 128u;    // la_member_loads_device: a member rank outside [-1, M) / a consumer rank outside [0, M)

constexpr uint32_t kStatusMoves = 256u;    // la_assignment_moves_device: a duplicate partition id inside a topic, a current id without a
                                           // previous one (one layout), a rank (previous, mapped or current) or a d_prev_topic
                                           // entry (two layouts) out of range

constexpr uint32_t kStatusCoop = 2 * kStatusMoves;      // la_cooperative_adjust_device: a target rank outside [-1, M), an owned
                                                        // topic outside [-1, T), or a (topic, partition id) claimed twice

constexpr uint32_t kStatusSticky = 2 * kStatusCoop;     // la_sticky_ties_device: a duplicate id in a topic's input segment, or an
                                                        // output id that is no input id of its topic or appears twice

// Every status bit is listed here: a new one that repeats a value, or is not a single bit, does not compile.
constexpr uint32_t kStatusBits[] = {kStatusShape, kStatusUnsorted, kStatusInternal, kStatusOrder,  kStatusWire,  kStatusSparse,
                                    kStatusBounds, kStatusLoads,   kStatusMoves,    kStatusCoop,   kStatusSticky};
constexpr bool status_bits_distinct() {
    uint32_t seen = 0;
    for (uint32_t b : kStatusBits) {
        if (b == 0 || (b & (b - 1)) != 0 || (seen & b) != 0) return false;
        seen |= b;
    }
    return true;
}
static_assert(status_bits_distinct(), "every status bit is one bit of its own");

constexpr int32_t kTileNoDefer = 8;       // TileArgs::flags: the bounds prove that every tile packs -- no deferred list, no wide
                                          // launch; a tile that does not pack after all raises kStatusBounds
constexpr int32_t kTileWireOut = 16;      // TileArgs::flags: out_wire instead of out_pid / out_rank (needs kTileNoDefer)
constexpr int32_t kTileSkipOversize = 4;  // TileArgs::flags: topics beyond the tile belong to another path, no error
constexpr int32_t kTileAlwaysStage2 = 32; // TileArgs::flags: (lab hook, LA_TILE_ALWAYS_STAGE2) never skip the second-stage `begin` loads
// TileArgs::begin_sparse_max unless LA_TILE_BEGIN_SPARSE_MAX says otherwise (lab hook; 0: always the vector form).  At the
// target's 1 % of partitions without a committed offset a 512-partition wavefront holds 5.1 of them on average.  32 since a
// pass serves all eight ballots: 16 and 32 are level at the target, 32 is 0.9 % faster at 5 % (25.6 per wavefront) and level
// with the vector form at 10 %; 64 is slower than the vector form from 5 % on (profiles/tile_begin_onetrip.txt).
constexpr int32_t kTileBeginSparseMax = 32;

constexpr int64_t kTileMaxPartitions = 1024;   // 64 lanes x 16 records
constexpr int64_t kTileMaxConsumers = 64;      // one consumer bin per lane
constexpr int64_t kLargeMaxConsumers = 8192;   // large path: 8 bins per thread x 1024 threads

// The tail of a small rebalance's ONE launch (tile kernel, single-launch form: the whole batch resident at once).  Every
// workgroup counts itself done on `counter`; the last one builds every member's list from the results the others wrote
// (group_small_body_staged, la_group_small.h; skipped when member_off is null: an ungrouped call) and stores `done | status` where the
// calling thread is spinning -- assignment, lists and completion in one launch instead of three (Main.java:147-156).
struct TileTail {
    int32_t enabled;            // 0: no tail (every launch but a zero-copy small call's)
    int32_t n_members;
    int32_t n;                  // entries (partitions of the batch), <= kSmallGroupN when the lists are wanted
    int32_t pad_;
    int64_t n_topics;
    const int64_t* part_off;    // of the WHOLE batch, from topic 0 (what grouped_topic indexes)
    const int32_t* out_pid;     // the launch's own results
    const int32_t* out_rank;
    int64_t* member_off;        // null: no lists
    int32_t* grouped_topic;     // may be null
    int32_t* grouped_partition;
    uint32_t* counter;          // device word, zero between calls (the last workgroup resets it)
    uint32_t* fin_flag;         // host word (coherent, mapped)
};

// Arguments of the fused wave-tile kernel (all device pointers).
struct TileArgs {
    int64_t n_topics;
    int64_t n_total;            // partitions in the whole batch (loads are clamped to it)
    int64_t k_total;            // consumer entries in the whole batch
    const int64_t* part_off;
    const int32_t* pid;
    const int64_t* begin;       // may be null (treated as 0; only read when !reset_latest)
    const int64_t* end;
    const int64_t* committed;
    const int64_t* lag;         // non-null: precomputed lags, offsets ignored
    const int64_t* cons_off;
    const int32_t* cons_rank;
    int32_t* out_pid;
    int32_t* out_rank;
    int64_t* out_total;         // may be null
    uint32_t* status;
    int32_t reset_latest;
    int32_t flags;              // LA_FLAG_* of the batch (test hooks) | kTileSkipOversize
    // tiles the packed kernel leaves to the wide kernel (LA_ALGO_AUTO): a counter pair that alternates
    // per launch (the wide kernel zeroes the other one), and the list of tile ids
    // non-null: slot s of the launch is topic topic_list[s] (shape classes of a ragged batch); null: topic s
    const int32_t* topic_list;
    int32_t* defer_count;
    int32_t* defer_count_next;
    int32_t* defer_list;
    TileTail tail;              // honoured by the single-launch form only (wave_tile_launch says whether it was)
    // LA_FLAG_WIRE_OUT: results as wire elements ((rank + 1) << wire_id_bits) | id of wire_bytes (2 or 4) each instead of the
    // two int32 arrays; only with kTileNoDefer (one launch of the packed-record kernel, 32-bit indexing)
    void* out_wire;
    int32_t wire_bytes, wire_id_bits;
    // stage 2 of a wavefront in which at most this many elements lack a committed offset fetches exactly those `begin` words
    // through scalar loads; more than that (or 0 here) take the vector form.  Negative: the launcher decides (kTileBeginSparseMax
    // in a launch that fills the chip, 0 in one round of wavefronts)
    int32_t begin_sparse_max;
};

// bytes of defer_list a launch over n_topics topics may need (one tile holds >= 1 topic)
inline size_t wave_tile_defer_bytes(int64_t n_topics) { return (size_t)(n_topics > 0 ? n_topics : 1) * sizeof(int32_t); }

inline bool wave_tile_fits(int64_t max_p, int64_t max_c) {
    return max_p <= kTileMaxPartitions && max_c <= kTileMaxConsumers;
}
void wave_tile_pick(int64_t max_p, int64_t max_c, int* L, int* E);
// true when ids in [0, max_id] and lags in [0, max_lag] pack into 64-bit records in every tile of the shape the launch would pick
bool wave_tile_always_packs(int64_t max_p, int64_t max_c, int64_t max_lag, int64_t max_id);
// mode: 0 = rounds, record format picked per wavefront; 1 = rounds, wide records forced; 2 = literal argmin
// *tail_done (may be null) <- true when a.tail.enabled and the launch was the single-launch form, whose last workgroup runs
// the tail; otherwise the caller finishes the call with its own launches.
hipError_t wave_tile_launch(TileArgs a, int64_t max_p, int64_t max_c, int mode, hipStream_t stream, bool* tail_done = nullptr);

// Elementwise lag: out_lag[i] = computePartitionLag(...)   (Main.java:376-404)
hipError_t lag_launch(int64_t n, const int64_t* begin, const int64_t* end, const int64_t* committed,
                      bool reset_latest, int64_t* out_lag, hipStream_t stream);

// begin[idx[j] - base] = val[j] for the m entries of a sparse begin list cut for positions [lo, hi); sets kStatusSparse.
hipError_t sparse_begin_launch(int64_t m, const int64_t* idx, const int64_t* val, int64_t base, int64_t lo, int64_t hi,
                               int64_t* begin, uint32_t* status, hipStream_t stream);

// The last launch of a zero-copy small call: *h_flag = 0x80000000 | *d_status (h_flag in coherent host memory).
hipError_t finish_status_launch(const uint32_t* d_status, uint32_t* h_flag, hipStream_t stream);
hipError_t wake_launch(hipStream_t stream);                  // one empty kernel (la_wake, for the streams its dummy call does not use)

// Checks that every topic's cons_rank segment is strictly ascending; sets kStatusUnsorted.
hipError_t check_consumers_launch(int64_t n_topics, const int64_t* cons_off, const int32_t* cons_rank,
                                  uint32_t* status, hipStream_t stream);

// ---- block path (la_block.hip): one workgroup per topic, everything in LDS --------------------
constexpr int64_t kBlockMaxPartitions = 8192;    // with up to kBlockMaxConsumers consumers
constexpr int64_t kBlockMaxConsumers = 2048;
constexpr int64_t kBlockWidePartitions = 16384;  // with up to kBlockWideConsumers consumers (16 records per thread)
constexpr int64_t kBlockWideConsumers = 1024;
constexpr int kBlockClasses = 5;               // LDS / workgroup size classes, see block_class()

struct BlockArgs {
    const int64_t* part_off;    // the batch's offsets (device)
    const int64_t* cons_off;
    const int32_t* list;        // topic indices this launch handles (device); null: inline_list
    int32_t n_list;
    int32_t inline_list[8];     // a handful of topics travel in the kernel arguments: no list copy
    const int32_t* pid;
    const int64_t* begin;
    const int64_t* end;
    const int64_t* committed;
    const int64_t* lag;
    const int32_t* cons_rank;
    int32_t* out_pid;
    int32_t* out_rank;
    int64_t* out_total;
    uint32_t* status;
    int32_t reset_latest;
    int32_t np_cap, nc_cap;     // LDS capacity in records / bins, set by the launcher
    int32_t dense_ids;          // set by the launcher: ids that are a permutation of 0 .. P-1 are placed by ONE scatter, not by digit passes
    int32_t key32_greedy;       // set by the launcher: 65 .. 256 consumers with packed totals take greedy_one_wave_key32
    int32_t radix_sort;         // set by the launcher: records that pack into one word are sorted by the workgroup's LSD radix
                                // sort (block_sort_radix) -- needs ranks from returning LDS atomics (large_atomic_rank_supported)
};

inline bool block_fits(int64_t p, int64_t c) {
    return (p <= kBlockMaxPartitions && c <= kBlockMaxConsumers) || (p <= kBlockWidePartitions && c <= kBlockWideConsumers);
}
inline int block_class(int64_t p, int64_t c) {
    if (p <= 512 && c <= 256) return 0;
    if (p <= 2048 && c <= 256) return 1;
    if (p <= 4096 && c <= 1024) return 2;
    if (p <= kBlockMaxPartitions) return 3;
    return 4;
}
hipError_t block_launch(BlockArgs a, int cls, hipStream_t stream);

// ---- large-topic path (device-wide radix sort, la_radix.hip + one-workgroup greedy, la_large.hip) ---------------------
// LA_FLAG_PROFILE: HIP events around the phases of the first large topic of a call (la_last_phase_times)
struct LargeProfile {
    hipEvent_t ev[4] = {};      // before the keys kernel, after the plan, after the last pass, after the greedy
    bool armed = false;         // the current call asked for it
    bool recorded = false;      // ev[] hold a topic's phases
    int64_t n = 0;              // its partitions
};

struct LargeScratch {
    void* buf = nullptr;
    size_t cap = 0;
    LargeProfile prof;
    // several large topics side by side (large_topics_launch): their argument blocks are built in a pinned slot (two, used in
    // turn: a slot is rewritten only after the copy that read it has completed) and copied to d_items on the call's stream
    struct Stage {
        void* h = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr;
    } stage[2];
    unsigned stage_next = 0;
    void* d_items = nullptr;
    size_t d_items_cap = 0;
};

struct LargeArgs {
    int64_t p0, n_part;         // partition segment of the topic
    int64_t c0, n_cons;         // consumer segment of the topic
    const int32_t* pid;
    const int64_t* begin;
    const int64_t* end;
    const int64_t* committed;
    const int64_t* lag;
    const int32_t* cons_rank;
    int32_t* out_pid;
    int32_t* out_rank;
    int64_t* out_total;
    uint32_t* status;
    int32_t reset_latest;
    int32_t no_sample_sort;     // 1 = LA_FLAG_NO_SAMPLE_SORT: every greedy round sorts its bins with the full network;
                                // 2 = LA_FLAG_SAMPLE_TIGHT: bucket limit 6, so sample-sorted and fallback rounds interleave
    int32_t no_run_merge;       // LA_FLAG_NO_RUN_MERGE: greedy rounds never merge ascending runs (they sort as if there were none)
    int32_t sort_multi_kernel;  // LA_FLAG_SORT_MULTIKERNEL: four kernels per radix pass (count, scans, scatter) instead of one
    int32_t no_moved_sort;      // LA_FLAG_NO_MOVED_SORT: greedy rounds never sort only the bins that move
    int64_t max_lag_hint;       // LA_FLAG_BOUNDS: 0 <= lag <= max_lag_hint and 0 <= id <= max_id_hint for every partition (the caller's
    int64_t max_id_hint;        // guarantee), or -1: radix passes over digits the bounds rule out are not even launched (round 6)
    int32_t rounds_follow;      // 1: greedy_rounds_kernel and map_ranks_kernel follow emit_ids_kernel -- the three agree on the narrow form of
                                // the rounds' lags and results (rounds_io, la_large.hip)
};

// Once per device at context creation (synchronous): checks the hardware property the radix sort's atomic ranking relies on
// (la_radix.hip, as large_atomic_rank_supported; the launchers below are la_large.hip's).
hipError_t large_init_device();
int large_atomic_rank_supported();      // of the current device: 1 = ranks come from returning LDS atomics, 0 = match form
hipError_t large_topic_launch(LargeScratch& scratch, const LargeArgs& a, bool argmin, hipStream_t stream);
// `count` large topics (each with n_part > 0 and at most kLargeMaxConsumers consumers) SIDE BY SIDE: the per-topic loop of
// assign(Map,Map) (Main.java:177-184) is independent across topics, so every phase is one launch over all of them -- keys,
// plan, each radix pass (grid.y = topic), ids, one greedy workgroup per topic, ranks -- instead of ~15 launches and a
// one-CU chain per topic, one topic after another.  Falls back to that serial form for a single topic and for the
// four-kernel-pass test hook.
hipError_t large_topics_launch(LargeScratch& scratch, const LargeArgs* args, int count, hipStream_t stream);
// A topic with more than kLargeMaxConsumers consumers: bins in HBM, every round one stable device sort of the bins + one
// pass that hands the round's partitions out (ceil(P / C) rounds of ~11 launches).  Any C up to 2^31 - 1.
hipError_t huge_topic_launch(LargeScratch& scratch, const LargeArgs& a, hipStream_t stream);
void large_scratch_release(LargeScratch& scratch);
// Waits for the profiled topic's events; ms[3] = keys + plan, sort passes (+ tie repair), ids + greedy; passes[4] = active id
// passes, active key passes, 1 if the sort went keys first, 1 if it had to be redone in full.
hipError_t large_profile_read(LargeScratch& scratch, float* ms, int* passes, int64_t* n);

// ---- grouping by member (la_group.hip) ------------------------------------------------------------------------------------
// Stable grouping of the n assignment entries by member rank (see la_group_by_member in lagassign.h).
hipError_t group_by_member_launch(LargeScratch& scratch, int64_t n, int32_t n_members, int64_t n_topics,
                                  const int64_t* part_off, const int32_t* out_partition, const int32_t* member_rank,
                                  int64_t* member_off, int32_t* grouped_topic, int32_t* grouped_partition,
                                  int32_t* grouped_entry, uint32_t* status, hipStream_t stream, uint32_t* fin_flag = nullptr,
                                  bool* fin_done = nullptr);
// (fin_flag: a zero-copy call's completion word in host memory; when the one-workgroup form runs it also finishes the call --
//  *fin_done says whether it did, otherwise the caller launches finish_status_launch)

// ---- narrow wire format of the all-gather (la_wire.hip) -----------------------------------------------------------
void wire_format_for(int64_t max_partition_id, int64_t n_members, int* elem_bytes, int* id_bits);     // pure host code
bool wire_format_valid(int elem_bytes, int id_bits);
hipError_t wire_pack_launch(int64_t n, const int32_t* pid, const int32_t* rank, int elem_bytes, int id_bits, void* out,
                            uint32_t* status, hipStream_t stream);
hipError_t wire_unpack_launch(int64_t n, const void* in, int elem_bytes, int id_bits, int32_t* pid, int32_t* rank,
                              hipStream_t stream);

// ---- per-member roll-up of an assignment (la_loads.hip) -----------------------------------------------------------------
// Up to this many members the bins live in LDS (per-workgroup tables, one global atomic per non-zero bin and workgroup); beyond
// it every element is one 64-bit global atomic add.  4096 sums of 8 bytes = the 32 KiB of LDS a workgroup takes.
constexpr int32_t kLoadsLdsMaxMembers = 4095;
// Zeroes the outputs on `stream`, then ONE launch over both inputs.  member_rank == null: no counts (member_partitions and
// unassigned are not touched); cons_rank == null: no sums.  A rank out of range is skipped and raises kStatusLoads.
hipError_t member_loads_launch(int64_t n, const int32_t* member_rank, int64_t k, const int32_t* cons_rank,
                               const int64_t* total_lag, int32_t n_members, int64_t* member_partitions, int64_t* member_lag,
                               int64_t* unassigned, uint32_t* status, hipStream_t stream);

// ---- who moved between two rebalances (la_moves.hip) ----------------------------------------------------------------------
// A topic of up to kMovesLdsMaxPartitions partitions is joined in one workgroup's LDS (a 64 KiB table at the limit); larger
// topics go through a table in device memory.  Up to kMovesLdsMaxMembers members the gained / lost counts are 32-bit LDS bins
// beside the table (2 x 4096 counters = 32 KiB: 96 KiB of the 160 KiB a gfx950 workgroup may take), beyond it global atomics.
constexpr int64_t kMovesLdsMaxPartitions = 4096;
constexpr int32_t kMovesLdsMaxMembers = 4096;
constexpr int32_t kMovesMaxMembers = (1 << 30) - 1;     // a slot keeps owner + 2 in 31 bits next to its matched mark
constexpr int32_t kMovesNoPrevious = -2;                // LA_MOVES_NO_PREVIOUS (lagassign.h): prev_owner of an added entry

struct MovesScratch {           // of one shard, grown lazily: never the assign scratch (results kept on the device stay valid)
    void* table = nullptr;      // the global form's hash table
    size_t table_cap = 0;
    StagedList list;            // its topic list
};

struct MovesCall {              // la_moves_args (lagassign.h), validated
    int32_t n_topics, n_members, n_prev_members;
    int64_t n_partitions, max_partitions_per_topic;
    const int64_t* part_off;
    const int32_t *out_partition, *out_member_rank, *prev_partition, *prev_member_rank;
    const int32_t* map;         // null: identity
    int32_t* prev_owner;        // outputs, each may be null
    int64_t *topic_moved, *member_gained, *member_lost, *moved;
};

// Zeroes the outputs on `stream`, then at most one launch (hint within kMovesLdsMaxPartitions) or three (LDS form for the
// small topics, insert and lookup of the global form for the others, found from h_part_off).  hipErrorOutOfMemory when the
// table cannot be had.  Sets kStatusMoves / kStatusShape / kStatusInternal.
hipError_t assignment_moves_launch(MovesScratch& s, const MovesCall& c, const int64_t* h_part_off, uint32_t* status,
                                   hipStream_t stream);
void moves_scratch_release(MovesScratch& s);

// The same question when the two assignments have a layout each (la_moves_layouts.hip; la_moves_args with d_prev_part_off).
struct MovesLayoutsCall {
    MovesCall c;                    // as above; part_off / n_topics / n_partitions are TODAY's layout
    int32_t n_prev_topics;
    int64_t n_prev_partitions;      // prev_partition / prev_member_rank hold this many entries
    const int64_t* prev_part_off;   // [n_prev_topics + 1]
    const int32_t* prev_topic;      // [n_topics] today's topic -> its topic of the previous layout, -1: new; null: identity
    int64_t *topic_added, *topic_removed, *added, *removed;      // outputs, each may be null
};

// Zeroes the outputs on `stream`, then at most one launch (hint within kMovesLdsMaxPartitions) or four (LDS form, and insert,
// lookup and sweep of the global form for the (today, previous) pairs with a side over the limit, found from the host arrays,
// which the caller has validated).  The table is `s.table`, as above.  Sets kStatusMoves / kStatusShape / kStatusInternal.
hipError_t assignment_moves_layouts_launch(MovesScratch& s, const MovesLayoutsCall& c, const int64_t* h_part_off,
                                           const int64_t* h_prev_part_off, const int32_t* h_prev_topic, uint32_t* status,
                                           hipStream_t stream);

// ---- certify an assignment (la_verify.hip) ---------------------------------------------------------------------------------
// One workgroup verifies a topic in LDS: the id join (la_join.h), the topic's lags, its consumers' ranks and one slot per
// (round, consumer) -- 136 KiB at the limit of both, within the 160 KiB a gfx950 workgroup may take.  Topics beyond that go,
// with LA_FLAG_VERIFY_LARGE, through the same tables in device memory (the global form: all large topics of a call side by side
// in kVerifyGlobalLaunches launches ordered by their boundaries), found on the host from h_part_off / h_cons_off.
constexpr int64_t kVerifyMaxPartitions = 4096;
constexpr int64_t kVerifyMaxConsumers = 4096;
constexpr int64_t kVerifyGlobalMaxPartitions = (1 << 30) - 2;      // the join's payload (an index + 2) keeps bit 63 for the mark
constexpr int kVerifyGlobalLaunches = 6;      // insert | lookup | order + chunk sums | chunk scan | apply | rounds + left out
constexpr int kVerifyMaxLaunches = 1 + kVerifyGlobalLaunches;      // what la_last_launches reports at most (lagassign.h)
constexpr uint32_t kVerdictIds = 1u, kVerdictOrder = 2u, kVerdictOwner = 4u, kVerdictGreedy = 8u, kVerdictTotals = 16u,
                   kVerdictUnchecked = 32u;      // LA_VERDICT_* of lagassign.h

struct VerifyScratch {          // of one shard, grown lazily: never the assign scratch (results kept on the device stay valid)
    void* work = nullptr;       // the global form's tables, one allocation carved into regions
    size_t work_cap = 0;
    StagedList list;            // its topic list
};

struct VerifyCall {             // la_device_batch (lagassign.h) as la_verify_assignment_device reads it, validated
    int32_t n_topics, reset_latest;
    int64_t n_partitions, n_consumers, max_partitions_per_topic, max_consumers_per_topic;
    const int64_t *part_off, *cons_off;
    const int32_t* pid;
    const int64_t *begin, *end, *committed, *lag;      // lag non-null: precomputed lags, offsets ignored; begin may be null
    const int32_t* cons_rank;
    const int32_t *out_pid, *out_rank;                 // the results under test
    const int64_t* out_total;                          // null: the totals are not checked
    int32_t* verdict;           // [T] or null
    int64_t* summary;           // [4] or null
};

// Initialises the summary on `stream`, then at most ONE launch.  Sets kStatusShape / kStatusInternal.
// With `large` (LA_FLAG_VERIFY_LARGE; h_part_off / h_cons_off validated by the caller: ascending inside [0, N] / [0, K]) the
// topics over the limit are listed from the host offsets and verified by the global form in front of that launch: at most
// kVerifyGlobalLaunches more, whatever their number and size; hipErrorOutOfMemory, with nothing enqueued, when its tables
// cannot be had.  Without a large topic the flagged call enqueues what the unflagged one does and touches no scratch.
hipError_t verify_assignment_launch(VerifyScratch* large, const VerifyCall& c, const int64_t* h_part_off,
                                    const int64_t* h_cons_off, uint32_t* status, hipStream_t stream);
void verify_scratch_release(VerifyScratch& s);

// ---- sticky ties: the previous owner decides among partitions of equal lag (la_sticky.hip) ------------------------------------
// One workgroup re-matches a topic in LDS, up to kVerifyMaxPartitions partitions as the verify call: the id join, the topic's
// lags, both rank arrays and two arrays of sort keys -- 136 KiB at the limit.  A larger topic is passed through, or, with
// LA_FLAG_STICKY_LARGE, re-matched by the global form below.
struct StickyCall {             // la_device_batch + la_sticky_args (lagassign.h) as la_sticky_ties_device reads them, validated
    int32_t n_topics, reset_latest;
    int64_t n_partitions, max_partitions_per_topic;
    const int64_t* part_off;
    const int32_t* pid;
    const int64_t *begin, *end, *committed, *lag;      // lag non-null: precomputed lags, offsets ignored; begin may be null
    const int32_t *out_pid, *out_rank;                 // the assign call's results
    const int32_t* prev_owner;
    int32_t* sticky;            // [N]
    int64_t *topic_kept, *topic_saved;                 // [T] or null
    int64_t* summary;           // [4] or null
};

// ---- sticky ties of topics beyond the LDS limit (la_sticky_large.hip, LA_FLAG_STICKY_LARGE) -------------------------------------
// The global form: all topics of a call with more than kVerifyMaxPartitions partitions side by side, the phases of the LDS kernel
// as launches over tables in device memory, the (run, member) ranks from the radix sort of la_radix.h.
constexpr int64_t kStickyGlobalMaxPartitions = kVerifyGlobalMaxPartitions;      // the join's payload, as in verify
// The sort takes two elements per partition and 2^31 - 1 elements: the large topics of ONE call hold at most this many partitions
// together (beyond it: hipErrorOutOfMemory, nothing enqueued -- the working memory would be ~100 GiB)
constexpr int64_t kStickyGlobalMaxTotal = (1 << 30) - 1;
// insert | lookup | run heads: chunk maxima | their scan | run starts + sort keys  (5)
// the sort's plan + 8 digit passes: 4 member digits, 4 run-start digits; a pass is ONE launch below 2^30 sort elements, else 4  (1 + 8 x 4)
// match | leftovers: chunk sums | their scan | leftover ranks | emit  (5)
constexpr int kStickyOwnLaunches = 10;
constexpr int kStickyGlobalLaunches = kStickyOwnLaunches + 1 + 8 * 4;      // 43; 19 while a call's large topics stay below 2^29 partitions
constexpr int kStickyMaxLaunches = 1 + kStickyGlobalLaunches;             // what la_last_launches reports at most (lagassign.h)
constexpr uint32_t kStickyBigBad = 1u, kStickyBigChanged = 2u;            // StickyWork::ctr[4 j + 2]

struct StickyBig {              // one topic of the global form; every offset and size is the HOST's, inside [0, N]
    int64_t p0, np;             // its segment of the batch
    int64_t q0;                 // its first position in the concatenated list of all large topics' positions
    int64_t table0;             // its table region, in slots
    int64_t step0;              // its first workgroup step (kStickyStep positions each), numbered through the topics
    int32_t topic, bits;        // the table region has 1 << bits slots
};

struct StickyWork {             // the global form's device memory, as the kernels see it (every pointer a kernel argument)
    uint64_t* table;
    int64_t* lag;               // [L] the lag at every position of the concatenated list
    unsigned long long* ctr;    // [4 n_big] kept before | kept after | kStickyBig* bits | unused, of every large topic
    unsigned long long* tot;    // [2] partitions not placed | positions not filled, over the whole list
    uint32_t *placed, *src_of, *hole_rank, *loose;      // [L] each
    uint32_t *cmax, *csum_loose, *csum_hole;            // [n_steps] each: one word per chunk (= step) of the two-level scans
    const StickyBig* big;       // ascending in topic
    int32_t n_big;
    int64_t n_pos, n_steps;     // L; workgroup steps
};

struct StickyScratch {          // of one shard, grown lazily: never the assign scratch (results kept on the device stay valid)
    void* work = nullptr;       // tables, per-position arrays and the sort's buffers, one allocation carved into regions
    size_t work_cap = 0;
    StagedList list;            // its topic list
    // what sticky_large_reserve found for the call it was made for (host arithmetic only)
    int64_t n_big = 0, n_pos = 0, n_steps = 0;
    size_t n_table = 0;
};

// Lists the topics of more than kVerifyMaxPartitions (and at most kStickyGlobalMaxPartitions) partitions from the host's offsets
// (validated by the caller: ascending inside [0, N]) into s.list and grows s.work for them.  Enqueues nothing; s.n_big == 0
// afterwards: the batch holds no such topic and nothing was touched.  hipErrorOutOfMemory when the memory cannot be had.
hipError_t sticky_large_reserve(StickyScratch& s, const StickyCall& c, const int64_t* h_part_off);
// The global form behind a reserve for the same call: at most kStickyGlobalLaunches launches.  *out: what the LDS kernel, which
// runs last, needs to record these topics' counts.
hipError_t sticky_large_enqueue(StickyScratch& s, const StickyCall& c, uint32_t* status, hipStream_t stream, StickyWork* out);
void sticky_scratch_release(StickyScratch& s);

// Zeroes the summary on `stream`, then at most ONE launch.  Sets kStatusSticky / kStatusShape / kStatusInternal.
// With `large` (LA_FLAG_STICKY_LARGE; h_part_off validated by the caller) the topics over the limit are re-matched by the global
// form in front of that launch: at most kStickyGlobalLaunches more, whatever their number and size; `reserved`: the caller has
// called sticky_large_reserve for this call already.  Without a large topic the flagged call enqueues what the unflagged one
// does and touches no scratch.
hipError_t sticky_ties_launch(const StickyCall& c, uint32_t* status, hipStream_t stream, StickyScratch* large = nullptr,
                              const int64_t* h_part_off = nullptr, bool reserved = false);

}  // namespace la
