/*
 * lagassign.h -- C ABI of the MI355X-native lag-based partition assignor.
 *
 * This is the drop-in boundary: the Java host (a ConsumerPartitionAssignor with the
 * same configure()/name()/assign() surface as the reference) does everything that is
 * string- or container-shaped and calls these functions through a thin JNI shim
 * (see INTEGRATION.md).  Everything below is plain pointers and sizes.
 *
 * "Main.java:N" =
 *   reference src/main/java/com/github/grantneale/kafka/LagBasedPartitionAssignor.java:N
 *
 * What each entry point replaces:
 *   la_compute_lag          static long computePartitionLag(...)            Main.java:376-404
 *   la_assign_batch         readTopicPartitionLags' per-partition lag call  Main.java:344-356
 *                           + the per-topic loop of assign(Map,Map)         Main.java:177-184
 *                           + assignTopic (sort + greedy + update)          Main.java:204-266
 *   la_assign_batch_sparse  the same with beginning offsets only where they are read   Main.java:384-396
 *   la_assign_batch_lags    static assign(Map,Map) on precomputed lags      Main.java:166-188
 *   la_assign_batch_device  the same two, on buffers already resident in HBM
 *   la_group_by_member      building every member's List<TopicPartition>      Main.java:171-174, :264
 *   la_assign_batch_grouped la_assign_batch + la_group_last_by_member in one call: the body of
 *                           assign(Cluster, GroupSubscription) between the offset RPCs and the wrapping  Main.java:147-156
 *   la_assign_batch_cooperative  nothing in the reference, whose protocol is eager: the same body for a COOPERATIVE host --
 *                           the assignment, the owned lists joined against it and every member's adjusted list in one call
 *   la_create_multi         the per-topic loop, sharded over the GPUs of a node Main.java:177-184
 *   la_assign_batch_device_on  the same loop for a caller whose data already lives on every GPU
 *   la_plan_shards          (which topics of that loop each shard takes)
 *   la_allgather_results    nothing in the reference (it has one thread and one heap): the reassembly of the global
 *                           assignment on every GPU, one RCCL all-gather over xGMI
 *   la_pack_results_on, la_unpack_results_on, la_allgather_packed, la_wire_format_for
 *                           the same gather in 2 (or 4) bytes per assigned partition instead of 8
 *   la_member_loads_device  nothing in the reference: the cross-topic sum, per member, of what its per-topic debug summary
 *                           prints (Main.java:279-306) -- partitions and total lag every member ended up with
 *   la_assignment_moves_device  nothing in the reference (its assignor is eager: every rebalance deals all partitions out again):
 *                           how many partitions changed owner between two rebalances, and who gained or lost them
 *   la_verify_assignment_device  nothing in the reference: a certificate that a result IS what assignTopic (Main.java:204-266)
 *                           would have produced for these inputs, checked without running it again
 *   la_cooperative_adjust_device  nothing in the reference, whose protocol is eager: the assignment a COOPERATIVE assignor
 *                           returns -- every partition that changes hands between two live members withheld for this round
 *   la_sticky_ties_device   nothing in the reference, which orders partitions of equal lag by id: the same assignment with the
 *                           partitions of each run of equal lag re-matched to their previous owners
 *   LA_FLAG_STICKY_LARGE / LA_COOP_STICKY_LARGE  nothing in the reference: la_sticky_ties_device for topics of more than 4096
 *                           partitions too, re-matched through tables in device memory
 *   la_cooperative_round_sticky_device  nothing in the reference: la_cooperative_adjust_device, la_sticky_ties_device and
 *                           la_cooperative_round_device on the sticky order, chained by hand until now, in one call
 *   la_assign_batch_cooperative_sticky  nothing in the reference: la_assign_batch_cooperative with the round on the sticky order
 *   la_hint_next_call       nothing in the reference's arithmetic: what the marshalling loop of readTopicPartitionLags
 *                           (Main.java:344-356) knows for free -- the largest end offset and partition id it walked past
 *   la_last_phase_times     nothing: measurement hook (radix-sort phase against the HBM roofline)
 *   la_device_features, la_last_pipeline, la_last_launches   nothing: diagnostics (what the library found / did)
 *   la_wake                       nothing in the reference: the head start its RPC phase (Main.java:147) gives the device
 *
 * Data model (SoA; TopicPartitionLag, Main.java:431-455, flattened):
 *   topic t owns partitions [part_off[t], part_off[t+1]) of the per-partition arrays and
 *   consumers  [cons_off[t], cons_off[t+1]) of cons_rank.
 *
 *   cons_rank[k] is the subscribing member's rank under java.lang.String.compareTo over
 *   all memberIds (0 = smallest).  Within one topic's segment the ranks MUST be strictly
 *   ascending (sorted, de-duplicated); the host does this once per rebalance.  The
 *   device never sees strings: "lowest memberId" (Main.java:259) == "lowest rank".
 *
 * Results, per topic segment, in the order the reference appends them (Main.java:264):
 *   out_partition[i]    partition id of the i-th assignment (lag desc, id asc)
 *   out_member_rank[i]  rank of the member that received it (-1: topic has no consumers,
 *                       Main.java:211-213)
 *   out_total_lag[k]    final consumerTotalLags of consumer k of that topic
 *                       (Main.java:265, the value the debug summary prints, :283-291)
 *
 * Buffers (every entry point, host and device arrays alike; tests/test_buffer_contract_gpu.py holds the library to it):
 *   - an array needs only its element's alignment: a view that starts at any element of a larger buffer (one shard's
 *     slice, t[1:]) is as good as a fresh allocation;
 *   - results are written only inside [0, N) / [0, K) (member_off: [0, M]) of the arrays given for them -- the wide
 *     stores of the kernels never reach past the last element or before the first;
 *   - inputs (the const arrays, h_part_off / h_cons_off included, and the caller's own arrays of the in-place
 *     pipelines) are never written, not even as scratch.
 *
 * Arithmetic is Java's: 64-bit two's-complement wrap on subtract/add, signed compares.
 * Results are bit-identical to the reference for every input, including negative lags
 * and overflowing totals.
 *
 * Threading: a la_ctx is single-threaded for its CALLER (one per assignor instance, like
 * the reference's own non-thread-safe state, Main.java:89); inside a host-buffer call the
 * library runs one host thread per lane of every shard (threads of the context, parked between calls; since ABI 0.4.0 -- spawned and
 * joined per call before) and returns when they are done.  No global mutable state.
 * Errors: every function returns LA_OK or a negative code and never throws or aborts;
 * la_last_error() gives the text.  There is NO CPU fallback in this library: without a
 * usable gfx950 device la_create fails and the caller (the Java host) decides.
 */
#ifndef LAGASSIGN_H
#define LAGASSIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LA_OK        0
#define LA_EINVAL   (-1)  /* bad argument (NULL, negative size, unsorted cons_rank, ...) */
#define LA_ENOMEM   (-2)  /* host or device allocation failed                           */
#define LA_EHIP     (-3)  /* a HIP runtime call or kernel failed                        */
#define LA_ENODEV   (-4)  /* no usable gfx950 device                                    */
#define LA_ESHAPE   (-5)  /* a topic exceeds the shape hint given for a device batch    */

/* auto.offset.reset as the reference reads it (Main.java:391-396): "latest"
 * (equalsIgnoreCase) -> LA_RESET_LATEST; EVERY other string, "none" included, behaves
 * as earliest. */
#define LA_RESET_LATEST   0
#define LA_RESET_EARLIEST 1

/* committed_off value meaning "no committed offset" (partitionMetadata == null,
 * Main.java:384).  Any negative value is treated the same; OffsetAndMetadata cannot
 * hold one. */
#define LA_NO_COMMITTED (-1)

/* la_device_batch.algo */
#define LA_ALGO_AUTO    0  /* round-structured greedy (default, fastest)                */
#define LA_ALGO_ROUNDS  1  /* force the round-structured greedy                         */
#define LA_ALGO_ARGMIN  2  /* literal per-partition wavefront argmin over the bins      */
#define LA_ALGO_ROUNDS_WIDE 3 /* rounds, but never the packed 64-bit record format (tile path);
                              * results are identical, this exists so tests can run both  */

/* la_device_batch.flags -- test hooks; results are identical with or without them */
#define LA_FLAG_INDEX64      1  /* 64-bit element indexing even when 32-bit offsets would do   */
#define LA_FLAG_DEFER_WIDE   2  /* never the single-launch form for small batches: tiles that  *
                                 * cannot use packed records go through the deferred-tile list */
#define LA_FLAG_RAGGED       4  /* topic shapes vary a lot: with h_part_off / h_cons_off given, let the  *
                                 * library group tile-sized topics by shape (one launch per class over  *
                                 * a topic list) instead of running all of them at the largest shape.   *
                                 * la_assign_batch decides this itself from the offsets.                */
#define LA_FLAG_SHAPE_CLASSES 8 /* with LA_FLAG_RAGGED: always one launch per non-empty shape class,     *
                                 * whatever the cost estimate says (test hook)                          */
#define LA_FLAG_PROFILE      16 /* measurement hook: HIP events around the phases of the first large-path  *
                                 * topic of this call (keys, radix-sort passes, greedy); la_last_phase_times *
                                 * reads them.  Device entry point only.                                  */
#define LA_FLAG_NO_SAMPLE_SORT 32 /* large path: every greedy round sorts its consumer bins with the full   *
                                 * bitonic network instead of the sample sort (test hook)                 */
#define LA_FLAG_SAMPLE_TIGHT 64 /* large path: the sample sort gives a round up (falls back to the full network)  *
                                 * above 6 bins per bucket instead of 96, so both kinds of round interleave  *
                                 * in one topic (test hook)                                                */

#define LA_FLAG_SORT_MULTIKERNEL 128 /* large path: every radix pass as four kernels (tile counts, two scans, scatter)   *
                                 * instead of the single-kernel pass with decoupled look-back (test hook / A-B)         */

#define LA_FLAG_NO_RUN_MERGE 256 /* large path: greedy rounds whose bins form a few ascending runs sort them like any other   *
                                 * round instead of merging the runs (test hook / A-B)                                  */

#define LA_FLAG_NO_MOVED_SORT 2048 /* large path: greedy rounds in which few bins change places sort all of them like any other    *
                                  * round instead of only the bins that move (test hook / A-B)                            */

#define LA_FLAG_BOUNDS      1024 /* max_lag_hint and max_partition_id_hint below are valid: the caller guarantees 0 <= lag <=          *
                                 * max_lag_hint for every lag the batch produces (the largest end offset will do: a lag never exceeds    *
                                 * it) and 0 <= partition id <= max_partition_id_hint.  When the bounds PROVE that every tile's records  *
                                 * pack into 64 bits, the tile path drops its second launch (the wide-record kernel over the list of     *
                                 * deferred tiles, empty in that case): one launch per batch instead of two.  On the large path (since   *
                                 * round 6) the radix passes over digits the bounds rule out -- key digits above the largest lag's bits, *
                                 * id digits above the largest id's -- are not launched.  A partition that violates the bounds is        *
                                 * reported by la_sync as LA_EINVAL -- never a silently different result.                                */
#define LA_FLAG_WIRE_OUT    4096 /* d_out_wire / wire_elem_bytes / wire_id_bits below are valid (since ABI 0.4.0): the results leave the kernels     *
                                 * in the narrow wire format of the multi-GPU all-gather (la_wire_format_for, below) -- one element of 2 or 4 bytes  *
                                 * per assigned partition, ((member rank + 1) << id_bits) | partition id, in assignment order -- INSTEAD of the two   *
                                 * int32 arrays (d_out_partition / d_out_member_rank are not written and may be NULL): what la_pack_results_on        *
                                 * would produce from them, without the 8 B written and read again per partition.  For the batches the gather is     *
                                 * for: every topic tile-sized (shape hint within 1024 x 64, no LA_FLAG_RAGGED), LA_FLAG_BOUNDS proving that every    *
                                 * tile packs, fewer than 2^29 partitions; anything else is LA_EINVAL (run the batch without the flag and pack).     *
                                 * A pair that does not fit the format is reported by la_sync as LA_EINVAL.  d_out_total_lag is written as usual.     */
#define LA_FLAG_VERIFY_LARGE 8192 /* la_verify_assignment_device[_on] only (every other entry ignores it): topics of more than 4096 partitions or  *
                                  * consumers are found from h_part_off / h_cons_off (then required) and verified through tables in device memory  *
                                  * instead of reading LA_VERDICT_UNCHECKED -- see that call.  It reads host memory and may allocate: not capturable */
#define LA_FLAG_STICKY_LARGE 16384 /* la_sticky_ties_device and la_cooperative_round_sticky_device only      (every other entry ignores it): topics *
                                   * of more than 4096 partitions are found from h_part_off (then required) and re-matched through tables in device *
                                   * memory instead of being passed through -- see la_sticky_ties_device.  It reads host memory and may allocate:    *
                                   * not capturable                                                                                              */
#define LA_FLAG_PINNED_LARGE 32768 /* la_assign_pinned_device only (every other entry ignores it): topics of more than 4096 partitions are found   *
                                   * from h_part_off / h_cons_off (then required) and assigned through device memory instead of being skipped     *
                                   * with LA_ESHAPE -- see that call.  It reads host memory and may allocate: not capturable                       */
#define LA_FLAG_SERIAL_LARGE 512 /* large path: the batch's large topics one after another (round 3's form) instead of side by   *
                                 * side in shared launches (test hook / A-B)                                            */

typedef struct la_ctx la_ctx;

/* la_create / la_create_multi flags */
#define LA_CREATE_LANES_MASK   0xFu   /* low 4 bits: lanes (streams + host threads) per shard for the chunked    *
                                       * H2D / kernels / D2H overlap of the host-buffer calls; 0 = automatic      *
                                       * (3 for one or two shards, 2 beyond; environment LA_LANES overrides)      */
#define LA_CREATE_SPLIT_ALWAYS 0x10u  /* test hook: shard and chunk every batch, however small (normally a batch  *
                                       * under 65 536 partitions per extra shard stays on fewer devices and a     *
                                       * shard under 2 chunks of 524 288 partitions is one chunk, no threads)     */

/* Number of HIP devices visible to the process (>= 0), or a negative code. */
int la_device_count(void);

/* Creates a context on HIP device `device_id` (streams, scratch, kernels). */
int la_create(la_ctx **out, int device_id, unsigned flags);

/* Creates a context over several devices of one node: shard i of every host-buffer call runs on
 * device_ids[i].  This is the multi-GPU form of the per-topic loop of assign(Map,Map) (Main.java:177-184):
 * assignTopic touches only its own topic's bins (Main.java:216-225), so a batch is split into n_devices
 * contiguous topic ranges balanced by partition count (la_plan_shards), every range runs the whole hot path on
 * its device concurrently (one host thread per lane), and each shard's results are copied straight to their
 * offset in the caller's output arrays -- that IS the reassembly of the global assignment; no device ever needs
 * another device's topics.  n_devices = 0 (device_ids NULL) = every device of the node.  An id may appear more than
 * once (several logical shards on one GPU; how the tests exercise the split on a one-GPU box).
 * The device-buffer entry points without a shard argument (la_assign_batch_device, la_group_by_member_device, la_sync,
 * la_stream) use the first device; their *_on forms take any shard.  la_compute_lag and la_group_by_member split large
 * inputs over the shards like the assign calls do. */
int la_create_multi(la_ctx **out, int n_devices, const int *device_ids, unsigned flags);
void la_destroy(la_ctx *ctx);

/* Shards of the context, and the HIP device of shard i. */
int la_shard_count(const la_ctx *ctx);
int la_shard_device(const la_ctx *ctx, int shard);

/* What the library found out about shard i's device when the context was created (bit mask; measurement / diagnostics):
 *   LA_FEATURE_ATOMIC_RANK  the radix sort of the large path ranks equal digits with returning LDS atomics -- the device
 *                           passed the lane-order check that form relies on (otherwise: wave-match ranking, same results). */
#define LA_FEATURE_ATOMIC_RANK 1
int la_device_features(const la_ctx *ctx, int shard);

/* The planner the library uses for shards and for the chunks inside a shard: contiguous topic ranges
 * [bounds[r], bounds[r+1]) for r in [0, n_shards), balanced by partition count (bounds[r] = first topic boundary
 * at or after r/n_shards of the partitions).  Every topic lands in exactly one range; ranges may be empty.
 * bounds has n_shards + 1 entries.  Pure host code: needs no context and no device, so a multi-process
 * launcher (one process per GPU) can shard a batch exactly as a multi-device context would. */
int la_plan_shards(int32_t n_topics, const int64_t *part_off, int32_t n_shards, int32_t *bounds);

/* The split the last la_assign_batch / la_assign_batch_lags call used: returns the number of shards S and writes
 * min(S + 1, capacity) bounds (bounds may be NULL). */
int la_last_shard_bounds(const la_ctx *ctx, int32_t *bounds, int32_t capacity);

/* How the last la_assign_batch / la_assign_batch_lags call moved its data (diagnostics, tests):
 *   LA_PIPELINE_ZERO_COPY the call a real rebalance is: kernels read and write host memory in place, no copy, no stream wait
 *   LA_PIPELINE_ONE_COPY  a small batch: one H2D and one D2H of a staging buffer
 *   LA_PIPELINE_LANES     chunks over the shard's lanes, one host thread of the context per lane (pageable caller arrays:
 *                         their copies block the issuing thread)
 *   LA_PIPELINE_STREAMS   every array of the call is pinned but not device-mapped (hipHostRegister without the mapped flag;
 *                         LA_NO_MAPPED_PIPELINE=1): no threads; all H2D copies in order on one stream, kernels on a second, D2H
 *                         copies on a third, chained per chunk by events -- the input link stays busy from the first byte to the last
 *   LA_PIPELINE_MAPPED    every array is pinned and mapped (la_host_alloc): the kernels work on the caller's arrays in place */
#define LA_PIPELINE_ONE_COPY 0
#define LA_PIPELINE_LANES    1
#define LA_PIPELINE_STREAMS  2
#define LA_PIPELINE_MAPPED    4   /* every array of the call is pinned AND device-mapped (la_host_alloc): no copies and no chunks --
                                   * the kernels read the caller's arrays in place over PCIe (each input byte is touched once,
                                   * `begin` only where there is no committed offset) and write the results straight into them */
#define LA_PIPELINE_ZERO_COPY 3   /* calls whose arrays fit one staging buffer (up to 12 MB, ~340 000 partitions; for pinned
                                   * caller arrays less, see LA_PIPELINE_MAPPED; environment LA_ZERO_COPY_BYTES overrides,
                                   * 0 = never): no copy at all -- the inputs are packed into coherent, device-mapped host
                                   * memory, the kernels read them there and write totals / results / member lists into it;
                                   * the call's last launch stores the status where the calling thread is spinning */
int la_last_pipeline(const la_ctx *ctx);

/* Pinned host memory for the arrays handed to the host-buffer calls (a JNI shim wraps it in a direct ByteBuffer
 * with NewDirectByteBuffer): the copies then run as plain DMA, without the runtime staging or pinning pageable
 * pages per call.  Optional -- every entry point takes pageable memory too.  NULL on failure.
 * The memory is also device-mapped: its address is valid on the context's devices, so a caller without device memory of its
 * own may hand it to a device entry point as a d_* array (examples/assign_example.c does, for three partitions).  Every access
 * then crosses PCIe, and the counting outputs of such a call take 64-bit atomics over the link, which needs a platform with
 * PCIe atomics -- a convenience for small calls and tests, not a way to run a batch. */
void *la_host_alloc(la_ctx *ctx, size_t bytes);
void la_host_free(la_ctx *ctx, void *p);
/* Text of the last error on this context ("" if none).  ctx may be NULL: returns the
 * text of the last la_create failure on the calling thread. */
const char *la_last_error(const la_ctx *ctx);
/* ABI version: major*10000 + minor*100 + patch.  LA_VERSION is the header's, la_version() the loaded library's: a shim
 * (JNI, ctypes) compares the two before it binds entry points that older libraries lack.
 *   0.2.1 (201)  rounds 2-3: multi-device contexts, grouped calls, *_on device entry points, la_allgather_results
 *   0.3.0 (300)  round 4: la_wire_format_for / la_pack_results_on / la_unpack_results_on / la_allgather_packed (narrow wire
 *                format of the all-gather), la_assign_batch_sparse / la_assign_batch_grouped_sparse (begin offsets only
 *                where there is no committed offset); every entry point restores the caller's current HIP device
 *   0.4.0 (400)  round 5: la_hint_next_call (the caller's bounds on lags and ids reach the host-buffer calls: one tile launch
 *                instead of two), la_last_launches, la_last_phase_times_sized
 *   0.5.0 (500)  round 6: la_wake (the device's queues woken while the host still fetches offsets); LA_FLAG values unchanged
 *                later, WITHOUT a bump: la_member_loads_device / la_member_loads_device_on (per-member roll-up of an assignment);
 *                la_assignment_moves_device / la_assignment_moves_device_on (who moved between two rebalances);
 *                la_verify_assignment_device / la_verify_assignment_device_on (certify an assignment);
 *                la_cooperative_adjust_device (the cooperative form of a rebalance);
 *                la_cooperative_round_device / la_cooperative_round (that form and every member's list of it in one call);
 *                la_assign_batch_cooperative (a cooperative rebalance from host buffers in one call);
 *                la_sticky_ties_device (among partitions of equal lag the previous owner keeps its own);
 *                la_cooperative_round_sticky_device (the cooperative round on the sticky order in one call);
 *                la_assign_batch_cooperative_sticky (a cooperative rebalance on the sticky order from host buffers);
 *                LA_FLAG_STICKY_LARGE, LA_COOP_STICKY_LARGE (sticky ties for topics of any size);
 *                LA_FLAG_PINNED_LARGE, LA_COOP_PINNED_LARGE, LA_PINNED_LARGE_MAX_PARTITIONS, LA_PINNED_LARGE_LAUNCHES (the
 *                pinned assignment for topics of any size);
 *                a shim detects them by symbol lookup (dlsym / getattr) instead of by version */
#define LA_VERSION 500
int la_version(void);

/* computePartitionLag over n partitions (host buffers).  begin_off may be NULL when
 * reset_mode == LA_RESET_LATEST.  Main.java:376-404.
 * Reuses the device scratch the last assign call's results live in: after it (and after la_group_by_member)
 * la_group_last_by_member returns LA_EINVAL until the next la_assign_batch / la_assign_batch_lags. */
int la_compute_lag(la_ctx *ctx, int64_t n,
                   const int64_t *begin_off, const int64_t *end_off,
                   const int64_t *committed_off, int32_t reset_mode,
                   int64_t *out_lag);

/* What the caller's marshalling loop knows about the NEXT host-buffer assign call on this context (la_assign_batch, _sparse,
 * _lags, _grouped, _grouped_sparse) -- the reference's loop (Main.java:344-356) walks every partition's offsets anyway, so the
 * largest end offset and the largest partition id cost it two compares per partition.  One-shot: the hints apply to the next
 * such call and are forgotten when it returns, whatever it returns (a call without la_hint_next_call before it has none).
 *   LA_HINT_BOUNDS  the caller guarantees 0 <= lag <= max_lag for every lag the call computes (the largest end offset will do
 *                   when no begin / end / committed offset of the batch is negative, which Kafka guarantees: a lag never
 *                   exceeds its end offset) and 0 <= partition id <= max_partition_id.  The library hands them to its kernels
 *                   as LA_FLAG_BOUNDS (below): where they prove that every tile's records pack into 64 bits, the tile path
 *                   is ONE launch per chunk instead of two.  A partition that violates the bounds makes the call fail with
 *                   LA_EINVAL -- never a silently different result; a caller that is not sure gives no hint.
 * struct_size = sizeof(la_call_hints) of the caller's header (the struct may grow).  hints == NULL clears pending hints. */
#define LA_HINT_BOUNDS 1
typedef struct la_call_hints {
    int32_t struct_size;
    int32_t flags;               /* LA_HINT_* */
    int64_t max_lag;             /* LA_HINT_BOUNDS */
    int64_t max_partition_id;    /* LA_HINT_BOUNDS */
} la_call_hints;
int la_hint_next_call(la_ctx *ctx, const la_call_hints *hints);

/* Warm the path of the assign call that is about to come (since ABI 0.5.0).  What it is for: Kafka calls assign() on the group
 * leader once per rebalance -- minutes apart -- and the reference's assign() spends its first milliseconds on broker round trips
 * (readTopicPartitionLags, Main.java:147, :317-365) before it has a single offset to hand over.  After a second of idle a small
 * call costs several times what it costs back to back (tools/cold_c.c at the C ABI on MI355X, profiles/r06_p_cold_c.txt: a
 * 100-partition la_assign_batch_grouped 23 us back to back, 36 us after 50 ms of idle, 85 us after 1 s; 2 000 partitions 32 / 46 /
 * 101 us): the device's queue, the link, the mapped pages, the runtime's code in the host's caches are all cold.  la_wake runs
 * ONE one-partition rebalance through the real small-call path and waits for it (it pays the cold call itself: ~95 us), and
 * launches one empty kernel on every other stream of the context; the assign call that follows within ~20 ms then takes 34 us
 * (100 partitions) / 48 us (2 000) / 73 us (10 000: 127 cold); 200 ms later most of the effect is gone, and calls of hundreds of
 * thousands of partitions gain nothing.  A host calls it when it ENTERS assign(), before its RPCs.  Optional, never needed for
 * correctness.  A pending
 * la_hint_next_call and the diagnostics of the last real call (la_last_pipeline, la_last_launches) survive it; results kept on
 * the device for la_group_last_by_member do not (LA_EINVAL until the next assign call, as after la_compute_lag). */
int la_wake(la_ctx *ctx);

/* Kernel launches the last host-buffer call (or the last la_assign_batch_device[_on] call) on this context enqueued -- every
 * kernel of the library counts, copies and memsets do not.  Diagnostics / tests: a batch of tile-sized topics whose hints prove
 * that every tile packs reports 1 per chunk (+ 1 per chunk for the consumer-rank check of the copying pipelines).  The counter
 * behind it is process-wide: exact while no other context of the process is inside a call. */
int64_t la_last_launches(const la_ctx *ctx);

/* One rebalance: lag from offsets, then sort + greedy per topic.  All pointers are
 * caller-owned host memory, valid for the duration of the call.  N = part_off[T],
 * K = cons_off[T].  out_total_lag may be NULL. */
int la_assign_batch(la_ctx *ctx, int32_t n_topics,
                    const int64_t *part_off,       /* [T+1]                              */
                    const int32_t *partition_id,   /* [N]                                */
                    const int64_t *begin_off,      /* [N]  NULL allowed iff LATEST       */
                    const int64_t *end_off,        /* [N]                                */
                    const int64_t *committed_off,  /* [N]  <0 == none                    */
                    int32_t reset_mode,
                    const int64_t *cons_off,       /* [T+1]                              */
                    const int32_t *cons_rank,      /* [K]  ascending within each topic   */
                    int32_t *out_partition,        /* [N]  (both NULL: results stay on   */
                    int32_t *out_member_rank,      /* [N]   the device, see la_group_last_by_member) */
                    int64_t *out_total_lag);       /* [K]  or NULL                       */

/* la_assign_batch with `begin` handed over SPARSELY.  computePartitionLag reads the beginning offset only where a partition
 * has no committed offset and auto.offset.reset is not "latest" (Main.java:384-396) -- typically ~1 % of a group's
 * partitions -- while a dense begin_off array is 8 of the 28 input bytes per partition that cross PCIe, the link that bounds
 * every host-buffer call.  Here the caller lists only those partitions:
 *   none_index[j]  position (index into the per-partition arrays, 0 .. N-1) of a partition without a committed offset,
 *                  ASCENDING (the marshaller meets them in order: GpuLagBasedPartitionAssignor.java, `md == null`)
 *   none_begin[j]  its beginning offset
 * A partition with committed_off < 0 that is NOT listed has begin 0 -- the reference's getOrDefault(tp, 0L) for a missing
 * beginning offset (Main.java:350-351).  Entries whose partition HAS a committed offset are harmless (never read).
 * In LA_RESET_LATEST mode the list is ignored (may be NULL).  A list that is not ascending or leaves [0, N): LA_EINVAL.
 * Results are those of la_assign_batch on the equivalent dense array, bit for bit. */
int la_assign_batch_sparse(la_ctx *ctx, int32_t n_topics,
                           const int64_t *part_off, const int32_t *partition_id,
                           const int64_t *end_off, const int64_t *committed_off, int32_t reset_mode,
                           int64_t n_none, const int64_t *none_index, const int64_t *none_begin,
                           const int64_t *cons_off, const int32_t *cons_rank,
                           int32_t *out_partition, int32_t *out_member_rank, int64_t *out_total_lag);

/* Same, on precomputed lags: the static assign(Map,Map) seam the reference's own tests
 * use (Test.java:127-128).  lag[] may hold any int64, negatives included. */
int la_assign_batch_lags(la_ctx *ctx, int32_t n_topics,
                         const int64_t *part_off, const int32_t *partition_id,
                         const int64_t *lag,
                         const int64_t *cons_off, const int32_t *cons_rank,
                         int32_t *out_partition, int32_t *out_member_rank,
                         int64_t *out_total_lag);

/* A batch whose bulk arrays already live in device memory (HBM). */
typedef struct la_device_batch {
    int32_t n_topics;
    int32_t reset_mode;
    int32_t algo;                    /* LA_ALGO_*                                        */
    int32_t flags;                   /* LA_FLAG_*; 0 in normal use                       */
    int64_t n_partitions;            /* N                                                */
    int64_t n_consumers;             /* K                                                */
    /* Shape hint: upper bounds over the batch.  With a hint within one wave tile (1024
     * partitions x 64 consumers) and no LA_FLAG_RAGGED, a topic that exceeds it is reported
     * as LA_ESHAPE by la_sync(); nothing is written for it -- neither its partitions' results
     * nor its consumers' totals -- and the other topics of the batch are assigned as usual.
     * With a larger hint, or LA_FLAG_RAGGED, the library routes every topic by its real
     * shape (h_part_off / h_cons_off, below): a topic over the hint is assigned like any other. */
    int64_t max_partitions_per_topic;
    int64_t max_consumers_per_topic;
    /* device pointers */
    const int64_t *d_part_off;       /* [T+1]                                            */
    const int32_t *d_partition_id;   /* [N]                                              */
    const int64_t *d_begin_off;      /* [N] or NULL (LATEST only)                        */
    const int64_t *d_end_off;        /* [N] (ignored when d_lag != NULL)                 */
    const int64_t *d_committed_off;  /* [N] (ignored when d_lag != NULL)                 */
    const int64_t *d_lag;            /* [N] or NULL: precomputed lags instead of offsets */
    const int64_t *d_cons_off;       /* [T+1]                                            */
    const int32_t *d_cons_rank;      /* [K]                                              */
    int32_t *d_out_partition;        /* [N]  (not looked at when N == 0)                 */
    int32_t *d_out_member_rank;      /* [N]                                              */
    int64_t *d_out_total_lag;        /* [K] or NULL                                      */
    /* host copies of the two offset arrays; required only when the shape hint exceeds
     * what one wavefront tile holds (1024 partitions or 64 consumers per topic): the
     * library then looks at every topic's size on the host (a few ns per topic) and
     * sends it down the wave-tile path, the block path (one workgroup per topic, up to
     * 8192 partitions x 2048 consumers, all such topics side by side) or the large path
     * (device-wide radix sort + one greedy workgroup per topic, the batch's large topics side by side in
     * shared launches; beyond 8192 consumers the bins live in HBM and every greedy round is a device
     * sort: any consumer count, Main.java:240-263 has no bound).  Also read when LA_FLAG_RAGGED is set.
     * NULL otherwise -- or NULL anyway: the library then fetches the offsets itself, which
     * makes that call wait on `stream` (not asynchronous, not capturable).  Calls on one context are expected to be stream-ordered: the
     * per-call topic lists live in context-owned device memory. */
    const int64_t *h_part_off;
    const int64_t *h_cons_off;
    /* with LA_FLAG_BOUNDS (since ABI 0.3.0; ignored without the flag) */
    int64_t max_lag_hint;            /* upper bound of every lag of the batch, >= 0                */
    int64_t max_partition_id_hint;   /* upper bound of every partition id, >= 0                    */
    /* with LA_FLAG_WIRE_OUT (since ABI 0.4.0; ignored without the flag) */
    void   *d_out_wire;              /* [N] elements of wire_elem_bytes each, element-aligned      */
    int32_t wire_elem_bytes;         /* 2 or 4 (la_wire_format.elem_bytes)                         */
    int32_t wire_id_bits;            /* la_wire_format.id_bits                                     */
} la_device_batch;

/* Enqueues the whole batch on `stream` and returns without waiting.  `stream` is a
 * hipStream_t used exactly as given (NULL = HIP's default stream); la_stream() gives
 * the context's own stream.  Device-detected errors surface in la_sync.
 * A batch of tile-sized topics (shape hint within 1024 x 64, no LA_FLAG_RAGGED) is kernel
 * launches only once the context has seen one call of that size (scratch allocated), so
 * it may be captured in a HIP graph and replayed; eager launches cost about the same. */
int la_assign_batch_device(la_ctx *ctx, const la_device_batch *batch, void *stream);

/* Waits for `stream` and returns LA_OK or the first device-detected error. */
int la_sync(la_ctx *ctx, void *stream);

/* The device entry points on ANY shard of a multi-device context: a caller that keeps its data in HBM drives all the
 * node's GPUs from one context (la_assign_batch_device / la_sync / la_stream are shard 0's).  The batch's pointers must
 * belong to la_shard_device(ctx, shard); `stream` is a stream of that device (la_shard_stream gives the shard's own).
 * Shards are independent -- their calls may be enqueued back to back from one host thread and run concurrently, which
 * is the per-topic loop of assign(Map,Map) (Main.java:177-184) over several devices with the data already resident:
 * split the topics with la_plan_shards, give shard i the range [bounds[i], bounds[i+1]), sync every shard. */
void *la_shard_stream(la_ctx *ctx, int shard);
int la_assign_batch_device_on(la_ctx *ctx, int shard, const la_device_batch *batch, void *stream);
int la_sync_on(la_ctx *ctx, int shard, void *stream);

/* Phase times of the first large-path topic (one topic beyond the block path: device-wide radix sort, then the
 * one-workgroup greedy) of the last la_assign_batch_device call that carried LA_FLAG_PROFILE.  Measurement only:
 * it is how bench.py reports the radix-sort phase against the HBM roofline from inside one run.  Waits for that
 * topic's kernels.  LA_EINVAL when no such topic was profiled. */
typedef struct la_phase_times {
    int64_t n_partitions;
    int32_t id_passes;     /* active 8-bit passes over the partition-id digits (0 when ids arrive ascending)  */
    int32_t key_passes;    /* active passes over the lag-key digits; constant digits are skipped on the device */
    float keys_ms;         /* lag + keys + the 12 digit histograms, pass plan                                  */
    float sort_ms;         /* every active radix pass (+ the tie repair of a keys-first sort): until the order is final */
    float greedy_ms;       /* ids in assignment order + the greedy rounds                                      */
    int32_t keys_first;    /* 1: the sort skipped the id passes and put runs of equal lags in id order afterwards
                            * (large topics with shuffled ids and no frequent lag; since ABI 0.3.0)             */
    int32_t redone;        /* 1: a run of equal lags did not fit the repair and the sort was redone in full     */
} la_phase_times;
int la_last_phase_times(la_ctx *ctx, la_phase_times *out);
/* The same for a caller compiled against any version of this header: writes min(out_size, sizeof(la_phase_times)) bytes.
 * la_last_phase_times writes the whole struct of THIS header (40 bytes since ABI 0.3.0, 32 before): a shim built against 0.2.x
 * must check la_version() < 300 before it calls that one, or call this one with its own sizeof. */
int la_last_phase_times_sized(la_ctx *ctx, void *out, size_t out_size);

/* The context's own (non-blocking) hipStream_t, used by the host-buffer entry points. */
void *la_stream(la_ctx *ctx);

/* Assignment -> per-member lists: the wrap step of the reference (every member's list is created at
 * Main.java:171-174 and appended to at :264, topic by topic in the order the topics were given, inside a
 * topic in assignment order; Main.java:152-156 then wraps each list).  Input: the result arrays of an
 * assign call.  Output, with M = n_members (ranks 0..M-1):
 *   member_off[r] .. member_off[r+1]   member r's slice of the grouped arrays (member_off has M+1 entries);
 *                                      positions before member_off[0] hold the entries of topics that had no
 *                                      consumer (rank -1), which the reference leaves unassigned
 *   grouped_topic[j], grouped_partition[j]   topic index (into part_off) and partition id of the j-th entry,
 *                                      in exactly the order the reference's list for that member holds them
 * It is a stable device radix sort of the entry indices by member rank.  grouped_topic may be NULL.
 * Like la_compute_lag this call takes over the scratch of the last assign call: the results held for
 * la_group_last_by_member are gone afterwards. */
int la_group_by_member(la_ctx *ctx, int32_t n_topics, const int64_t *part_off,
                       const int32_t *out_partition, const int32_t *out_member_rank, int32_t n_members,
                       int64_t *member_off, int32_t *grouped_topic, int32_t *grouped_partition);

/* The same for the results the last successful la_assign_batch / la_assign_batch_lags call on this context left
 * on the device: nothing is uploaded again.  A caller that only wants the grouped form gives that call
 * out_partition = out_member_rank = NULL (both), which also skips their download: the assignment then crosses
 * PCIe once, as member_off + grouped_topic + grouped_partition.  LA_EINVAL when there is no such result (no
 * assign call yet, or another host-buffer call on this context since).  grouped_topic may be NULL.
 * (After a call on pinned, device-mapped arrays -- LA_PIPELINE_MAPPED -- that DID take the ungrouped results, "on the device"
 * means the caller's own result arrays, which the kernels wrote in place: leave them as they are until this call.) */
int la_group_last_by_member(la_ctx *ctx, int32_t n_members,
                            int64_t *member_off, int32_t *grouped_topic, int32_t *grouped_partition);

/* Both steps in one call -- what the reference's assign(Cluster, GroupSubscription) does between reading the offsets
 * and wrapping the lists (Main.java:147-156): la_assign_batch with the ungrouped result left on the device, then
 * la_group_last_by_member.  For the call a real rebalance is (its arrays fit the library's staging buffer: 12 MB) the lists
 * are built behind the assignment kernels on the same stream -- up to 1 024 entries inside the assignment kernel itself -- and
 * land in that buffer with the status and the totals: no copy, one wait.  Larger batches run the two steps one after the other.  The results stay
 * on the device as after la_assign_batch (la_group_last_by_member may be called again).  grouped_topic and out_total_lag
 * may be NULL. */
int la_assign_batch_grouped(la_ctx *ctx, int32_t n_topics, const int64_t *part_off, const int32_t *partition_id,
                            const int64_t *begin_off, const int64_t *end_off, const int64_t *committed_off,
                            int32_t reset_mode, const int64_t *cons_off, const int32_t *cons_rank, int32_t n_members,
                            int64_t *member_off, int32_t *grouped_topic, int32_t *grouped_partition,
                            int64_t *out_total_lag);

/* la_assign_batch_grouped with the sparse `begin` of la_assign_batch_sparse: what the Java host calls. */
int la_assign_batch_grouped_sparse(la_ctx *ctx, int32_t n_topics, const int64_t *part_off, const int32_t *partition_id,
                                   const int64_t *end_off, const int64_t *committed_off, int32_t reset_mode,
                                   int64_t n_none, const int64_t *none_index, const int64_t *none_begin,
                                   const int64_t *cons_off, const int32_t *cons_rank, int32_t n_members,
                                   int64_t *member_off, int32_t *grouped_topic, int32_t *grouped_partition,
                                   int64_t *out_total_lag);

/* Same on device buffers (N = n_partitions entries); enqueues on `stream` and returns. */
int la_group_by_member_device(la_ctx *ctx, int32_t n_topics, int64_t n_partitions,
                              const int64_t *d_part_off, const int32_t *d_out_partition,
                              const int32_t *d_out_member_rank, int32_t n_members,
                              int64_t *d_member_off, int32_t *d_grouped_topic, int32_t *d_grouped_partition,
                              void *stream);

/* The north star's single RCCL all-gather, in native code, for a caller that drives every GPU of the node from ONE process
 * (la_create_multi + la_assign_batch_device_on): every shard's result buffer to every shard's device.
 *   d_send[i]  `count` int32 on shard i's device (e.g. its [2, cap] result buffer: partition order | member rank)
 *   d_recv[i]  n_shards * count int32 on shard i's device; shard j's block lands at d_recv[i] + j * count
 * One ncclAllGather per shard inside one ncclGroupStart / ncclGroupEnd, enqueued on la_shard_stream(ctx, i) -- i.e. behind
 * whatever la_assign_batch_device_on enqueued there; la_sync_on waits for it.  ncclAllGather moves equal counts: pad the
 * shards to the largest (la_plan_shards balances them to within one topic).  The communicators are created on first use
 * (ncclCommInitAll over the context's devices) and live as long as the context.
 * librccl is loaded at run time, on first use (dlopen; a copy already in the process is preferred): LA_ENODEV when it is
 * not there.  RCCL wants one DISTINCT device per rank: LA_EINVAL for a context with several shards on one device.
 * (One process per GPU -- bench.py, torch.distributed -- calls RCCL through its own framework instead.) */
int la_allgather_results(la_ctx *ctx, int64_t count, const int32_t *const *d_send, int32_t *const *d_recv);

/* ---- the narrow wire format of that all-gather ------------------------------------------------------------------------
 * What the gather moves per assigned partition is a (partition id, member) pair in assignment order (Main.java:264): 8 B as
 * two int32 arrays, but 8 + 6 bits of information at the 100 000 x 256 x 32 target.  xGMI is the slow station of the
 * multi-GPU step (7 links x ~77 GB/s per direction against ~5 TB/s of HBM), so the gather's bytes are the step's time.
 * One wire element =
 *       ((member rank + 1) << id_bits) | partition id        (rank + 1 == 0: the topic had no consumer, Main.java:211-213)
 * as an unsigned integer of elem_bytes = 2, 4 or 8 bytes; the 8-byte form (id_bits = 32) carries ANY int32 pair.
 *   la_wire_format_for   the narrowest format for ids in [0, max_partition_id] and ranks in [-1, n_members); pass
 *                        max_partition_id < 0 when ids may be negative or are not known (-> the 8-byte form).  Pure host code.
 *   la_pack_results_on   n results of shard `shard` (device arrays, e.g. what la_assign_batch_device_on wrote) -> n wire
 *                        elements; enqueued on `stream`.  A pair that does not fit `fmt` is reported by la_sync_on as LA_EINVAL.
 *   la_unpack_results_on the reverse, on any shard's device (e.g. over the whole gathered buffer, padding included).
 *   la_allgather_packed  la_allgather_results for `count` elements of elem_bytes each.
 * Pointers 16-byte aligned take the 16-byte-access kernels; any alignment of elem_bytes works. */
typedef struct la_wire_format {
    int32_t elem_bytes;    /* 2, 4 or 8 */
    int32_t id_bits;       /* low bits of an element that hold the partition id (32 in the 8-byte form) */
} la_wire_format;
int la_wire_format_for(int64_t max_partition_id, int64_t n_members, la_wire_format *out);
int la_pack_results_on(la_ctx *ctx, int shard, int64_t n, const int32_t *d_out_partition,
                       const int32_t *d_out_member_rank, const la_wire_format *fmt, void *d_packed, void *stream);
int la_unpack_results_on(la_ctx *ctx, int shard, int64_t n, const void *d_packed, const la_wire_format *fmt,
                         int32_t *d_out_partition, int32_t *d_out_member_rank, void *stream);
int la_allgather_packed(la_ctx *ctx, int64_t count, int32_t elem_bytes, const void *const *d_send, void *const *d_recv);

/* la_group_by_member_device on shard `shard` (buffers on that shard's device). */
int la_group_by_member_device_on(la_ctx *ctx, int shard, int32_t n_topics, int64_t n_partitions,
                                 const int64_t *d_part_off, const int32_t *d_out_partition,
                                 const int32_t *d_out_member_rank, int32_t n_members,
                                 int64_t *d_member_off, int32_t *d_grouped_topic, int32_t *d_grouped_partition,
                                 void *stream);

/* Per-member roll-up of an assignment (nothing in the reference computes it; it is the cross-topic sum of what the
 * debug summary prints per topic, Main.java:283-291).  With M = n_members:
 *   d_member_partitions[r] = #{ i in [0,N) : d_out_member_rank[i] == r }                       r in [0, M)
 *   d_unassigned[0]        = #{ i in [0,N) : d_out_member_rank[i] == -1 }   (topics without consumers, Main.java:211-213)
 *   d_member_lag[r]        = sum of d_out_total_lag[k] over k in [0,K) with d_cons_rank[k] == r,
 *                            Java long arithmetic (64-bit two's-complement wrap)
 * Either half may be left out: d_out_member_rank == NULL (then d_member_partitions and d_unassigned must be NULL),
 * or d_cons_rank == NULL (then d_out_total_lag and d_member_lag must be NULL); both NULL is LA_EINVAL.  (The input pointer
 * decides, also when its size is 0: an empty half that is present still has its outputs zeroed.)
 * d_unassigned may be NULL.  Outputs are OVERWRITTEN (a member that received nothing reads 0).
 * Enqueues on `stream` and returns -- behind la_assign_batch_device on the same stream it reads that call's results, no sync in
 * between; a rank outside [-1, M) in d_out_member_rank or outside [0, M) in d_cons_rank is not counted, never written
 * through, and reported by la_sync as LA_EINVAL (what the other entries added to the outputs is then unspecified).
 * N == 0 / K == 0 are valid.  At most one kernel launch (la_last_launches) behind the memsets that zero the outputs; the call
 * needs no scratch, so the results kept for la_group_last_by_member stay valid.
 * Buffer contract as everywhere in this header (element alignment only, no write outside [0,M) / [0,1), inputs
 * never written). */
int la_member_loads_device(la_ctx *ctx, int64_t n_partitions, const int32_t *d_out_member_rank,
                           int64_t n_consumers, const int32_t *d_cons_rank, const int64_t *d_out_total_lag,
                           int32_t n_members, int64_t *d_member_partitions, int64_t *d_member_lag,
                           int64_t *d_unassigned, void *stream);
/* The same on shard `shard` (buffers and stream on that shard's device; la_sync_on reports a bad rank).  Shards hold disjoint
 * topic ranges, so the element-wise (wrapping) sum of their roll-ups is the roll-up of the whole batch. */
int la_member_loads_device_on(la_ctx *ctx, int shard, int64_t n_partitions, const int32_t *d_out_member_rank,
                              int64_t n_consumers, const int32_t *d_cons_rank, const int64_t *d_out_total_lag,
                              int32_t n_members, int64_t *d_member_partitions, int64_t *d_member_lag,
                              int64_t *d_unassigned, void *stream);

/* Who moved between two rebalances (nothing in the reference computes it).  Both assignments are results of an assign call
 * over ONE layout (the same d_part_off; for topics whose partition count changed see TWO LAYOUTS below) -- each in its own assignment
 * order, so the previous owner of an entry is found by a join on (topic, partition id), not by position.  With M = n_members,
 * for entry i of topic t of the current assignment:
 *   p = d_prev_member_rank[j] of the entry j of topic t of the previous assignment with d_prev_partition[j] == d_out_partition[i]
 *   q = p < 0 ? -1 : (d_prev_rank_map ? d_prev_rank_map[p] : p)          that owner in TODAY's ranks (-1: none, or it left)
 *   c = d_out_member_rank[i]
 *   d_prev_owner[i] = q;   the entry has MOVED iff q != c  (-1 -> -1 is no move: a topic without consumers both times, or an
 *                          owner that left with nobody taking over)
 *   a moved entry adds 1 to d_topic_moved[t] and d_moved[0], to d_member_gained[c] when c >= 0, to d_member_lost[q] when q >= 0
 * Outputs are OVERWRITTEN; each may be NULL, all NULL is LA_EINVAL.  Enqueues on `stream` and returns -- behind
 * la_assign_batch_device on the same stream it reads that call's results, no sync in between.  N == 0 and T == 0 are valid
 * (the outputs are zeroed).
 * Input contract: inside one topic the ids of each assignment are distinct and the two id sets are equal; ids are any int32.
 * n_members < 2^30.  Reported by la_sync as LA_EINVAL: a duplicate id inside a topic (either assignment), a current id without
 * a previous one, a previous rank outside [-1, M_prev), a mapped or current rank outside [-1, M).  Such an entry is never
 * stored through; what the rest of the call wrote is then unspecified, but inside the arrays.
 * Shape: max_partitions_per_topic is the hint of la_device_batch.  Within 4096 partitions (one workgroup joins a topic in
 * LDS) a topic over the hint is reported by la_sync as LA_ESHAPE and nothing is written for it (neither its d_prev_owner
 * entries nor its d_topic_moved; the other topics are done as usual); with a larger hint the library finds the larger topics
 * from h_part_off, which is then required (LA_EINVAL without it).
 * At most one kernel launch with a hint within that limit, three otherwise (la_last_launches; memsets do not count).  The table
 * of the larger topics is a buffer of the shard's own (LA_ENOMEM when it cannot be had), so the results kept for
 * la_group_last_by_member stay valid.  Buffer contract as everywhere in this header.
 *
 * TWO LAYOUTS (d_prev_part_off != NULL): the rebalance happened because topics gained partitions, appeared or were deleted, so
 * the previous assignment has a layout of its own -- d_prev_part_off [T_prev+1] over N_prev entries of d_prev_partition /
 * d_prev_member_rank.  Today's topic t is topic s = d_prev_topic[t] of it (t itself without a map, which needs T_prev == T);
 * its previous segment is [prev_part_off[s], prev_part_off[s+1]), or empty when s == -1 (the topic is new).  Then
 *   a current entry whose id has a previous entry in that segment is treated as above (d_prev_owner[i] = q, moved iff q != c);
 *   a current entry whose id has none is ADDED: d_prev_owner[i] = LA_MOVES_NO_PREVIOUS, +1 to d_topic_added[t] and d_added[0],
 *     +1 to d_member_gained[c] when c >= 0; it counts for neither d_topic_moved nor d_moved;
 *   a previous entry j of the segment that no current id matched is REMOVED: +1 to d_topic_removed[t] and d_removed[0], +1 to
 *     d_member_lost[q_j] when q_j >= 0 (q_j: its owner in today's ranks, mapped as above).
 * So gained[r] counts what r holds now and did not hold before, lost[r] the reverse; with equal id sets every number is the
 * one-layout call's and added = removed = 0.  A missing id is no error in this form.  la_sync reports as LA_EINVAL: a duplicate
 * id inside either segment (also among the added ids, and in a new topic), a rank out of range as above, a d_prev_topic[t]
 * outside [-1, T_prev); such an entry or topic is skipped and nothing is read or stored through it (a current entry with a bad
 * rank is skipped before its id is looked up, so its previous entry is then counted as removed: the numbers of a call that
 * ends in LA_EINVAL are unspecified, as above).  Not checked: no previous topic is named twice.
 * A previous topic that no entry names is not looked at -- list a deleted topic today as a topic without partitions to have
 * its partitions counted as removed (the assign call accepts such topics).  All nine outputs are overwritten, each may be
 * NULL, all NULL is LA_EINVAL.  T == 0, N == 0 and N_prev == 0 are valid in any combination (N == 0: everything removed).
 * Shape: the hint bounds the topics of BOTH layouts; a pair (t, s) is joined in LDS while max(P_t, P_prev_s) <= 4096 and a pair
 * over a hint within that limit is LA_ESHAPE with nothing written for it.  With a larger hint the larger pairs are found on the
 * host, from h_part_off, h_prev_part_off and (with d_prev_topic) h_prev_topic, which must equal the device arrays; LA_EINVAL
 * at the call when one is missing, an offset array does not ascend from 0 to N / N_prev, or a map entry lies outside
 * [-1, T_prev).  At most one launch with a hint within the limit, four otherwise (LDS form, insert, lookup, sweep).
 *
 * struct_size: 128 (the struct up to d_moved: one layout, nothing behind byte 128 is read) or sizeof(la_moves_args) of this
 * header and above; anything else is LA_EINVAL.  With d_prev_part_off == NULL no field from n_prev_topics on is looked at. */
#define LA_MOVES_NO_PREVIOUS (-2)
typedef struct la_moves_args {
    int32_t struct_size;              /* sizeof(la_moves_args) of the caller's header */
    int32_t n_topics;                 /* T */
    int64_t n_partitions;             /* N = part_off[T] */
    int64_t max_partitions_per_topic; /* shape hint, as in la_device_batch */
    const int64_t *d_part_off;        /* [T+1], the layout BOTH assignments share */
    const int64_t *h_part_off;        /* host copy; required when the hint exceeds the one-workgroup limit */
    const int32_t *d_out_partition;   /* [N] current assignment (results of an assign call) */
    const int32_t *d_out_member_rank; /* [N] */
    const int32_t *d_prev_partition;  /* [N] previous assignment, same layout ([N_prev] with d_prev_part_off) */
    const int32_t *d_prev_member_rank;/* [N] */
    int32_t n_members;                /* M: ranks of the CURRENT membership */
    int32_t n_prev_members;           /* M_prev; read only when d_prev_rank_map != NULL */
    const int32_t *d_prev_rank_map;   /* [M_prev] previous rank -> current rank, -1 = member left; NULL = identity (M_prev = M) */
    int32_t *d_prev_owner;            /* [N] or NULL */
    int64_t *d_topic_moved;           /* [T] or NULL */
    int64_t *d_member_gained;         /* [M] or NULL */
    int64_t *d_member_lost;           /* [M] or NULL */
    int64_t *d_moved;                 /* [1] or NULL */
    /* ---- two layouts; struct_size 128 ends here ---- */
    int32_t n_prev_topics;            /* T_prev */
    int32_t reserved;                 /* 0 */
    int64_t n_prev_partitions;        /* N_prev = prev_part_off[T_prev]; d_prev_partition / d_prev_member_rank then hold N_prev entries */
    const int64_t *d_prev_part_off;   /* [T_prev+1] layout of the PREVIOUS assignment.  NULL: one layout -- the call is exactly the
                                         one above and no field from n_prev_topics on is looked at */
    const int64_t *h_prev_part_off;   /* host copy; required where h_part_off is (hint beyond the one-workgroup limit) */
    const int32_t *d_prev_topic;      /* [T] today's topic t is topic d_prev_topic[t] of the previous layout, -1: the topic is new.
                                         NULL: identity (then T_prev must equal T) */
    const int32_t *h_prev_topic;      /* host copy; required with d_prev_topic where h_part_off is, not looked at without it */
    int64_t *d_topic_added;           /* [T] or NULL */
    int64_t *d_topic_removed;         /* [T] or NULL */
    int64_t *d_added;                 /* [1] or NULL */
    int64_t *d_removed;               /* [1] or NULL */
} la_moves_args;
int la_assignment_moves_device(la_ctx *ctx, const la_moves_args *args, void *stream);
/* The same on shard `shard` (buffers and stream on that shard's device; la_sync_on reports the errors).  Shards hold disjoint
 * topic ranges, so the element-wise sum of their gained / lost / moved is that of the whole batch. */
int la_assignment_moves_device_on(la_ctx *ctx, int shard, const la_moves_args *args, void *stream);

/* Certify an assignment (nothing in the reference computes it).  `batch` is the struct an assign call took, inputs and results:
 * the same memory, stream-ordered behind la_assign_batch_device with no sync in between, or any other arrays of that layout
 * (what la_unpack_results_on wrote on the far side of the all-gather, for instance).  Per topic with P partitions, C consumers,
 * distinct partition ids and strictly ascending cons_rank the reference's result is unique (Main.java:204-266), and the topic's
 * (d_out_partition, d_out_member_rank, d_out_total_lag) equal it if and only if
 *   V1 ids     every d_out_partition[i] of the segment is an id of the topic's d_partition_id segment, none used twice; lag_i is
 *              then the Java lag of that input partition (d_lag, or begin / end / committed with reset_mode, as the assign
 *              call computes it)
 *   V2 order   neighbours i, i+1: lag_i > lag_(i+1) signed, or the lags are equal and id_i < id_(i+1)
 *   V3 owners  C == 0: every rank is -1.  Otherwise every rank is one of the topic's cons_rank values; inside a round (positions
 *              [rC, min(P, rC + C))) the owners are distinct and the keys (the owner's wrapping int64 total over the earlier
 *              rounds, rank) ascend strictly along the positions, compared signed as Long.compare does; in a partial last
 *              round every consumer that was not picked has a key greater than the last picked one
 *   V4 totals  d_out_total_lag[k] is consumer k's final wrapping total (skipped when d_out_total_lag == NULL)
 * Outputs are OVERWRITTEN; either may be NULL, both NULL is LA_EINVAL:
 *   d_topic_verdict[t]  0: topic t is certified.  Otherwise a mask of LA_VERDICT_*.  A topic that is not certified never reads
 *                       0, and LA_VERDICT_UNCHECKED is exact (it stands alone: such a topic reports no other bit).  The class
 *                       bits 1-16 are diagnostics: a single fault sets the bit of its class, and once V1 fails what the later
 *                       checks report for that topic is unspecified.
 *   d_summary[4]        [0] topics with any of the bits 1-16, [1] topics UNCHECKED, [2] / [3] the lowest topic index counted in
 *                       [0] / [1], or -1
 * The order la_sticky_ties_device writes, put in place of d_out_partition, reads 0 or exactly LA_VERDICT_ORDER: inside a run of
 * equal lag its ids no longer ascend, V1, V3 and V4 hold.
 * A non-zero verdict is data, not an error: la_sync still returns LA_OK.  Offsets that leave [0, N) / [0, K) are LA_ESHAPE from
 * la_sync: nothing is read through them, and the topic reads UNCHECKED.  T == 0 and N == 0 are valid (summary 0, 0, -1, -1).
 * Of the batch's other fields: algo is not looked at, h_part_off / h_cons_off only with LA_FLAG_VERIFY_LARGE (below); flags with
 * LA_FLAG_WIRE_OUT is LA_EINVAL (unpack first), every flag but these two is ignored; the shape hints size the workgroups' LDS and nothing else -- a hint that is not
 * positive or lies beyond the limit asks for the limit, and a topic within the limit but over a hint is, as in the assign call,
 * LA_ESHAPE from la_sync (it reads UNCHECKED, the other topics are verified as usual).
 * At most one kernel launch (la_last_launches) behind the memsets that initialise the summary; no scratch, so the results kept
 * for la_group_last_by_member stay valid.  Buffer contract as everywhere in this header: element alignment only, writes only
 * inside [0, T) / [0, 4), the inputs and the results under test are never written.
 *
 * One workgroup verifies a topic in its LDS, which holds 4096 partitions and 4096 consumers: WITHOUT LA_FLAG_VERIFY_LARGE a larger
 * topic reads LA_VERDICT_UNCHECKED (data, not an error), no host array is read and nothing is allocated.
 * WITH LA_FLAG_VERIFY_LARGE (the flag means nothing to any other entry point) such topics are verified too:
 *   - h_part_off and h_cons_off are required (LA_EINVAL without them, or when they do not ascend inside [0, N] / [0, K]).  The
 *     host walks them and lists the LARGE topics: more than 4096 partitions or more than 4096 consumers.
 *   - Topics within the limit are verified as without the flag, verdict for verdict, the hint rules included.
 *   - Every large topic goes through the same join and the same V1-V4 in tables in device memory (about 60 B per partition and
 *     20 B per consumer of the large topics, a buffer of the shard's own that is grown on first use and freed by la_destroy --
 *     never the assign scratch, so kept results stay valid; LA_ENOMEM, with nothing enqueued, when it cannot be had).  Its verdict
 *     is 0 or a mask of LA_VERDICT_* under the rules above; d_summary counts it like any other topic.  Any consumer count is
 *     accepted; a topic of more than 2^30 - 2 partitions still reads LA_VERDICT_UNCHECKED.
 *   - The large topics are read through the HOST offsets alone.  Where they differ from d_part_off[t], d_part_off[t+1],
 *     d_cons_off[t], d_cons_off[t+1] the topic reads LA_VERDICT_UNCHECKED and la_sync returns LA_ESHAPE; so does a topic that is
 *     over the limit by the device's offsets but not by the host's.  Every verdict word is written, and counted, exactly once.
 *   - Launches: at most 7 kernel launches (la_last_launches) -- one for the topics within the limit, at most six for ALL large
 *     topics of the call side by side, whatever their number and size -- behind memsets and one copy of the topic list.  A
 *     flagged call whose batch holds no large topic enqueues what the unflagged call does and allocates nothing.
 *   - The call reads host memory while it is issued and may allocate: like an assign call that routes by h_part_off it must not
 *     be captured into a graph. */
#define LA_VERDICT_IDS        1   /* V1 */
#define LA_VERDICT_ORDER      2   /* V2 */
#define LA_VERDICT_OWNER      4   /* V3: not a subscriber, the -1 rule broken, or twice in a round */
#define LA_VERDICT_GREEDY     8   /* V3: the keys of a round do not ascend, or a consumer left out should have been picked */
#define LA_VERDICT_TOTALS    16   /* V4 */
#define LA_VERDICT_UNCHECKED 32   /* the topic could not be verified: more than 4096 partitions or more than 4096 consumers    *
                                   * (with LA_FLAG_VERIFY_LARGE: more than 2^30 - 2 partitions, or host and device offsets that *
                                   * disagree), duplicate ids in the INPUT segment, or a cons_rank segment that is not strictly  *
                                   * ascending                                                                                   */
int la_verify_assignment_device(la_ctx *ctx, const la_device_batch *batch, int32_t *d_topic_verdict, int64_t *d_summary,
                                void *stream);
/* The same on shard `shard` (buffers and stream on that shard's device; la_sync_on reports the errors). */
int la_verify_assignment_device_on(la_ctx *ctx, int shard, const la_device_batch *batch, int32_t *d_topic_verdict,
                                   int64_t *d_summary, void *stream);

/* The cooperative form of a rebalance (nothing in the reference computes it: its protocol is eager).  The TARGET is the result
 * of an assign call (d_part_off, d_out_partition, d_out_member_rank; ranks in [-1, M)); the call runs stream-ordered behind it,
 * no sync in between.  The previous owners come as Kafka hands them over, each member's Subscription.ownedPartitions():
 *   member r claims the entries [d_owned_member_off[r], d_owned_member_off[r+1]) of d_owned_topic / d_owned_partition
 *   (n_owned is the capacity of these two arrays).  Entries before off[0] and from off[M] on are not looked at, so the output of
 *   la_group_by_member_device can be passed as it is (its unassigned entries sit before member_off[0]): the lists of rebalance
 *   n are the owned lists of rebalance n + 1 without touching the host.  d_owned_topic[j] is an index into TODAY's topics, or -1
 *   where the host could not map the topic (it was deleted, say): such an entry is skipped and counted as stale.
 *   n_owned == 0: nobody owns anything (the first rebalance of a group); the three pointers may be NULL.
 * With M = n_members, for entry i of topic t of the target:
 *   c = d_out_member_rank[i];  q = the member whose owned slice holds (t, d_out_partition[i]), or -1 when none does
 *   d_prev_owner[i] = q
 *   d_coop_member_rank[i] = c when q == -1 or q == c, otherwise -1 -- in [-1, M), so la_group_by_member_device on it yields the
 *                           lists to return; the withheld entries land before member_off[0], next to those of topics without
 *                           consumers
 *   the entry is exactly one of   KEPT      c >= 0, q == c
 *                                 FRESH     c >= 0, q == -1
 *                                 WITHHELD  c >= 0, q >= 0, q != c      (the old owner revokes it, the follow-up rebalance
 *                                                                         hands it to c)
 *                                 DROPPED   c == -1, q >= 0             (the topic lost its consumers: the owner must let go)
 *                                 IDLE      c == -1, q == -1
 *   d_member_kept[M], d_member_fresh[M], d_member_pending[M]   the KEPT, FRESH and WITHHELD entries by c (pending: what the
 *                                                              follow-up rebalance will bring that member)
 *   d_member_release[M]   by q: WITHHELD plus DROPPED -- what that member has to revoke
 *   d_topic_withheld[T]   WITHHELD per topic
 *   d_summary[6]          kept, fresh, withheld, dropped, stale, followup.  stale: owned entries inside [off[0], off[M]) that
 *                         matched no entry of the target, those with topic -1 included; followup: 1 when withheld + dropped > 0
 *                         (another rebalance is needed), otherwise 0
 * All outputs are OVERWRITTEN; each may be NULL, all NULL is LA_EINVAL.  T == 0 and N == 0 are valid.  n_members < 2^30.
 * Partition ids are any int32.  Reported by la_sync as LA_EINVAL (a status bit of this call's own): a target rank outside
 * [-1, M), an owned topic outside [-1, T), the same (topic, id) claimed twice (by one member or by two).  Such an entry is never
 * stored through and nothing is read through it; the other numbers of that call are unspecified but stay inside the arrays.
 * Reported by la_sync as LA_ESHAPE: owned offsets that do not ascend inside [0, n_owned], part offsets that do not ascend from 0
 * to N.  Nothing is read through an offset: positions come from the walk over [0, n_owned) / [0, N) alone.  The offsets are
 * checked by the launch that uses them, so a call that has no use for an array does not look at it: d_part_off with N == 0,
 * d_owned_member_off with n_owned == 0.  Not checked: that the ids of a target topic are distinct (they are, in the result of
 * an assign call).
 * The join is ONE open-addressing table over the call, keyed by (topic, id) -- which fills a 64-bit word, so the claiming member
 * lives in a payload array beside the key array: 12 B per slot, 2^ceil(log2(2 n_owned)) slots, and no limit on topics, ids or
 * members beyond the ones above.  The table is a buffer of the shard's own, grown on first use and freed by la_destroy -- never
 * the assign scratch, so the results kept for la_group_last_by_member stay valid; LA_ENOMEM, with nothing enqueued, when it
 * cannot be had.  At most two kernel launches (la_last_launches; memsets do not count): insert the owned entries, look the
 * target up.  The call may allocate: it must not be captured into a graph.  The table is ONE per shard, zeroed and filled by
 * every call: the cooperative calls of a shard must be ordered among themselves -- one stream, or events between streams --
 * as for the table of la_assignment_moves_device and the tables of LA_FLAG_VERIFY_LARGE.  Buffer contract as everywhere in this header:
 * element alignment only, no write outside the arrays, inputs never written.
 * The call runs on shard 0 of the context (buffers and stream on that shard's device, la_sync reports the errors); a form with a
 * shard argument is not part of this ABI yet.
 * struct_size: sizeof(la_coop_args) of the caller's header; less than this library's is LA_EINVAL. */
typedef struct la_coop_args {
    int32_t struct_size;              /* sizeof(la_coop_args) of the caller's header */
    int32_t n_topics;                 /* T */
    int64_t n_partitions;             /* N = part_off[T] */
    const int64_t *d_part_off;        /* [T+1] */
    const int32_t *d_out_partition;   /* [N] the target (results of an assign call) */
    const int32_t *d_out_member_rank; /* [N] */
    int32_t n_members;                /* M */
    int32_t reserved;                 /* 0 */
    int64_t n_owned;                  /* capacity of d_owned_topic / d_owned_partition */
    const int64_t *d_owned_member_off;/* [M+1] */
    const int32_t *d_owned_topic;     /* [n_owned] index into today's topics, or -1 */
    const int32_t *d_owned_partition; /* [n_owned] */
    int32_t *d_prev_owner;            /* [N] or NULL */
    int32_t *d_coop_member_rank;      /* [N] or NULL */
    int64_t *d_member_kept;           /* [M] or NULL */
    int64_t *d_member_fresh;          /* [M] or NULL */
    int64_t *d_member_pending;        /* [M] or NULL */
    int64_t *d_member_release;        /* [M] or NULL */
    int64_t *d_topic_withheld;        /* [T] or NULL */
    int64_t *d_summary;               /* [6] or NULL */
} la_coop_args;
int la_cooperative_adjust_device(la_ctx *ctx, const la_coop_args *args, void *stream);

/* The cooperative round in one call: la_cooperative_adjust_device AND the lists a cooperative assignor hands back -- every
 * member's list of the ADJUSTED assignment.
 *   adjust             exactly as for la_cooperative_adjust_device: the same inputs, the same eight outputs, bit for bit what
 *                      that call writes, every one of them still optional -- here all eight may be NULL, the lists are outputs
 *                      too.  adjust.struct_size is not looked at (the outer struct_size covers the whole struct).
 *   member_off, grouped_topic, grouped_partition
 *                      what la_group_by_member_device writes for (d_part_off, d_out_partition, the adjusted ranks, M): member
 *                      r's list is [member_off[r], member_off[r+1]); the withheld entries and those of topics without consumers
 *                      sit before member_off[0].  So the lists of round n can be the owned arrays of round n + 1 as they lie.
 *                      The lists do not need adjust.d_coop_member_rank: they are the same when it is NULL.  N < 2^31.
 * Errors and hostile input as for la_cooperative_adjust_device: the same conditions are LA_EINVAL / LA_ESHAPE from la_sync,
 * nothing is read through an offset, a bad entry is never stored through; the lists of a call that ends in such an error are
 * unspecified but stay inside the arrays.  Buffer contract as everywhere in this header.  Both calls run on shard 0.
 * Two forms, the same results:
 *   ONE WORKGROUP  N <= 2048, n_owned <= 2048, M <= 2046 and T <= 2048 -- what a real rebalance is.  EXACTLY ONE kernel launch
 *                  (la_last_launches == 1), whatever is NULL or empty: the (topic, id) table, every counter and the lists live
 *                  in that workgroup's LDS, which writes every counting output in full.  No memset, no allocation, no table in
 *                  device memory, no scratch of any kind: the call can be captured into a graph, needs no ordering against
 *                  other cooperative calls, and the results kept for la_group_last_by_member stay valid.
 *   GENERAL        any limit exceeded, or LA_COOP_FORCE_TABLE: la_cooperative_adjust_device followed by
 *                  la_group_by_member_device on the adjusted ranks (a buffer of the shard's own when d_coop_member_rank is
 *                  NULL, grown before anything is enqueued: LA_ENOMEM then).  la_last_launches is the sum of the two: at most 2
 *                  plus the launches of that grouping (one up to 2 560 entries, two or a radix sort's beyond).  Everything said
 *                  of the table above holds: the call may allocate, must not be captured, and the cooperative calls of a shard
 *                  must be ordered among themselves.  The grouping runs in the scratch la_group_by_member_device uses, which is
 *                  the one la_group_last_by_member itself sorts in and holds no kept result: kept results stay valid here too.
 * struct_size: sizeof(la_coop_round_args) of the caller's header; less than this library's is LA_EINVAL.  flags: LA_COOP_*, any
 * other bit is LA_EINVAL.  member_off NULL, or grouped_partition NULL with N > 0, is LA_EINVAL.
 *
 * la_cooperative_round takes HOST memory for every pointer of the struct (the d_ prefix of `adjust` notwithstanding): what the
 * Java host and the C++ mirror have.  The inputs are packed into a staging buffer of shard 0's own -- pinned host memory and
 * device memory, grown before anything is enqueued (LA_ENOMEM then leaves nothing enqueued), never the assign scratch -- and
 * travel as ONE H2D copy; the device call above runs on la_stream(ctx); the outputs come back as ONE D2H copy; the call waits and
 * returns what la_sync would return (on an error the caller's outputs are left as they were).  A pending la_hint_next_call
 * survives it, and so do the results kept for la_group_last_by_member, in both forms (see above). */
#define LA_COOP_FORCE_TABLE 1   /* test hook / A-B: never the one-workgroup form; results identical */
typedef struct la_coop_round_args {
    int32_t struct_size;          /* sizeof(la_coop_round_args) of the caller's header */
    int32_t flags;                /* LA_COOP_* */
    la_coop_args adjust;          /* as for la_cooperative_adjust_device, every output optional */
    int64_t *member_off;          /* [M+1]  required */
    int32_t *grouped_topic;       /* [N] or NULL */
    int32_t *grouped_partition;   /* [N]  required when N > 0 */
} la_coop_round_args;
int la_cooperative_round_device(la_ctx *ctx, const la_coop_round_args *args, void *stream);
int la_cooperative_round(la_ctx *ctx, const la_coop_round_args *args);   /* every pointer is HOST memory */

/* A COOPERATIVE rebalance in one host call: la_assign_batch / _sparse / _lags AND la_cooperative_round on its result.  It replaces
 * no line of Main.java (the reference is eager); it is to a cooperative host what la_assign_batch_grouped is to the eager one:
 * offsets, subscriptions and what every member owns go in, the lists to hand back come out.  Every pointer is HOST memory.
 *   the rebalance     exactly the inputs of the assign calls: `lag` non-NULL is la_assign_batch_lags (the four offset fields are
 *                     not looked at); otherwise begin_off non-NULL is la_assign_batch and begin_off NULL is la_assign_batch_sparse
 *                     with (n_none, none_index, none_begin) -- LA_RESET_LATEST reads neither.  The TARGET is what that call
 *                     returns for these inputs, bit for bit, and every error condition of that call applies.
 *   the owned lists   n_owned, owned_member_off, owned_topic, owned_partition as la_coop_args has them; n_members is M.
 *   outputs           member_off, grouped_topic, grouped_partition and the eight adjust outputs: what la_cooperative_round writes
 *                     for that target and these owned lists, with the same LA_EINVAL / LA_ESHAPE conditions.  out_total_lag,
 *                     out_partition / out_member_rank (both or neither) describe the TARGET.  member_off is required,
 *                     grouped_partition when N > 0; everything else may be NULL.
 * On any error the caller's outputs are left as they were.  A pending la_hint_next_call is consumed, as by every host-buffer
 * assign call.  Afterwards the target stays kept on the device, exactly as after la_assign_batch_grouped: la_group_last_by_member
 * yields the target's EAGER lists.  Buffer contract as everywhere in this header.  The call runs on the whole context like
 * la_assign_batch; the round itself on shard 0.
 * Two forms, the same results:
 *   FUSED    the call is one a zero-copy staged call serves (one shard, staging layout within the zero-copy size), within the
 *            four ONE WORKGROUP limits above, without LA_COOP_FORCE_TABLE.  The owned arrays ride in the staging buffer the
 *            assignment kernels read in place; the target stays in device memory; ONE launch of the round's workgroup behind
 *            them reads it, writes every output into the staging buffer and stores the completion word the calling thread
 *            spins on.  No copy, no memset, no stream synchronize.  la_last_pipeline is LA_PIPELINE_ZERO_COPY; la_last_launches
 *            is what la_assign_batch reports for the same inputs and hints (the round takes the place of its finishing launch):
 *            2 for a one-tile batch with bounds hints.
 *   GENERAL  everything else: the assign call into buffers of the context's own, then la_cooperative_round; la_last_launches is
 *            the sum of the two.
 * struct_size: sizeof(la_assign_coop_args) of the caller's header; less than this library's is LA_EINVAL.  flags: LA_COOP_*, any
 * other bit is LA_EINVAL.  reserved must be 0. */
typedef struct la_assign_coop_args {
    int32_t struct_size;            /* sizeof(la_assign_coop_args) of the caller's header */
    int32_t flags;                  /* LA_COOP_* */
    int32_t n_topics, reset_mode;
    const int64_t *part_off;        /* [T+1] */
    const int32_t *partition_id;    /* [N] */
    const int64_t *lag;             /* [N] or NULL */
    const int64_t *begin_off;       /* [N] dense, or NULL: the sparse list */
    const int64_t *end_off, *committed_off;
    int64_t n_none;
    const int64_t *none_index, *none_begin;
    const int64_t *cons_off;        /* [T+1] */
    const int32_t *cons_rank;       /* [K] */
    int32_t n_members, reserved;    /* M; 0 */
    int64_t n_owned;
    const int64_t *owned_member_off;/* [M+1] */
    const int32_t *owned_topic, *owned_partition;   /* [n_owned] */
    int64_t *member_off;            /* [M+1]  required */
    int32_t *grouped_topic;         /* [N] or NULL */
    int32_t *grouped_partition;     /* [N]  required when N > 0 */
    int64_t *out_total_lag;         /* [K] or NULL: the target's totals */
    int32_t *out_partition, *out_member_rank;       /* [N] or both NULL: the target */
    int32_t *prev_owner, *coop_member_rank;         /* [N] or NULL */
    int64_t *member_kept, *member_fresh, *member_pending, *member_release;   /* [M] or NULL */
    int64_t *topic_withheld;        /* [T] or NULL */
    int64_t *summary;               /* [6] or NULL */
} la_assign_coop_args;
int la_assign_batch_cooperative(la_ctx *ctx, const la_assign_coop_args *args);

/* Sticky ties: among partitions of EQUAL lag, keep the previous owner (nothing in the reference computes it).  The reference
 * hands a topic's partitions out by (lag descending, id ascending); inside a run of equal lag it cannot tell them apart, and
 * permuting the partitions of such a run leaves the owner at every position, every consumer's count and total and every member's
 * load as they are.  So the reference's greedy decides who gets how much; this call decides WHICH partitions of a run, by their
 * previous owner.  A group that has caught up (most lags 0) otherwise reshuffles nearly every partition on every rebalance.
 * `batch` is the struct an assign call took, inputs and results, read as la_verify_assignment_device reads it: the lag from
 * d_lag, or from begin / end / committed with reset_mode; d_part_off, d_partition_id, d_out_partition and d_out_member_rank are
 * read; consumers, algo, the host offsets and every flag are ignored, but LA_FLAG_WIRE_OUT is LA_EINVAL (unpack first).  The
 * call runs stream-ordered behind the assign call and behind the call that produced d_prev_owner, no sync in between.
 * For topic t with positions i in [part_off[t], part_off[t+1]):
 *   lag_i = the Java lag of the input partition of the topic whose id is d_out_partition[i] (a join on the id, as in verify);
 *   a RUN is a maximal range of consecutive positions of equal lag_i;  c_i = d_out_member_rank[i];  q_i = d_prev_owner[i].
 * Inside one run R:
 *   1  for every c >= 0, S_c = the positions of R with c_i == c, ascending
 *   2  for every c >= 0, W_c = the positions of R with q_i == c, ascending
 *   3  for k < min(|S_c|, |W_c|) the partition at position W_c[k] goes to position S_c[k]
 *   4  the partitions not placed by 3, in ascending position, go to the positions not filled by 3, in ascending position
 *   5  d_sticky_partition[dest] = d_out_partition[src]
 * A position is KEPT when the partition placed there has q >= 0 and q equals the position's c; "kept before" is the same count
 * over d_out_partition as it came.  Kept after, sum over c of min(|S_c|, |W_c|) per run, is the most any permutation that keeps
 * the lag at every position can reach.  Owners -1 (a topic without consumers) and previous owners < 0 (-1, LA_MOVES_NO_PREVIOUS)
 * never match; a q that is no owner in the run matches nothing and is never used as an index.
 * d_out_member_rank and d_out_total_lag stay valid for the sticky order as they are: pass d_sticky_partition in place of
 * d_out_partition to la_cooperative_round_device, la_group_by_member_device or la_member_loads_device.  For
 * la_verify_assignment_device the sticky order reads 0 or exactly LA_VERDICT_ORDER per topic -- ids inside a run no longer
 * ascend; V1, V3 and V4 hold.
 * Outputs are OVERWRITTEN:
 *   d_sticky_partition[N]  required when N > 0; must not overlap any input (equal to d_out_partition: LA_EINVAL)
 *   d_topic_kept[T]        kept AFTER per topic, or NULL
 *   d_topic_saved[T]       kept after - kept before (>= 0), or NULL
 *   d_summary[4]           kept before, kept after, topics whose order changed, topics passed through, or NULL
 * One workgroup re-matches a topic in its LDS, which holds 4096 partitions.  A larger topic is PASSED THROUGH: its
 * d_sticky_partition is a copy of d_out_partition, saved 0, kept the count before, and it is counted in d_summary[3] -- data, not
 * an error: the reference's order is always a valid answer.  max_partitions_per_topic sizes the LDS as in verify: a hint that
 * is not positive or lies over the limit asks for the limit; a topic within the limit but over the hint is LA_ESHAPE from la_sync
 * and passed through.  Offsets that leave [0, N] are LA_ESHAPE: nothing is read through them and nothing at all is written for
 * that topic.  LA_EINVAL from la_sync (a status bit of this call's own), the topic passed through: a duplicate id in a topic's
 * input segment; an output id that is no input id of the topic, or appears twice.  T == 0 and N == 0 are valid (summary zeros).
 * At most one kernel launch (la_last_launches) behind the memset of the summary; no scratch and no allocation, so the call can be
 * captured into a graph and the results kept for la_group_last_by_member stay valid.  Buffer contract as everywhere in this
 * header: element alignment only, no write outside [0, N) / [0, T) / [0, 4), inputs never written.
 * The call runs on shard 0 of the context (buffers and stream on that shard's device, la_sync reports the errors); a form with a
 * shard argument is not part of this ABI yet.
 * LA_FLAG_STICKY_LARGE (batch->flags): topics of ANY size.  Without the flag nothing above changes: no host array is read,
 * nothing is allocated, large topics are passed through.  With it h_part_off is required and must ascend inside [0, N]
 * (LA_EINVAL at the call otherwise, as LA_FLAG_VERIFY_LARGE checks it).  Topics within 4096 partitions behave exactly as without
 * the flag, hint rules included.  Every topic of more than 4096 and at most LA_STICKY_GLOBAL_MAX_PARTITIONS (2^30 - 2)
 * partitions is re-matched by the GLOBAL FORM, whatever the hint says: all of them side by side through tables in device
 * memory -- the id join, the runs by a device-wide max-scan, the ranks inside (run, member) groups by the library's stable radix
 * sort, the leftovers by a device-wide scan -- with results bit for bit those of rules 1-5; d_summary[3] then counts only the
 * topics still passed through (a topic beyond 2^30 - 2 partitions: data, as before).  A BAD large topic (a duplicate input id, a
 * foreign or repeated output id) is LA_EINVAL from la_sync and passed through exactly -- copied, kept after = kept before, saved
 * 0, counted in d_summary[3] -- while every other topic of the call, large ones included, stays exact.  Every output word of a
 * call that ends in LA_OK or LA_EINVAL is written exactly once.  Large topics are read through the HOST's offsets alone: where
 * d_part_off[t] or d_part_off[t+1] differs from the host's for a large topic, or a topic is over the limit by the device's offsets
 * but not by the host's, la_sync returns LA_ESHAPE and the outputs of that call are unspecified but stay inside the arrays.
 * Launches (la_last_launches): at most 1 + LA_STICKY_GLOBAL_LAUNCHES (43), whatever the number and size of the large topics --
 * ten phases of the global form's own, the sort's plan and at most eight digit passes (one launch each while the call's large
 * topics hold fewer than 2^29 partitions together: 19 then; four each beyond).  A flagged call WITHOUT a large topic enqueues
 * exactly what the unflagged call does and touches no scratch.  Working memory is a buffer of the shard's own, never the assign
 * scratch (the results kept for la_group_last_by_member stay valid): 89 to 105 bytes per large-topic partition -- the table 16 to
 * 32, the lag 8, four 32-bit words of matching state, two sort elements of 24 and their look-back granules -- plus 12 per 1024
 * partitions and 32 per topic.  It is grown before anything is enqueued: LA_ENOMEM leaves nothing enqueued.  A limit of the CALL,
 * beside the per-topic one: the sort takes two elements per large-topic partition and at most 2^31 - 1 elements, so the large
 * topics of one call may hold 2^30 - 1 partitions TOGETHER (one topic of the largest size fits); a call beyond that is LA_ENOMEM
 * with nothing enqueued -- its working memory would exceed 100 GiB -- not a pass-through: split it.  With large topics the flagged call reads host memory and may allocate:
 * it must not be captured, and the flagged calls of one shard must be ordered among themselves (one stream, or events), as the
 * calls with LA_FLAG_VERIFY_LARGE.
 * struct_size: sizeof(la_sticky_args) of the caller's header; less than this library's is LA_EINVAL.  reserved must be 0. */
#define LA_STICKY_GLOBAL_LAUNCHES 43
#define LA_STICKY_GLOBAL_MAX_PARTITIONS ((1 << 30) - 2)
typedef struct la_sticky_args {
    int32_t struct_size;           /* sizeof(la_sticky_args) of the caller's header */
    int32_t reserved;              /* 0 */
    const int32_t *d_prev_owner;   /* [N] previous owner, in today's ranks, of the partition at each position of d_out_partition: *
                                    * what la_assignment_moves_device / la_cooperative_adjust_device write as d_prev_owner        */
    int32_t *d_sticky_partition;   /* [N] required when N > 0 */
    int64_t *d_topic_kept;         /* [T] or NULL */
    int64_t *d_topic_saved;        /* [T] or NULL */
    int64_t *d_summary;            /* [4] or NULL */
} la_sticky_args;
int la_sticky_ties_device(la_ctx *ctx, const la_device_batch *batch, const la_sticky_args *args, void *stream);

/* The cooperative round WITH sticky ties in one call.  `batch` is the struct an assign call took, inputs and results, read
 * exactly as la_sticky_ties_device reads it: the lag from d_lag, or from begin / end / committed with reset_mode; the hint rules
 * of that call apply; LA_FLAG_WIRE_OUT is LA_EINVAL.  The TARGET comes from `batch`: n_topics, n_partitions, d_part_off,
 * d_out_partition, d_out_member_rank -- the same five fields of round.adjust are not looked at, and neither are
 * round.struct_size and round.flags.  Everything else of `round` (the owned lists, n_members, the eight adjust outputs, the
 * three lists) is as for la_cooperative_round_device.
 * DEFINITION: every output is, bit for bit, what this chain writes on one stream:
 *   1  la_cooperative_adjust_device on the target, wanting only d_prev_owner;
 *   2  la_sticky_ties_device(batch, {that d_prev_owner, d_sticky_partition, d_topic_kept, d_topic_saved, d_sticky_summary});
 *   3  la_cooperative_round_device with d_sticky_partition in place of d_out_partition: the eight adjust outputs and the lists.
 * So the round's outputs describe the STICKY order: d_prev_owner[i] is the previous owner of the partition at position i of
 * d_sticky_partition, and the lists are the owned arrays of the next round as they lie.  d_out_member_rank and d_out_total_lag
 * of the batch stay valid for the sticky order as they are.
 * Errors are the union of the three calls' errors, reported by la_sync under the same conditions and with the same guarantees:
 * a bad entry is never stored through, nothing is read through an offset, outputs of a failing call are unspecified but stay
 * inside the arrays; a topic that step 2 passes through (a duplicate input id, a foreign or repeated output id, a topic over
 * the hint or over 4096 partitions) keeps the reference's order.  T == 0, N == 0 and n_owned == 0 are valid; with n_owned == 0
 * d_sticky_partition equals d_out_partition.  Buffer contract as everywhere in this header.  The call runs on shard 0.
 * LA_FLAG_STICKY_LARGE in batch->flags (h_part_off then required, checked at the call as in la_sticky_ties_device) reaches step 2
 * of the GENERAL form: topics of more than 4096 partitions are re-matched there as that call describes, its launches added to
 * the chain's; the sticky scratch is reserved together with the chain's other buffers, before the first launch.  The ONE
 * WORKGROUP form holds N <= 2048 and so no large topic: the flag changes nothing there.
 * Two forms, the same results:
 *   ONE WORKGROUP  N <= LA_COOP_STICKY_ENTRIES (2048), n_owned <= LA_COOP_STICKY_OWNED (2048), M <= LA_COOP_STICKY_MEMBERS
 *                  (2046) and T <= LA_COOP_STICKY_TOPICS (2048), without LA_COOP_FORCE_TABLE.  EXACTLY ONE kernel launch
 *                  (la_last_launches == 1): both joins, the re-matching, every counter and the lists live in that workgroup's
 *                  LDS.  No memset, no allocation, no scratch: the call can be captured into a graph and the results kept for
 *                  la_group_last_by_member stay valid.  A topic over the batch's hint is found by the kernel itself: LA_ESHAPE
 *                  from la_sync, the topic passed through, as in step 2.
 *   GENERAL        anything else: the chain above through the same launchers; la_last_launches is their sum.  The intermediate
 *                  d_prev_owner (and the adjusted ranks when d_coop_member_rank is NULL) live in buffers of shard 0's own; these
 *                  intermediates of the call's own and the (topic, id) table are grown before anything is enqueued (LA_ENOMEM
 *                  from them leaves nothing enqueued; the grouping at the end may still grow its scratch behind the first two
 *                  steps, as in la_cooperative_round_device).  What la_cooperative_round_device says
 *                  of its general form holds: the call may allocate, must not be captured, and the cooperative calls of a shard
 *                  must be ordered among themselves.
 * struct_size: sizeof(la_coop_sticky_args) of the caller's header; less than this library's is LA_EINVAL.  flags:
 * LA_COOP_FORCE_TABLE or 0, any other bit is LA_EINVAL.  round.adjust.reserved must be 0.  round.member_off NULL, or
 * round.grouped_partition NULL with N > 0, is LA_EINVAL. */
#define LA_COOP_STICKY_LARGE 2   /* la_assign_batch_cooperative_sticky only: sticky ties for topics of any size (see that call) */
#define LA_COOP_STICKY_ENTRIES 2048
#define LA_COOP_STICKY_OWNED 2048
#define LA_COOP_STICKY_MEMBERS 2046
#define LA_COOP_STICKY_TOPICS 2048
typedef struct la_coop_sticky_args {
    int32_t struct_size;            /* sizeof(la_coop_sticky_args) of the caller's header */
    int32_t flags;                  /* LA_COOP_FORCE_TABLE or 0 */
    la_coop_round_args round;       /* as for la_cooperative_round_device, but for the target (see above) */
    int32_t *d_sticky_partition;    /* [N] required when N > 0; must not overlap an input */
    int64_t *d_topic_kept;          /* [T] or NULL */
    int64_t *d_topic_saved;         /* [T] or NULL */
    int64_t *d_sticky_summary;      /* [4] or NULL */
} la_coop_sticky_args;
int la_cooperative_round_sticky_device(la_ctx *ctx, const la_device_batch *batch, const la_coop_sticky_args *args, void *stream);

/* A COOPERATIVE rebalance on the STICKY order in one host call: la_assign_batch_cooperative with the round replaced by the
 * sticky round above.  Every pointer is HOST memory.
 *   coop             exactly as for la_assign_batch_cooperative: the rebalance's inputs, the owned lists, the outputs.
 *                    coop.struct_size is not looked at; coop.flags holds LA_COOP_FORCE_TABLE and / or LA_COOP_STICKY_LARGE, any
 *                    other bit LA_EINVAL; coop.reserved must be 0.  LA_COOP_STICKY_LARGE (this call alone takes it, every
 *                    other call rejects it): the round runs with LA_FLAG_STICKY_LARGE and h_part_off = part_off, so topics
 *                    of more than 4096 partitions are re-matched too; without it, they are passed through.
 *   out_partition, out_member_rank, out_total_lag (of coop)   describe the TARGET, in the reference's order, bit for bit what the
 *                    assign call returns for these inputs.
 *   sticky_partition, the eight adjust outputs and the three lists   describe the STICKY order: what
 *                    la_cooperative_round_sticky_device writes for that target, these lags and these owned lists.
 *   topic_kept, topic_saved, sticky_summary   as d_topic_kept / d_topic_saved / d_sticky_summary of that call.
 * Every error condition of the assign call and of the sticky round applies; on any error the caller's outputs are left as they
 * were.  A pending la_hint_next_call is consumed.  The call makes NO promise about la_group_last_by_member afterwards.
 * Two forms, the same results, bit for bit on every output:
 *   FUSED    the call is one a zero-copy staged call serves (one shard, staging layout within the zero-copy size), within the
 *            four ONE WORKGROUP limits of la_cooperative_round_sticky_device, without LA_COOP_FORCE_TABLE (LA_COOP_STICKY_LARGE
 *            does not matter: a call of that size holds no large topic).  partition_id, the lag source and the owned arrays
 *            ride in the staging buffer the assignment kernels read in place -- the lags, or end and committed plus a dense
 *            begin; for the sparse form the host scatters none_begin over zeros while packing, LA_RESET_LATEST stages no begin
 *            -- the target stays in device memory; ONE launch of the sticky round's workgroup behind them reads the target and,
 *            once and by index, the lag source, writes every output into the staging buffer and stores the completion word
 *            the calling thread spins on.  No copy, no memset, no stream synchronize.  la_last_pipeline is
 *            LA_PIPELINE_ZERO_COPY; la_last_launches is what the assign call reports for the same inputs and hints (the round
 *            takes the place of its finishing launch): 2 for a one-tile batch with bounds hints.  The target stays kept on
 *            the device as after la_assign_batch_cooperative.  Measured against the general form in one process
 *            (profiles/assign_coop_sticky_probe.txt) it is faster at 100, 1 000 and 2 048 partitions, so no size within the
 *            limits is excluded.
 *   GENERAL  everything else: the assign call runs into buffers of the context's own; then the target, the owned arrays,
 *            partition_id and the lag source (packed as above; the lag itself is computed on the device) travel as ONE H2D copy
 *            through the cooperative staging buffers of shard 0, la_cooperative_round_sticky_device runs on la_stream(ctx) with
 *            the largest topic as its hint and the outputs come back as ONE D2H copy.  la_last_launches is the sum of the
 *            assign call's and the round's.
 * LA_NO_FUSED_STICKY in the environment, read at every call of this entry point, sends every call through the GENERAL form
 * (an A/B hook for tests and probes).
 * struct_size: sizeof(la_assign_sticky_args) of the caller's header; less than this library's is LA_EINVAL.  reserved must be 0. */
typedef struct la_assign_sticky_args {
    int32_t struct_size, reserved;          /* sizeof(la_assign_sticky_args) of the caller's header; 0 */
    la_assign_coop_args coop;               /* exactly as for la_assign_batch_cooperative */
    int32_t *sticky_partition;              /* [N] or NULL */
    int64_t *topic_kept, *topic_saved;      /* [T] or NULL */
    int64_t *sticky_summary;                /* [4] or NULL */
} la_assign_sticky_args;
int la_assign_batch_cooperative_sticky(la_ctx *ctx, const la_assign_sticky_args *args);

/* The PINNED assignment: the follow-up of a cooperative rebalance that moves nothing that is owned (nothing in the reference
 * computes it).  The cooperative round withholds what changes owner and asks for a follow-up rebalance; that follow-up only
 * settles if it hands the withheld partitions out WITHOUT moving the owned ones, and the reference's greedy over fresh lags
 * does not: a lagging group's offsets move between two rebalances and most of the target moves with them.  Here a partition
 * that a subscriber of its topic owns stays with that owner and only the others are dealt out, by the reference's own rule,
 * from bins that start with what every consumer already holds.
 *   batch   the struct an assign call takes: topics, partition ids, the lag source (d_lag, or begin / end / committed with
 *           reset_mode, the lag computed exactly as the assign call computes it), d_cons_off / d_cons_rank, and the three result
 *           arrays.  algo, the hints, h_part_off / h_cons_off and every flag are ignored, except LA_FLAG_WIRE_OUT: LA_EINVAL,
 *           and LA_FLAG_PINNED_LARGE with the two host arrays (below).
 *   args    the owned lists, as la_coop_args has them, with the same rules: member r claims the entries
 *           [d_owned_member_off[r], d_owned_member_off[r+1]), entries before off[0] and from off[M] on are not looked at,
 *           topic -1 is stale; n_owned == 0: nobody owns anything and the three pointers may be NULL.
 * For topic t with consumer ranks R = cons_rank[c0:c1] (strictly ascending) and input partitions j of lag_j and id_j, q_j the
 * member whose owned slice holds (t, id_j), or -1:
 *   1  j is PINNED iff q_j is one of R, k_j its index there.  A partition whose claimant does not consume the topic is FOREIGN:
 *      it is dealt out like an unowned one (and the round that follows withholds it, as it should).
 *   2  every consumer k starts with count_k = its pinned partitions and total_k = the wrapping int64 sum of their lags: all
 *      pinned partitions are in the bins before anything is dealt.
 *   3  the positions are the reference's order, lag descending (signed), id ascending: d_out_partition is what
 *      la_assign_batch_device writes for the same inputs, bit for bit.
 *   4  walking the positions in ascending order, a pinned partition gets q_j; any other goes to the k with the least
 *      (count_k, total_k, R[k]), compared as Long.compare does; then count_k += 1, total_k += lag (wrapping).
 *   5  a topic without consumers: every rank is -1.  d_out_total_lag[c0 + k] is the final total_k.
 * With nothing owned the result IS the assign call's, bit for bit.  An input id that appears twice in a topic matches twice
 * (no error).  The three results have the layout of an assign result: la_group_by_member_device, the cooperative calls,
 * la_member_loads_device and la_assignment_moves_device take them as they are.  d_out_total_lag may be NULL.
 *   d_topic_free[T]   the partitions of the topic that are not pinned (what rule 4 dealt out; in a topic without consumers
 *                     all of them)
 *   d_summary[4]      pinned, free, foreign (part of free), stale: owned entries inside [off[0], off[M]) that matched no
 *                     partition, those with topic -1 included
 * Both are OVERWRITTEN and may be NULL.  T == 0, N == 0 and n_owned == 0 are valid.  n_members < 2^30.
 * Reported by la_sync as LA_EINVAL: a cons_rank segment that does not ascend strictly (the assign call's status bit); an owned
 * topic outside [-1, T) or the same (topic, id) claimed twice (the cooperative calls' bit).  As LA_ESHAPE: owned offsets that
 * do not ascend inside [0, n_owned] (positions come from the walk over the owned arrays alone), part or consumer offsets of a
 * topic that descend or leave [0, N] / [0, K] -- such a topic is skipped -- and a topic of more than LA_PINNED_MAX_PARTITIONS
 * partitions or LA_PINNED_MAX_CONSUMERS consumers: nothing is written for it, neither its results nor its totals, it counts
 * nowhere, and the other topics are done as usual.
 * One workgroup per topic holds the topic in its LDS.  The join is the (topic, id) table of la_cooperative_adjust_device, the
 * shard's own buffer: never the assign scratch (kept results stay valid), LA_ENOMEM with nothing enqueued when it cannot be
 * had, and this call is ordered with the shard's other cooperative calls.  At most two kernel launches behind the memsets
 * (la_last_launches): insert the owned entries, do the topics.  The call may allocate: it must not be captured.  Buffer
 * contract as everywhere in this header.  The call runs on shard 0.
 * struct_size: sizeof(la_pinned_args) of the caller's header; less than this library's is LA_EINVAL.  reserved, reserved2: 0.
 *
 * LA_FLAG_PINNED_LARGE (batch->flags): topics of ANY size.  Without the flag nothing above changes: no host array is read,
 * nothing is allocated, a topic over LA_PINNED_MAX_PARTITIONS is LA_ESHAPE and skipped.  With it batch->h_part_off and
 * batch->h_cons_off are required and must ascend inside [0, N] / [0, K] (LA_EINVAL at the call otherwise, nothing enqueued).  A
 * topic within 4096 partitions is done exactly as without the flag: same kernel, same results.  A topic of more than 4096 and at
 * most LA_PINNED_LARGE_MAX_PARTITIONS (2^30 - 2) partitions and at most LA_PINNED_MAX_CONSUMERS consumers is a LARGE topic: it
 * is assigned by the large form (la_pinned_large.hip) and every output is rules 1-5 bit for bit -- results, totals,
 * d_topic_free[t] and the topic's share of d_summary.  All large topics of a call run side by side.  A topic of more than
 * LA_PINNED_MAX_CONSUMERS consumers stays LA_ESHAPE and skipped, whatever its partitions.
 * Large topics are read through the HOST's offsets alone.  la_sync returns LA_ESHAPE, and the call's outputs are unspecified
 * but stay inside the arrays, when d_part_off[t], d_part_off[t+1], d_cons_off[t] or d_cons_off[t+1] differs from the host's for
 * a large topic, or when a topic is large by the device's offsets but not by the host's.  The errors above keep their codes in
 * a large topic (unsorted ranks, a double claim, an owned topic out of range: LA_EINVAL); an input id that appears twice in a
 * large topic matches twice.
 * Launches (la_last_launches): at most 2 + LA_PINNED_LARGE_LAUNCHES, whatever the number of large topics -- keys and plan of
 * the library's radix sort, its 12 digit passes once per tile class the large topics fall into (at most three: below 2^17,
 * below 3 x 2^20 partitions, above), classify, chunk scan, compact, levels; the count is the same for one large topic as for
 * several of one tile class.  A flagged call without a large topic enqueues exactly what the unflagged call does and touches
 * no new scratch.
 * Working memory is a buffer of the shard's own, never the assign scratch (kept results stay valid), grown before anything is
 * enqueued (LA_ENOMEM leaves nothing enqueued): per large-topic partition 24 B of sort buffers (two keys of 8, two payloads
 * of 4), 0.5 B of the sort's look-back granules, 1 B of flags and 4 B of the free list => about 30 B, + 4 B per chunk of 1024
 * positions, 12 B per consumer of a large topic and about 26 KiB of sort control per large topic.  A call whose large topics
 * hold more than LA_PINNED_LARGE_MAX_PARTITIONS partitions together is LA_ENOMEM with nothing enqueued.  With large topics the
 * call reads host memory and may allocate: it must not be captured, and flagged calls of one shard must be ordered among
 * themselves. */
#define LA_PINNED_MAX_PARTITIONS 4096
#define LA_PINNED_MAX_CONSUMERS  2048
#define LA_PINNED_LARGE_MAX_PARTITIONS ((1 << 30) - 2)
#define LA_PINNED_LARGE_LAUNCHES 42
typedef struct la_pinned_args {
    int32_t struct_size, reserved;           /* sizeof(la_pinned_args) of the caller's header; 0 */
    int32_t n_members, reserved2;            /* M; 0 */
    int64_t n_owned;                         /* capacity of d_owned_topic / d_owned_partition */
    const int64_t *d_owned_member_off;       /* [M+1] */
    const int32_t *d_owned_topic, *d_owned_partition;   /* [n_owned] */
    int64_t *d_topic_free;                   /* [T] or NULL */
    int64_t *d_summary;                      /* [4] or NULL: pinned, free, foreign (part of free), stale */
} la_pinned_args;
int la_assign_pinned_device(la_ctx *ctx, const la_device_batch *batch, const la_pinned_args *args, void *stream);

/* LA_COOP_PINNED, in la_assign_coop_args.flags of la_assign_batch_cooperative only (every other entry answers LA_EINVAL to the
 * bit): the TARGET of the call is the pinned assignment above instead of the assign call's.  Every output keeps its meaning;
 * out_partition, out_member_rank and out_total_lag describe the pinned target.  The inputs and the owned arrays travel as ONE
 * H2D copy through the cooperative staging buffers of shard 0 (the sparse begin is scattered over zeros while packing), the
 * pinned assignment and then the round run on device memory on la_stream, the outputs come back as ONE D2H copy, one wait.  There
 * is no fused form.  A topic over LA_PINNED_MAX_PARTITIONS / LA_PINNED_MAX_CONSUMERS is LA_ESHAPE at the call, with nothing
 * enqueued: the caller falls back to the call without the flag.  On any error the caller's outputs are left as they were.  The
 * call makes NO promise about la_group_last_by_member afterwards. */
#define LA_COOP_PINNED 4
/* LA_COOP_PINNED_LARGE, valid only together with LA_COOP_PINNED on la_assign_batch_cooperative (alone, or on any other entry:
 * LA_EINVAL): the pinned assignment runs with LA_FLAG_PINNED_LARGE and the caller's part_off / cons_off as the host offsets.
 * The call then refuses only a topic of more than LA_PINNED_MAX_CONSUMERS consumers or LA_PINNED_LARGE_MAX_PARTITIONS
 * partitions (LA_ESHAPE, nothing enqueued). */
#define LA_COOP_PINNED_LARGE 8

#ifdef __cplusplus
}
#endif
#endif /* LAGASSIGN_H */
