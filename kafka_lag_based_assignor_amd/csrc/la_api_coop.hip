// la_api_coop.hip -- the cooperative and sticky entry points of include/lagassign.h: la_sticky_ties_device, la_cooperative_adjust_device,
// the two round calls on device memory, la_assign_pinned_device, la_cooperative_round on host buffers, and the two host calls
// that run an assign call (or, with LA_COOP_PINNED, the pinned assignment) and the round on its result.  Every struct of lagassign.h is checked and turned into its la_coop.h / la_kernels.h call in ONE
// function here; the host forms stage their arrays through the shard's cooperative staging buffers by ONE helper (CoopStage).
#include "la_ctx.h"

static_assert(LA_COOP_FORCE_TABLE == 1 && LA_COOP_STICKY_LARGE == 2 && LA_COOP_PINNED == 4 && LA_COOP_PINNED_LARGE == 8, "lagassign.h");
static_assert(LA_PINNED_LARGE_MAX_PARTITIONS == la::kPinnedLargeMaxPartitions && LA_PINNED_LARGE_LAUNCHES == la::kPinnedLargeLaunches, "lagassign.h");
static_assert(LA_PINNED_MAX_PARTITIONS == la::kPinnedMaxPartitions && LA_PINNED_MAX_CONSUMERS == la::kPinnedMaxConsumers, "lagassign.h");
static_assert(LA_STICKY_GLOBAL_LAUNCHES == la::kStickyGlobalLaunches && LA_STICKY_GLOBAL_MAX_PARTITIONS == la::kStickyGlobalMaxPartitions, "lagassign.h");

namespace {

// The host offsets a flagged call reads its large topics through: they ascend inside [0, n_partitions] (as verify checks them)
int sticky_large_offsets_ok(la_ctx* ctx, const la_device_batch& b) {
    if (!b.h_part_off) return fail(ctx, LA_EINVAL, "LA_FLAG_STICKY_LARGE: h_part_off is required");
    for (int32_t t = 0; t <= b.n_topics; ++t) {
        const int64_t p = b.h_part_off[t];
        if (p < 0 || p > b.n_partitions || (t > 0 && p < b.h_part_off[t - 1]))
            return fail(ctx, LA_EINVAL, "LA_FLAG_STICKY_LARGE: h_part_off must ascend inside [0, n_partitions] (topic %d)", t < b.n_topics ? t : t - 1);
    }
    return LA_OK;
}

// The host offsets a flagged pinned call reads its large topics through: both ascend inside [0, n_partitions] / [0, n_consumers]
int pinned_large_offsets_ok(la_ctx* ctx, const la_device_batch& b) {
    if (!b.h_part_off || !b.h_cons_off) return fail(ctx, LA_EINVAL, "LA_FLAG_PINNED_LARGE: h_part_off and h_cons_off are required");
    for (int32_t t = 0; t <= b.n_topics; ++t) {
        const int64_t p = b.h_part_off[t], c = b.h_cons_off[t];
        if (p < 0 || p > b.n_partitions || (t > 0 && p < b.h_part_off[t - 1]))
            return fail(ctx, LA_EINVAL, "LA_FLAG_PINNED_LARGE: h_part_off must ascend inside [0, n_partitions] (topic %d)", t < b.n_topics ? t : t - 1);
        if (c < 0 || c > b.n_consumers || (t > 0 && c < b.h_cons_off[t - 1]))
            return fail(ctx, LA_EINVAL, "LA_FLAG_PINNED_LARGE: h_cons_off must ascend inside [0, n_consumers] (topic %d)", t < b.n_topics ? t : t - 1);
    }
    return LA_OK;
}

// What la_sticky_ties_device and the sticky round check of a la_device_batch, and the batch's side of the validated call: the
// previous owners and the four outputs are for the caller to check and fill in.
int sticky_call_of(la_ctx* ctx, const la_device_batch& b, la::StickyCall* out) {
    if (b.n_topics < 0 || b.n_partitions < 0) return fail(ctx, LA_EINVAL, "negative size");
    if (b.flags & LA_FLAG_WIRE_OUT)
        return fail(ctx, LA_EINVAL, "LA_FLAG_WIRE_OUT: unpack the results with la_unpack_results_on before re-matching them");
    if (b.n_topics == 0 && b.n_partitions != 0) return fail(ctx, LA_EINVAL, "partitions without topics");
    if (b.n_topics > 0 && !b.d_part_off) return fail(ctx, LA_EINVAL, "null offsets");
    if (b.n_partitions > 0 && (!b.d_out_partition || !b.d_out_member_rank)) return fail(ctx, LA_EINVAL, "null results");
    if (b.n_partitions > 0 && (!b.d_partition_id || (!b.d_lag && (!b.d_end_off || !b.d_committed_off))))
        return fail(ctx, LA_EINVAL, "null per-partition input");
    if (!b.d_lag && b.reset_mode != LA_RESET_LATEST && !b.d_begin_off && b.n_partitions > 0)
        return fail(ctx, LA_EINVAL, "begin_off is required unless reset_mode is LA_RESET_LATEST");
    la::StickyCall c{};
    c.n_topics = b.n_topics;
    c.reset_latest = b.reset_mode == LA_RESET_LATEST ? 1 : 0;
    c.n_partitions = b.n_partitions;
    c.max_partitions_per_topic = b.max_partitions_per_topic;
    c.part_off = b.d_part_off;
    c.pid = b.d_partition_id;
    c.begin = b.d_begin_off;
    c.end = b.d_end_off;
    c.committed = b.d_committed_off;
    c.lag = b.d_lag;
    c.out_pid = b.d_out_partition;
    c.out_rank = b.d_out_member_rank;
    *out = c;
    return LA_OK;
}

// What la_cooperative_adjust_device and the two round calls check of a la_coop_args, and the validated call.  need_output: the
// eight outputs are all a call has (the round calls have the lists beside them).
int coop_call_of(la_ctx* ctx, const la_coop_args& g, bool need_output, la::CoopCall* out) {
    if (g.n_topics < 0 || g.n_partitions < 0 || g.n_members < 0 || g.n_owned < 0) return fail(ctx, LA_EINVAL, "negative size");
    if (g.reserved != 0) return fail(ctx, LA_EINVAL, "la_coop_args.reserved must be 0");
    if (g.n_members > la::kMovesMaxMembers) return fail(ctx, LA_EINVAL, "n_members must be below 2^30");
    if (need_output && !g.d_prev_owner && !g.d_coop_member_rank && !g.d_member_kept && !g.d_member_fresh && !g.d_member_pending &&
        !g.d_member_release && !g.d_topic_withheld && !g.d_summary)
        return fail(ctx, LA_EINVAL, "every output is NULL");
    if (g.n_topics == 0 && g.n_partitions != 0) return fail(ctx, LA_EINVAL, "partitions without topics");
    if (g.n_partitions > 0 && (!g.d_part_off || !g.d_out_partition || !g.d_out_member_rank)) return fail(ctx, LA_EINVAL, "null buffer");
    if (g.n_owned > 0 && (!g.d_owned_member_off || !g.d_owned_topic || !g.d_owned_partition))
        return fail(ctx, LA_EINVAL, "null owned buffer");
    la::CoopCall c{};
    c.n_topics = g.n_topics;
    c.n_members = g.n_members;
    c.n_partitions = g.n_partitions;
    c.n_owned = g.n_owned;
    c.part_off = g.d_part_off;
    c.out_partition = g.d_out_partition;
    c.out_member_rank = g.d_out_member_rank;
    c.owned_off = g.d_owned_member_off;
    c.owned_topic = g.d_owned_topic;
    c.owned_partition = g.d_owned_partition;
    c.prev_owner = g.d_prev_owner;
    c.coop_rank = g.d_coop_member_rank;
    c.member_kept = g.d_member_kept;
    c.member_fresh = g.d_member_fresh;
    c.member_pending = g.d_member_pending;
    c.member_release = g.d_member_release;
    c.topic_withheld = g.d_topic_withheld;
    c.summary = g.d_summary;
    *out = c;
    return LA_OK;
}

// The lists of a round over the r->c.n_partitions entries of its target, checked and taken into `r`.
int coop_lists_of(la_ctx* ctx, int64_t* member_off, int32_t* grouped_topic, int32_t* grouped_partition, la::CoopRoundCall* r) {
    if (!member_off) return fail(ctx, LA_EINVAL, "member_off is NULL");
    if (r->c.n_partitions > 0 && !grouped_partition) return fail(ctx, LA_EINVAL, "grouped_partition is NULL");
    if (r->c.n_partitions > 0x7FFFFFFF) return fail(ctx, LA_ESHAPE, "at most 2^31-1 entries are supported");
    r->member_off = member_off;
    r->grouped_topic = grouped_topic;
    r->grouped_partition = grouped_partition;
    return LA_OK;
}

// a la_coop_round_args, checked: the adjust part as above, the lists' own pointers, the flags
int coop_round_call_of(la_ctx* ctx, const la_coop_round_args* args, la::CoopRoundCall* out) {
    if (!args) return fail(ctx, LA_EINVAL, "args is NULL");
    if (args->struct_size < (int32_t)sizeof(la_coop_round_args))
        return fail(ctx, LA_EINVAL, "la_coop_round_args.struct_size is %d, this library takes %d and above", (int)args->struct_size, (int)sizeof(la_coop_round_args));
    if (args->flags & ~LA_COOP_FORCE_TABLE) return fail(ctx, LA_EINVAL, "la_coop_round_args.flags holds a bit this library does not know");
    la::CoopRoundCall r{};
    if (int rc = coop_call_of(ctx, args->adjust, false, &r.c)) return rc;
    if (int rc = coop_lists_of(ctx, args->member_off, args->grouped_topic, args->grouped_partition, &r)) return rc;
    *out = r;
    return LA_OK;
}

// [a, a + na) and [b, b + nb) share a byte (null or empty: they do not)
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b || !na || !nb) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

// Sticky ties (la_sticky.hip).  Without LA_FLAG_STICKY_LARGE it owns no scratch: everything lives in the workgroups' LDS and the
// caller's outputs, so the call can be captured.  With the flag the topics over the LDS limit go through tables in device memory
// (la_sticky_large.hip) -- the shard's own buffer, not the assign scratch.  Either way the results kept for
// la_group_last_by_member stay as they are.  On shard 0, like the cooperative calls.
LA_API int la_sticky_ties_device(la_ctx* ctx, const la_device_batch* batch, const la_sticky_args* args, void* stream) {
    return shard_entry<true>(ctx, 0, "exception in la_sticky_ties_device", [&](Shard& sh) -> int {
        if (!batch) return fail(ctx, LA_EINVAL, "batch is NULL");
        if (!args) return fail(ctx, LA_EINVAL, "args is NULL");
        if (args->struct_size < (int32_t)sizeof(la_sticky_args))
            return fail(ctx, LA_EINVAL, "la_sticky_args.struct_size is %d, this library takes %d and above", (int)args->struct_size, (int)sizeof(la_sticky_args));
        const la_device_batch& b = *batch;
        const la_sticky_args& g = *args;
        if (g.reserved != 0) return fail(ctx, LA_EINVAL, "la_sticky_args.reserved must be 0");
        la::StickyCall c{};
        if (int rc = sticky_call_of(ctx, b, &c)) return rc;
        if (b.n_partitions > 0 && !g.d_prev_owner) return fail(ctx, LA_EINVAL, "d_prev_owner is NULL");
        if (b.n_partitions > 0 && !g.d_sticky_partition) return fail(ctx, LA_EINVAL, "d_sticky_partition is NULL");
        if (b.n_partitions > 0 && g.d_sticky_partition == b.d_out_partition)
            return fail(ctx, LA_EINVAL, "d_sticky_partition must not be d_out_partition: the call does not work in place");
        c.prev_owner = g.d_prev_owner;
        c.sticky = g.d_sticky_partition;
        c.topic_kept = g.d_topic_kept;
        c.topic_saved = g.d_topic_saved;
        c.summary = g.d_summary;
        const bool large = (b.flags & LA_FLAG_STICKY_LARGE) != 0;
        if (large)
            if (int rc = sticky_large_offsets_ok(ctx, b)) return rc;
        hipError_t e = la::sticky_ties_launch(c, sh.lanes[0].d_status, (hipStream_t)stream, large ? &sh.sticky : nullptr, b.h_part_off);
        return e != hipSuccess ? hip_fail(ctx, e, "sticky_ties: %s") : LA_OK;
    });
}

// The cooperative form of a rebalance (la_coop.hip), on shard 0.  The table is the shard's own buffer, not the assign scratch:
// the results kept for la_group_last_by_member stay as they are.
LA_API int la_cooperative_adjust_device(la_ctx* ctx, const la_coop_args* args, void* stream) {
    return shard_entry<true>(ctx, 0, "exception in la_cooperative_adjust_device", [&](Shard& sh) -> int {
        if (!args) return fail(ctx, LA_EINVAL, "args is NULL");
        if (args->struct_size < (int32_t)sizeof(la_coop_args))
            return fail(ctx, LA_EINVAL, "la_coop_args.struct_size is %d, this library takes %d and above", (int)args->struct_size, (int)sizeof(la_coop_args));
        la::CoopCall c{};
        if (int rc = coop_call_of(ctx, *args, true, &c)) return rc;
        hipError_t e = la::cooperative_adjust_launch(sh.coop, c, sh.lanes[0].d_status, (hipStream_t)stream);
        return e != hipSuccess ? hip_fail(ctx, e, "cooperative_adjust: %s") : LA_OK;
    });
}

// The cooperative round in one call (la_coop_small.hip), on shard 0: one launch of one workgroup within the limits of la_coop.h,
// otherwise the table form and the grouping behind it.  Neither touches the assign scratch or a kept result.
LA_API int la_cooperative_round_device(la_ctx* ctx, const la_coop_round_args* args, void* stream) {
    return shard_entry<true>(ctx, 0, "exception in la_cooperative_round_device", [&](Shard& sh) -> int {
        la::CoopRoundCall r{};
        if (int rc = coop_round_call_of(ctx, args, &r)) return rc;
        hipError_t e = la::cooperative_round_launch(sh.coop, sh.lanes[0].large, r, (args->flags & LA_COOP_FORCE_TABLE) != 0,
                                                    sh.lanes[0].d_status, (hipStream_t)stream);
        return e != hipSuccess ? hip_fail(ctx, e, "cooperative_round: %s") : LA_OK;
    });
}

// A round whose owned arrays and outputs are already where the device reads and writes them, as the public struct
// coop_sticky_call_of takes (the target fields stay empty: that call takes them from its batch).
la_coop_round_args coop_round_args_of(const la::CoopRoundCall& r) {
    la_coop_round_args a{};
    a.struct_size = (int32_t)sizeof a;
    la_coop_args& adj = a.adjust;
    adj.struct_size = (int32_t)sizeof adj;
    adj.n_members = r.c.n_members;
    adj.n_owned = r.c.n_owned;
    adj.d_owned_member_off = r.c.owned_off;
    adj.d_owned_topic = r.c.owned_topic;
    adj.d_owned_partition = r.c.owned_partition;
    adj.d_prev_owner = r.c.prev_owner;
    adj.d_coop_member_rank = r.c.coop_rank;
    adj.d_member_kept = r.c.member_kept;
    adj.d_member_fresh = r.c.member_fresh;
    adj.d_member_pending = r.c.member_pending;
    adj.d_member_release = r.c.member_release;
    adj.d_topic_withheld = r.c.topic_withheld;
    adj.d_summary = r.c.summary;
    a.member_off = r.member_off;
    a.grouped_topic = r.grouped_topic;
    a.grouped_partition = r.grouped_partition;
    return a;
}

// la_device_batch + la_coop_sticky_args, checked: the batch as la_sticky_ties_device checks it, the round as
// la_cooperative_round_device checks it with the target taken from the batch, the sticky outputs.
int coop_sticky_call_of(la_ctx* ctx, const la_device_batch* batch, const la_coop_sticky_args* args, la::CoopStickyCall* out) {
    if (!batch) return fail(ctx, LA_EINVAL, "batch is NULL");
    if (!args) return fail(ctx, LA_EINVAL, "args is NULL");
    if (args->struct_size < (int32_t)sizeof(la_coop_sticky_args))
        return fail(ctx, LA_EINVAL, "la_coop_sticky_args.struct_size is %d, this library takes %d and above", (int)args->struct_size, (int)sizeof(la_coop_sticky_args));
    if (args->flags & ~LA_COOP_FORCE_TABLE) return fail(ctx, LA_EINVAL, "la_coop_sticky_args.flags holds a bit this library does not know");
    const la_device_batch& b = *batch;
    la::CoopStickyCall k{};
    if (int rc = sticky_call_of(ctx, b, &k.s)) return rc;
    const size_t n4 = (size_t)b.n_partitions * 4, n8 = (size_t)b.n_partitions * 8;
    if (b.n_partitions > 0 && !args->d_sticky_partition) return fail(ctx, LA_EINVAL, "d_sticky_partition is NULL");
    for (const void* in : {(const void*)b.d_out_partition, (const void*)b.d_out_member_rank, (const void*)b.d_partition_id})
        if (ranges_overlap(args->d_sticky_partition, n4, in, n4))
            return fail(ctx, LA_EINVAL, "d_sticky_partition overlaps an input: the call does not work in place");
    for (const void* in : {(const void*)b.d_lag, (const void*)b.d_begin_off, (const void*)b.d_end_off, (const void*)b.d_committed_off})
        if (ranges_overlap(args->d_sticky_partition, n4, in, n8))
            return fail(ctx, LA_EINVAL, "d_sticky_partition overlaps an input: the call does not work in place");
    const la_coop_args& ra = args->round.adjust;
    const size_t o4 = ra.n_owned > 0 ? (size_t)ra.n_owned * 4 : 0;
    if (ranges_overlap(args->d_sticky_partition, n4, b.d_part_off, ((size_t)b.n_topics + 1) * 8) ||
        ranges_overlap(args->d_sticky_partition, n4, ra.d_owned_member_off, ra.n_members >= 0 ? ((size_t)ra.n_members + 1) * 8 : 0) ||
        ranges_overlap(args->d_sticky_partition, n4, ra.d_owned_topic, o4) || ranges_overlap(args->d_sticky_partition, n4, ra.d_owned_partition, o4))
        return fail(ctx, LA_EINVAL, "d_sticky_partition overlaps an input: the call does not work in place");
    la_coop_args adjust = args->round.adjust;       // the target is the batch's
    adjust.n_topics = b.n_topics;
    adjust.n_partitions = b.n_partitions;
    adjust.d_part_off = b.d_part_off;
    adjust.d_out_partition = b.d_out_partition;
    adjust.d_out_member_rank = b.d_out_member_rank;
    if (int rc = coop_call_of(ctx, adjust, false, &k.r.c)) return rc;
    if (int rc = coop_lists_of(ctx, args->round.member_off, args->round.grouped_topic, args->round.grouped_partition, &k.r)) return rc;
    k.s.sticky = args->d_sticky_partition;
    k.s.topic_kept = args->d_topic_kept;
    k.s.topic_saved = args->d_topic_saved;
    k.s.summary = args->d_sticky_summary;
    if (b.flags & LA_FLAG_STICKY_LARGE) {            // step 2 of the chain re-matches the large topics too
        if (int rc = sticky_large_offsets_ok(ctx, b)) return rc;
        k.h_part_off = b.h_part_off;
    }
    *out = k;
    return LA_OK;
}

// The cooperative round with sticky ties in one call (la_coop_sticky_small.hip), on shard 0: one launch of one workgroup within
// the limits of la_coop.h, otherwise the three launchers in turn.  Neither touches the assign scratch or a kept result.
LA_API int la_cooperative_round_sticky_device(la_ctx* ctx, const la_device_batch* batch, const la_coop_sticky_args* args, void* stream) {
    return shard_entry<true>(ctx, 0, "exception in la_cooperative_round_sticky_device", [&](Shard& sh) -> int {
        la::CoopStickyCall k{};
        if (int rc = coop_sticky_call_of(ctx, batch, args, &k)) return rc;
        hipError_t e = la::cooperative_round_sticky_launch(sh.coop, sh.sticky, sh.lanes[0].large, k, (args->flags & LA_COOP_FORCE_TABLE) != 0,
                                                           sh.lanes[0].d_status, (hipStream_t)stream);
        return e != hipSuccess ? hip_fail(ctx, e, "cooperative_round_sticky: %s") : LA_OK;
    });
}

// la_device_batch + la_pinned_args, checked: the batch as the sticky call checks it, with the consumers an assign call has and
// the results as outputs; the owned lists as coop_call_of checks them.
int pinned_call_of(la_ctx* ctx, const la_device_batch* batch, const la_pinned_args* args, la::PinnedCall* out) {
    if (!batch) return fail(ctx, LA_EINVAL, "batch is NULL");
    if (!args) return fail(ctx, LA_EINVAL, "args is NULL");
    if (args->struct_size < (int32_t)sizeof(la_pinned_args))
        return fail(ctx, LA_EINVAL, "la_pinned_args.struct_size is %d, this library takes %d and above", (int)args->struct_size, (int)sizeof(la_pinned_args));
    const la_device_batch& b = *batch;
    const la_pinned_args& g = *args;
    if (g.reserved != 0 || g.reserved2 != 0) return fail(ctx, LA_EINVAL, "la_pinned_args.reserved and reserved2 must be 0");
    if (b.n_topics < 0 || b.n_partitions < 0 || b.n_consumers < 0 || g.n_members < 0 || g.n_owned < 0) return fail(ctx, LA_EINVAL, "negative size");
    if (g.n_members > la::kMovesMaxMembers) return fail(ctx, LA_EINVAL, "n_members must be below 2^30");
    if (b.flags & LA_FLAG_WIRE_OUT) return fail(ctx, LA_EINVAL, "LA_FLAG_WIRE_OUT: the pinned assignment writes plain results");
    if (b.n_topics == 0 && (b.n_partitions != 0 || b.n_consumers != 0)) return fail(ctx, LA_EINVAL, "partitions or consumers without topics");
    if (b.n_topics > 0 && (!b.d_part_off || !b.d_cons_off)) return fail(ctx, LA_EINVAL, "null offsets");
    if (b.n_consumers > 0 && !b.d_cons_rank) return fail(ctx, LA_EINVAL, "null consumer ranks");
    if (b.n_partitions > 0 && (!b.d_out_partition || !b.d_out_member_rank)) return fail(ctx, LA_EINVAL, "null results");
    if (b.n_partitions > 0 && (!b.d_partition_id || (!b.d_lag && (!b.d_end_off || !b.d_committed_off))))
        return fail(ctx, LA_EINVAL, "null per-partition input");
    if (!b.d_lag && b.reset_mode != LA_RESET_LATEST && !b.d_begin_off && b.n_partitions > 0)
        return fail(ctx, LA_EINVAL, "begin_off is required unless reset_mode is LA_RESET_LATEST");
    if (g.n_owned > 0 && (!g.d_owned_member_off || !g.d_owned_topic || !g.d_owned_partition))
        return fail(ctx, LA_EINVAL, "null owned buffer");
    la::PinnedCall c{};
    c.n_topics = b.n_topics;
    c.n_members = g.n_members;
    c.reset_latest = b.reset_mode == LA_RESET_LATEST ? 1 : 0;
    c.n_partitions = b.n_partitions;
    c.n_consumers = b.n_consumers;
    c.n_owned = g.n_owned;
    c.part_off = b.d_part_off;
    c.cons_off = b.d_cons_off;
    c.pid = b.d_partition_id;
    c.cons_rank = b.d_cons_rank;
    c.begin = b.d_begin_off;
    c.end = b.d_end_off;
    c.committed = b.d_committed_off;
    c.lag = b.d_lag;
    c.owned_off = g.d_owned_member_off;
    c.owned_topic = g.d_owned_topic;
    c.owned_partition = g.d_owned_partition;
    c.out_pid = b.d_out_partition;
    c.out_rank = b.d_out_member_rank;
    c.out_total = b.d_out_total_lag;
    c.topic_free = g.d_topic_free;
    c.summary = g.d_summary;
    if ((b.flags & LA_FLAG_PINNED_LARGE) && b.n_topics > 0)      // the large topics are found from the host's offsets
        if (int rc = pinned_large_offsets_ok(ctx, b)) return rc;
    *out = c;
    return LA_OK;
}

// the large form's scratch and host offsets of a checked call, or none: what pinned_launch takes behind the call
la::PinnedLargeScratch* pinned_large_of(Shard& sh, const la_device_batch& b) {
    return (b.flags & LA_FLAG_PINNED_LARGE) && b.n_topics > 0 ? &sh.pinned_large : nullptr;
}

// The pinned assignment (la_pinned.hip), on shard 0: the insert launch of the cooperative table, then one workgroup per topic.
// With LA_FLAG_PINNED_LARGE the topics over the LDS limit go through the large form (la_pinned_large.hip) in between, in a buffer
// of the shard's own.
// The table is the shard's own buffer, not the assign scratch: the results kept for la_group_last_by_member stay as they are.
LA_API int la_assign_pinned_device(la_ctx* ctx, const la_device_batch* batch, const la_pinned_args* args, void* stream) {
    return shard_entry<true>(ctx, 0, "exception in la_assign_pinned_device", [&](Shard& sh) -> int {
        la::PinnedCall c{};
        if (int rc = pinned_call_of(ctx, batch, args, &c)) return rc;
        hipError_t e = la::pinned_launch(sh.coop, c, sh.lanes[0].d_status, (hipStream_t)stream, pinned_large_of(sh, *batch),
                                         batch->h_part_off, batch->h_cons_off);
        return e != hipSuccess ? hip_fail(ctx, e, "assign_pinned: %s") : LA_OK;
    });
}

namespace {

// ---- host arrays through the cooperative staging buffers of a shard: one copy in, the device call, one copy out, one wait ----------
// In the order of the layout: the inputs, then the outputs; 8-byte arrays first on either side, so that every array is aligned
// for its element.  A call plans the slots it has (the others stay empty and take no room), then: coop_stage_begin, the device
// call over at(), coop_stage_upload, its launch, coop_stage_finish.
enum { kInPartOff, kInOwnedOff, kInConsOff, kInLag, kInEnd, kInCommitted, kInBegin, kInTargetPid, kInTargetRank, kInInputId, kInOwnedTopic,
       kInOwnedPartition, kInConsRank, kCoopStageIns,
       kOutMemberOff = kCoopStageIns, kOutKept, kOutFresh, kOutPending, kOutRelease, kOutWithheld, kOutSummary, kOutTopicKept,
       kOutTopicSaved, kOutStickySummary, kOutTargetTotal, kOutPrevOwner, kOutCoopRank, kOutListTopic, kOutListPartition, kOutSticky,
       kOutTargetPid, kOutTargetRank, kCoopStageSlots };

struct CoopStage {
    // An input: where it is copied from (null: the call fills host() itself after coop_stage_begin).  An output: where the caller
    // wants it (null: it does not).  `live`: the slot lies in the layout and at() is its device address.
    struct Slot { const void* from; void* to; size_t off, bytes; bool live; } slot[kCoopStageSlots];
    size_t in_bytes, total;
    char *hp, *dp;                                             // the pinned and the device copy of the layout
    void in(int s, const void* from, size_t bytes) { slot[s] = {from, nullptr, 0, bytes, bytes != 0}; }
    // (`room`: the slot holds its bytes even where the caller does not want them -- the kernels write there all the same)
    void out(int s, void* to, size_t bytes, bool room) { slot[s] = {nullptr, to, 0, bytes, to || room}; }
    template <typename T> T* at(int s) const { return slot[s].live ? (T*)(dp + slot[s].off) : nullptr; }
    template <typename T> T* host(int s) const { return (T*)(hp + slot[s].off); }
};

// The cooperative staging buffers of a shard (pinned host memory and device memory) hold `total` bytes: both grown before anything
// is enqueued, so a failure leaves nothing behind.
int coop_stage_reserve(la_ctx* ctx, la::CoopScratch& s, size_t total) {
    if (total > s.stage_h_cap) {
        if (s.stage_h) { (void)hipHostFree(s.stage_h); s.stage_h = nullptr; s.stage_h_cap = 0; }
        const size_t want = total + total / 4 + 256;
        const hipError_t e = hipHostMalloc(&s.stage_h, want, hipHostMallocDefault);
        if (e != hipSuccess) { s.stage_h = nullptr; return hip_fail(ctx, e, "cooperative_round staging (host): %s"); }
        s.stage_h_cap = want;
    }
    if (total > s.stage_d_cap) {
        if (s.stage_d) { (void)hipFree(s.stage_d); s.stage_d = nullptr; s.stage_d_cap = 0; }
        const size_t want = total + total / 4 + 256;
        const hipError_t e = hipMalloc(&s.stage_d, want);
        if (e != hipSuccess) { s.stage_d = nullptr; return hip_fail(ctx, e, "cooperative_round staging (device): %s"); }
        s.stage_d_cap = want;
    }
    return LA_OK;
}

// The planned slots laid out, both halves of the staging buffer reserved, the inputs packed into the pinned half.
int coop_stage_begin(la_ctx* ctx, la::CoopScratch& s, CoopStage& sg) {
    size_t at = 0;
    for (int i = 0; i < kCoopStageSlots; ++i) {
        if (i == kCoopStageIns) sg.in_bytes = at;
        sg.slot[i].off = at;
        if (sg.slot[i].live) at += (sg.slot[i].bytes + 7) & ~(size_t)7;
    }
    sg.total = at;
    if (int rc = coop_stage_reserve(ctx, s, sg.total)) return rc;
    sg.hp = static_cast<char*>(s.stage_h);
    sg.dp = static_cast<char*>(s.stage_d);
    for (int i = 0; i < kCoopStageIns; ++i)
        if (sg.slot[i].live && sg.slot[i].from) memcpy(sg.hp + sg.slot[i].off, sg.slot[i].from, sg.slot[i].bytes);
    return LA_OK;
}

int coop_stage_upload(la_ctx* ctx, const CoopStage& sg, hipStream_t st) {
    char *const hp = sg.hp, *const dp = sg.dp;
    const size_t in_bytes = sg.in_bytes;
    if (in_bytes) LA_HIP(ctx, hipMemcpyAsync(dp, hp, in_bytes, hipMemcpyHostToDevice, st));
    return LA_OK;
}

// The outputs back in one copy, the wait, what the kernels flagged -- and, everything having succeeded, the caller's arrays.
int coop_stage_finish(la_ctx* ctx, const CoopStage& sg, Lane& ln, hipStream_t st) {
    char *const hp = sg.hp, *const dp = sg.dp;
    const size_t in_bytes = sg.in_bytes, out_bytes = sg.total - sg.in_bytes;
    LA_HIP(ctx, hipMemcpyAsync(hp + in_bytes, dp + in_bytes, out_bytes, hipMemcpyDeviceToHost, st));
    if (int rc = sync_status(ctx, ln, st)) return rc;
    for (int i = kCoopStageIns; i < kCoopStageSlots; ++i)
        if (sg.slot[i].to && sg.slot[i].bytes) memcpy(sg.slot[i].to, hp + sg.slot[i].off, sg.slot[i].bytes);
    return LA_OK;
}

// The owned arrays and the eleven outputs of the host-side round `h` (every pointer the caller's; h.c's sizes are the round's)
// as slots.  The offsets and the partitions of the lists always have room; `room`: every other output has it too.
void coop_stage_plan_round(CoopStage& sg, const la::CoopRoundCall& h, bool room) {
    const size_t N = (size_t)h.c.n_partitions, n = (size_t)h.c.n_owned, M = (size_t)h.c.n_members, T = (size_t)h.c.n_topics;
    sg.in(kInOwnedOff, h.c.owned_off, n ? (M + 1) * 8 : 0);
    sg.in(kInOwnedTopic, h.c.owned_topic, n * 4);
    sg.in(kInOwnedPartition, h.c.owned_partition, n * 4);
    sg.out(kOutMemberOff, h.member_off, (M + 1) * 8, true);
    sg.out(kOutKept, h.c.member_kept, M * 8, room);
    sg.out(kOutFresh, h.c.member_fresh, M * 8, room);
    sg.out(kOutPending, h.c.member_pending, M * 8, room);
    sg.out(kOutRelease, h.c.member_release, M * 8, room);
    sg.out(kOutWithheld, h.c.topic_withheld, T * 8, room);
    sg.out(kOutSummary, h.c.summary, 6 * 8, room);
    sg.out(kOutPrevOwner, h.c.prev_owner, N * 4, room);
    sg.out(kOutCoopRank, h.c.coop_rank, N * 4, room);
    sg.out(kOutListTopic, h.grouped_topic, N * 4, room);
    sg.out(kOutListPartition, h.grouped_partition, N * 4, true);
}

// ... and the same round with those pointers in the device half of the staging buffer; the target stays as `d` has it.
la::CoopRoundCall coop_stage_round(const CoopStage& sg, la::CoopRoundCall d) {
    d.c.owned_off = sg.at<const int64_t>(kInOwnedOff);
    d.c.owned_topic = sg.at<const int32_t>(kInOwnedTopic);
    d.c.owned_partition = sg.at<const int32_t>(kInOwnedPartition);
    d.member_off = sg.at<int64_t>(kOutMemberOff);
    d.c.member_kept = sg.at<int64_t>(kOutKept);
    d.c.member_fresh = sg.at<int64_t>(kOutFresh);
    d.c.member_pending = sg.at<int64_t>(kOutPending);
    d.c.member_release = sg.at<int64_t>(kOutRelease);
    d.c.topic_withheld = sg.at<int64_t>(kOutWithheld);
    d.c.summary = sg.at<int64_t>(kOutSummary);
    d.c.prev_owner = sg.at<int32_t>(kOutPrevOwner);
    d.c.coop_rank = sg.at<int32_t>(kOutCoopRank);
    d.grouped_topic = sg.at<int32_t>(kOutListTopic);
    d.grouped_partition = sg.at<int32_t>(kOutListPartition);
    return d;
}

// la_cooperative_round_device on host buffers: `host` is the validated call with every pointer the caller's.  The device call on
// lane 0's stream; only the wanted outputs have room.  It neither takes nor spends a pending la_hint_next_call.
int coop_round_host(la_ctx* ctx, Shard& sh, const la::CoopRoundCall& host, bool force_table) {
    const la::CoopCall& h = host.c;
    const size_t N = (size_t)h.n_partitions;
    CoopStage sg{};
    sg.in(kInPartOff, h.part_off, N ? ((size_t)h.n_topics + 1) * 8 : 0);
    sg.in(kInTargetPid, h.out_partition, N * 4);
    sg.in(kInTargetRank, h.out_member_rank, N * 4);
    coop_stage_plan_round(sg, host, false);
    if (int rc = coop_stage_begin(ctx, sh.coop, sg)) return rc;
    la::CoopRoundCall d = coop_stage_round(sg, host);
    d.c.part_off = sg.at<const int64_t>(kInPartOff);
    d.c.out_partition = sg.at<const int32_t>(kInTargetPid);
    d.c.out_member_rank = sg.at<const int32_t>(kInTargetRank);
    Lane& ln = sh.lanes[0];
    hipStream_t st = ln.stream;
    if (int rc = coop_stage_upload(ctx, sg, st)) return rc;
    hipError_t e = la::cooperative_round_launch(sh.coop, ln.large, d, force_table, ln.d_status, st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return hip_fail(ctx, e, "cooperative_round: %s");
    }
    return coop_stage_finish(ctx, sg, ln, st);
}

// What both host calls check of a la_assign_coop_args behind its struct_size (known_flags: the LA_COOP_* bits the entry takes;
// flags_name: the field as the entry's error names it), and what they make of it: the assign call `c` with the caller's result
// arrays, and the host-side round `q` that `c` carries -- the owned lists and every output, all the caller's; the target is filled
// in by whoever runs the round.
int assign_coop_call_of(la_ctx* ctx, const la_assign_coop_args* g, int32_t known_flags, const char* flags_name, HostCall& c,
                        la::CoopRoundCall& q) {
    if (g->flags & ~known_flags) return fail(ctx, LA_EINVAL, "%s holds a bit this library does not know", flags_name);
    if (g->reserved != 0) return fail(ctx, LA_EINVAL, "la_assign_coop_args.reserved must be 0");
    if (g->n_topics < 0 || g->n_members < 0 || g->n_owned < 0) return fail(ctx, LA_EINVAL, "negative size");
    if (g->n_members > la::kMovesMaxMembers) return fail(ctx, LA_EINVAL, "n_members must be below 2^30");
    if (g->n_owned > 0 && (!g->owned_member_off || !g->owned_topic || !g->owned_partition))
        return fail(ctx, LA_EINVAL, "null owned buffer");
    if (!g->member_off) return fail(ctx, LA_EINVAL, "member_off is NULL");
    const int32_t T = g->n_topics;
    if (T > 0 && g->part_off && g->part_off[T] > 0 && !g->grouped_partition) return fail(ctx, LA_EINVAL, "grouped_partition is NULL");
    q.c.n_topics = T;
    q.c.n_members = g->n_members;
    q.c.n_owned = g->n_owned;
    q.c.owned_off = g->owned_member_off;
    q.c.owned_topic = g->owned_topic;
    q.c.owned_partition = g->owned_partition;
    q.c.prev_owner = g->prev_owner;
    q.c.coop_rank = g->coop_member_rank;
    q.c.member_kept = g->member_kept;
    q.c.member_fresh = g->member_fresh;
    q.c.member_pending = g->member_pending;
    q.c.member_release = g->member_release;
    q.c.topic_withheld = g->topic_withheld;
    q.c.summary = g->summary;
    q.member_off = g->member_off;
    q.grouped_topic = g->grouped_topic;
    q.grouped_partition = g->grouped_partition;
    c.T = T; c.part_off = g->part_off; c.pid = g->partition_id; c.cons_off = g->cons_off; c.cons_rank = g->cons_rank;
    c.out_pid = g->out_partition; c.out_rank = g->out_member_rank; c.out_total = g->out_total_lag;
    if (g->lag) {                                            // la_assign_batch_lags
        c.reset_mode = LA_RESET_LATEST;
        c.lag = g->lag;
    } else {                                                 // la_assign_batch, or la_assign_batch_sparse without a dense begin
        c.reset_mode = g->reset_mode; c.end = g->end_off; c.committed = g->committed_off; c.begin = g->begin_off;
        if (!g->begin_off) { c.sparse = true; c.n_none = g->n_none; c.none_index = g->none_index; c.none_begin = g->none_begin; }
    }
    c.coop = &q;
    c.coop_general = (g->flags & LA_COOP_FORCE_TABLE) != 0;
    return LA_OK;
}

// la_assign_batch_cooperative with LA_COOP_PINNED: the target is the pinned assignment.  The rebalance's inputs and the owned
// arrays through the cooperative staging buffers of shard 0 -- one copy in; la_assign_pinned_device and then the round on the
// device copy of its result, both on lane 0's stream; the target and the round's outputs in one copy out; one wait.  A topic
// over the limits (with LA_COOP_PINNED_LARGE: over the large form's) is LA_ESHAPE before anything is enqueued.  The caller's arrays are written only after everything succeeded.
int assign_coop_pinned(la_ctx* ctx, const la_assign_coop_args* g) {
    la::CoopRoundCall q{};
    HostCall unused;
    if (int rc = assign_coop_call_of(ctx, g, LA_COOP_FORCE_TABLE | LA_COOP_PINNED | LA_COOP_PINNED_LARGE, "la_assign_coop_args.flags", unused, q)) return rc;
    const bool any_size = (g->flags & LA_COOP_PINNED_LARGE) != 0;
    const int64_t max_p = any_size ? (int64_t)LA_PINNED_LARGE_MAX_PARTITIONS : (int64_t)LA_PINNED_MAX_PARTITIONS;
    if ((g->out_partition == nullptr) != (g->out_member_rank == nullptr)) return fail(ctx, LA_EINVAL, "out_partition and out_member_rank: both or neither");
    const int32_t T = g->n_topics;
    if (T > 0 && (!g->part_off || !g->cons_off)) return fail(ctx, LA_EINVAL, "part_off / cons_off are NULL");
    if (T > 0 && (g->part_off[0] != 0 || g->cons_off[0] != 0)) return fail(ctx, LA_EINVAL, "part_off / cons_off must start at 0");
    for (int32_t t = 0; t < T; ++t) {
        const int64_t p = g->part_off[t + 1] - g->part_off[t], c = g->cons_off[t + 1] - g->cons_off[t];
        if (p < 0 || c < 0 || g->part_off[t + 1] > 0x7FFFFFFF || g->cons_off[t + 1] > 0x7FFFFFFF)
            return fail(ctx, LA_EINVAL, "part_off / cons_off must ascend, up to 2^31-1 entries (topic %d)", t);
        if (p > max_p || c > LA_PINNED_MAX_CONSUMERS)
            return fail(ctx, LA_ESHAPE, "LA_COOP_PINNED: topic %d has %lld partitions and %lld consumers, the pinned assignment takes %lld and %d",
                        t, (long long)p, (long long)c, (long long)max_p, LA_PINNED_MAX_CONSUMERS);
    }
    const int64_t N = T > 0 ? g->part_off[T] : 0, K = T > 0 ? g->cons_off[T] : 0;
    const bool latest = g->lag != nullptr || g->reset_mode == LA_RESET_LATEST;
    const bool use_begin = !g->lag && !latest;
    if (N > 0 && (!g->partition_id || (!g->lag && (!g->end_off || !g->committed_off)))) return fail(ctx, LA_EINVAL, "null per-partition input");
    if (use_begin && !g->begin_off && g->n_none > 0 && (!g->none_index || !g->none_begin)) return fail(ctx, LA_EINVAL, "null sparse begin list");
    if (use_begin && !g->begin_off && g->n_none < 0) return fail(ctx, LA_EINVAL, "negative size");
    if (K > 0 && !g->cons_rank) return fail(ctx, LA_EINVAL, "null consumer ranks");
    q.c.n_partitions = N;
    if (int rc = coop_lists_of(ctx, g->member_off, g->grouped_topic, g->grouped_partition, &q)) return rc;

    Shard& sh = ctx->shards[0];
    LA_HIP(ctx, hipSetDevice(sh.device));
    const size_t Ts = (size_t)T, Ns = (size_t)N, Ks = (size_t)K;
    CoopStage sg{};
    sg.in(kInPartOff, g->part_off, T > 0 ? (Ts + 1) * 8 : 0);
    sg.in(kInConsOff, g->cons_off, T > 0 ? (Ts + 1) * 8 : 0);
    sg.in(kInLag, g->lag, g->lag ? Ns * 8 : 0);
    sg.in(kInEnd, g->end_off, g->lag ? 0 : Ns * 8);
    sg.in(kInCommitted, g->committed_off, g->lag ? 0 : Ns * 8);
    sg.in(kInBegin, g->begin_off, use_begin ? Ns * 8 : 0);       // (without a dense begin: filled from the sparse list below)
    sg.in(kInInputId, g->partition_id, Ns * 4);
    sg.in(kInConsRank, g->cons_rank, Ks * 4);
    coop_stage_plan_round(sg, q, false);
    sg.out(kOutTargetTotal, g->out_total_lag, Ks * 8, true);
    sg.out(kOutTargetPid, g->out_partition, Ns * 4, true);
    sg.out(kOutTargetRank, g->out_member_rank, Ns * 4, true);
    if (int rc = coop_stage_begin(ctx, sh.coop, sg)) return rc;
    if (use_begin && !g->begin_off && Ns) {                      // the sparse list over zeros: marshalling, the lag itself is lag_of's
        int64_t* const begin = sg.host<int64_t>(kInBegin);
        memset(begin, 0, Ns * 8);
        for (int64_t i = 0; i < g->n_none; ++i)
            if (g->none_index[i] >= 0 && g->none_index[i] < N) begin[g->none_index[i]] = g->none_begin[i];
    }
    la_device_batch b{};
    b.n_topics = T;
    b.reset_mode = latest ? LA_RESET_LATEST : g->reset_mode;
    b.n_partitions = N;
    b.n_consumers = K;
    b.d_part_off = sg.at<int64_t>(kInPartOff);
    b.d_cons_off = sg.at<int64_t>(kInConsOff);
    b.d_partition_id = sg.at<int32_t>(kInInputId);
    b.d_cons_rank = sg.at<int32_t>(kInConsRank);
    b.d_lag = sg.at<int64_t>(kInLag);
    b.d_end_off = sg.at<int64_t>(kInEnd);
    b.d_committed_off = sg.at<int64_t>(kInCommitted);
    b.d_begin_off = sg.at<int64_t>(kInBegin);
    b.d_out_partition = sg.at<int32_t>(kOutTargetPid);
    b.d_out_member_rank = sg.at<int32_t>(kOutTargetRank);
    b.d_out_total_lag = sg.at<int64_t>(kOutTargetTotal);
    if (any_size) {                                              // the caller's offsets are the host's
        b.flags = LA_FLAG_PINNED_LARGE;
        b.h_part_off = g->part_off;
        b.h_cons_off = g->cons_off;
    }
    la::CoopRoundCall d = coop_stage_round(sg, q);
    d.c.part_off = b.d_part_off;
    d.c.out_partition = b.d_out_partition;
    d.c.out_member_rank = b.d_out_member_rank;
    la_pinned_args pa{};
    pa.struct_size = (int32_t)sizeof pa;
    pa.n_members = g->n_members;
    pa.n_owned = g->n_owned;
    pa.d_owned_member_off = d.c.owned_off;
    pa.d_owned_topic = d.c.owned_topic;
    pa.d_owned_partition = d.c.owned_partition;
    la::PinnedCall pc{};
    if (int rc = pinned_call_of(ctx, &b, &pa, &pc)) return rc;
    Lane& ln = sh.lanes[0];
    hipStream_t st = ln.stream;
    if (int rc = coop_stage_upload(ctx, sg, st)) return rc;
    hipError_t e = la::pinned_launch(sh.coop, pc, ln.d_status, st, pinned_large_of(sh, b), b.h_part_off, b.h_cons_off);
    if (e == hipSuccess) e = la::cooperative_round_launch(sh.coop, ln.large, d, (g->flags & LA_COOP_FORCE_TABLE) != 0, ln.d_status, st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return hip_fail(ctx, e, "assign_batch_cooperative (pinned): %s");
    }
    return coop_stage_finish(ctx, sg, ln, st);
}

}  // namespace

LA_API int la_cooperative_round(la_ctx* ctx, const la_coop_round_args* args) {
    return shard_entry<true>(ctx, 0, "exception in la_cooperative_round", [&](Shard& sh) -> int {
        la::CoopRoundCall r{};
        if (int rc = coop_round_call_of(ctx, args, &r)) return rc;
        return coop_round_host(ctx, sh, r, (args->flags & LA_COOP_FORCE_TABLE) != 0);
    });
}

// A cooperative rebalance from host buffers in one call: an assign call and the round on its result.  FUSED (la_host.hip,
// assign_small_zc): the round kernel is the zero-copy call's last launch.  GENERAL: the assign call into the context's own host
// buffers, then the body of la_cooperative_round on them; the caller's arrays are written only after both have succeeded.
LA_API int la_assign_batch_cooperative(la_ctx* ctx, const la_assign_coop_args* g) {
    DeviceGuard restore_device;
    LaunchSpan span(ctx);
    HintSpender spend_hints(ctx);
    if (!ctx) return LA_EINVAL;
    try {
        if (!g) return fail(ctx, LA_EINVAL, "args is NULL");
        if (g->struct_size < (int32_t)sizeof(la_assign_coop_args))
            return fail(ctx, LA_EINVAL, "la_assign_coop_args.struct_size is %d, this library takes %d and above", (int)g->struct_size, (int)sizeof(la_assign_coop_args));
        if (g->flags & LA_COOP_PINNED) return assign_coop_pinned(ctx, g);
        la::CoopRoundCall q{};
        HostCall c;
        if (int rc = assign_coop_call_of(ctx, g, LA_COOP_FORCE_TABLE, "la_assign_coop_args.flags", c, q)) return rc;
        bool done = false;
        c.coop_done = &done;
        if (int rc = assign_host(ctx, c)) return rc;
        if (done) return LA_OK;
        // the general form: the target lies in ctx->coop_target (totals | ids | ranks) -- or there is none (no topics)
        const int32_t T = g->n_topics;
        const int64_t N = T > 0 ? g->part_off[T] : 0, K = T > 0 ? g->cons_off[T] : 0;
        int64_t* const t_total = T > 0 ? ctx->coop_target.data() : nullptr;
        int32_t* const t_pid = T > 0 ? (int32_t*)(t_total + K) : nullptr;
        int32_t* const t_rank = T > 0 ? t_pid + N : nullptr;
        q.c.n_partitions = N;
        q.c.part_off = g->part_off;
        q.c.out_partition = t_pid;
        q.c.out_member_rank = t_rank;
        // (the lists once more, now that the target's size is known: beyond 2^31-1 entries the round refuses, LA_ESHAPE)
        if (int rc = coop_lists_of(ctx, g->member_off, g->grouped_topic, g->grouped_partition, &q)) return rc;
        Shard& sh = ctx->shards[0];
        LA_HIP(ctx, hipSetDevice(sh.device));
        if (int rc = coop_round_host(ctx, sh, q, (g->flags & LA_COOP_FORCE_TABLE) != 0)) return rc;
        if (g->out_total_lag && K > 0) memcpy(g->out_total_lag, t_total, (size_t)K * 8);
        if (g->out_partition && N > 0) {
            memcpy(g->out_partition, t_pid, (size_t)N * 4);
            memcpy(g->out_member_rank, t_rank, (size_t)N * 4);
        }
        return LA_OK;
    } catch (...) {
        return fail(ctx, LA_ENOMEM, "exception in la_assign_batch_cooperative");
    }
}

// A cooperative rebalance on the STICKY order from host buffers in one call.  FUSED (la_host.hip, assign_small_zc): the sticky
// round kernel is the zero-copy call's last launch -- one packing, no copy, one wait.  GENERAL: the assign call into buffers of
// the context's own (as coop_take_general arranges it), then target, owned arrays, partition ids and the lag source through the
// cooperative staging buffers -- one copy in, la_cooperative_round_sticky_device on lane 0's stream, one copy out, one wait; every
// output has room there, wanted or not.  The caller's arrays are written only after everything has succeeded.  LA_NO_FUSED_STICKY
// (environment, read at every call): the GENERAL form as it was before there was a fused one, for every call (A/B: tests,
// tools/coop_sticky_probe.py).
LA_API int la_assign_batch_cooperative_sticky(la_ctx* ctx, const la_assign_sticky_args* args) {
    DeviceGuard restore_device;
    LaunchSpan span(ctx);
    HintSpender spend_hints(ctx);
    if (!ctx) return LA_EINVAL;
    try {
        if (!args) return fail(ctx, LA_EINVAL, "args is NULL");
        if (args->struct_size < (int32_t)sizeof(la_assign_sticky_args))
            return fail(ctx, LA_EINVAL, "la_assign_sticky_args.struct_size is %d, this library takes %d and above", (int)args->struct_size, (int)sizeof(la_assign_sticky_args));
        if (args->reserved != 0) return fail(ctx, LA_EINVAL, "la_assign_sticky_args.reserved must be 0");
        const la_assign_coop_args* g = &args->coop;
        la::CoopRoundCall q{};
        HostCall c;
        if (int rc = assign_coop_call_of(ctx, g, LA_COOP_FORCE_TABLE | LA_COOP_STICKY_LARGE, "la_assign_sticky_args.coop.flags", c, q)) return rc;
        if ((g->out_partition == nullptr) != (g->out_member_rank == nullptr)) return fail(ctx, LA_EINVAL, "out_partition and out_member_rank: both or neither");
        // offsets the assign call would refuse are refused here, and so is a target beyond what the round takes
        const int32_t T = g->n_topics;
        const bool sized = T > 0 && g->part_off && g->cons_off && g->part_off[T] >= 0 && g->cons_off[T] >= 0 &&
                           g->part_off[T] <= 0x7FFFFFFF && g->cons_off[T] <= 0x7FFFFFFF;
        if (T > 0 && !sized) return fail(ctx, LA_EINVAL, "part_off / cons_off are NULL, or end below 0 or beyond 2^31-1 entries");
        const int64_t N = sized ? g->part_off[T] : 0, K = sized ? g->cons_off[T] : 0;
        // assign_host decides: FUSED ends in the sticky round's finishing form and sets `done`; otherwise it has become the plain
        // assign call into the context's own buffers that the GENERAL form below starts from (coop_take_general).  The A/B hook of
        // this entry point is one more reason for the latter, read at every call (the tests and the probe compare both forms in
        // one process)
        StickyOuts so;
        so.sticky_partition = args->sticky_partition;
        so.topic_kept = args->topic_kept;
        so.topic_saved = args->topic_saved;
        so.sticky_summary = args->sticky_summary;
        bool done = false;
        c.coop_done = &done; c.sticky = &so;
        if (getenv("LA_NO_FUSED_STICKY")) c.coop_general = true;
        if (int rc = assign_host(ctx, c)) return rc;
        if (done) return LA_OK;
        const int64_t* const t_total = sized ? ctx->coop_target.data() : nullptr;
        const int32_t* const t_pid = sized ? (const int32_t*)(t_total + K) : nullptr;
        const int32_t* const t_rank = sized ? t_pid + N : nullptr;
        int64_t hint = 0;                                        // the host knows the topics: the hint is the largest of them
        for (int32_t t = 0; t < T; ++t) hint = std::max<int64_t>(hint, g->part_off[t + 1] - g->part_off[t]);

        Shard& sh = ctx->shards[0];
        LA_HIP(ctx, hipSetDevice(sh.device));
        const size_t Ts = (size_t)T, Ns = (size_t)N;
        const bool latest = g->lag != nullptr || g->reset_mode == LA_RESET_LATEST;
        const bool use_begin = !g->lag && !latest;
        q.c.n_partitions = N;
        CoopStage sg{};
        sg.in(kInPartOff, g->part_off, T > 0 ? (Ts + 1) * 8 : 0);
        sg.in(kInLag, g->lag, g->lag ? Ns * 8 : 0);
        sg.in(kInEnd, g->end_off, g->lag ? 0 : Ns * 8);
        sg.in(kInCommitted, g->committed_off, g->lag ? 0 : Ns * 8);
        sg.in(kInBegin, g->begin_off, use_begin ? Ns * 8 : 0);   // (without a dense begin: filled from the sparse list below)
        sg.in(kInTargetPid, t_pid, Ns * 4);
        sg.in(kInTargetRank, t_rank, Ns * 4);
        sg.in(kInInputId, g->partition_id, Ns * 4);
        coop_stage_plan_round(sg, q, true);
        sg.out(kOutTopicKept, args->topic_kept, Ts * 8, true);
        sg.out(kOutTopicSaved, args->topic_saved, Ts * 8, true);
        sg.out(kOutStickySummary, args->sticky_summary, 4 * 8, true);
        sg.out(kOutSticky, args->sticky_partition, Ns * 4, true);
        if (int rc = coop_stage_begin(ctx, sh.coop, sg)) return rc;
        if (use_begin && !g->begin_off && Ns) {                  // the sparse list over zeros: marshalling, the lag itself is lag_of's
            int64_t* const begin = sg.host<int64_t>(kInBegin);
            memset(begin, 0, Ns * 8);
            for (int64_t i = 0; i < g->n_none; ++i)
                if (g->none_index[i] >= 0 && g->none_index[i] < N) begin[g->none_index[i]] = g->none_begin[i];
        }
        la_device_batch b{};
        b.n_topics = T;
        b.reset_mode = latest ? LA_RESET_LATEST : g->reset_mode;
        b.n_partitions = N;
        b.max_partitions_per_topic = hint;
        if ((g->flags & LA_COOP_STICKY_LARGE) && T > 0) {
            b.flags |= LA_FLAG_STICKY_LARGE;
            b.h_part_off = g->part_off;
        }
        b.d_part_off = sg.at<int64_t>(kInPartOff);
        b.d_partition_id = sg.at<int32_t>(kInInputId);
        b.d_lag = sg.at<int64_t>(kInLag);
        b.d_end_off = sg.at<int64_t>(kInEnd);
        b.d_committed_off = sg.at<int64_t>(kInCommitted);
        b.d_begin_off = sg.at<int64_t>(kInBegin);
        b.d_out_partition = sg.at<int32_t>(kInTargetPid);
        b.d_out_member_rank = sg.at<int32_t>(kInTargetRank);
        la_coop_sticky_args a{};
        a.struct_size = (int32_t)sizeof a;
        a.flags = g->flags & LA_COOP_FORCE_TABLE;
        a.round = coop_round_args_of(coop_stage_round(sg, q));
        a.d_sticky_partition = sg.at<int32_t>(kOutSticky);
        a.d_topic_kept = sg.at<int64_t>(kOutTopicKept);
        a.d_topic_saved = sg.at<int64_t>(kOutTopicSaved);
        a.d_sticky_summary = sg.at<int64_t>(kOutStickySummary);
        la::CoopStickyCall k{};
        if (int rc = coop_sticky_call_of(ctx, &b, &a, &k)) return rc;
        Lane& ln = sh.lanes[0];
        hipStream_t st = ln.stream;
        if (int rc = coop_stage_upload(ctx, sg, st)) return rc;
        hipError_t e = la::cooperative_round_sticky_launch(sh.coop, sh.sticky, ln.large, k, (g->flags & LA_COOP_FORCE_TABLE) != 0, ln.d_status, st);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);
            return hip_fail(ctx, e, "cooperative_round_sticky: %s");
        }
        if (int rc = coop_stage_finish(ctx, sg, ln, st)) return rc;
        // everything has succeeded: the target too
        if (g->out_partition && Ns) {
            memcpy(g->out_partition, t_pid, Ns * 4);
            memcpy(g->out_member_rank, t_rank, Ns * 4);
        }
        if (g->out_total_lag && K > 0) memcpy(g->out_total_lag, t_total, (size_t)K * 8);
        return LA_OK;
    } catch (...) {
        return fail(ctx, LA_ENOMEM, "exception in la_assign_batch_cooperative_sticky");
    }
}
