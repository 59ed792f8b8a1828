// la_moves_layouts.hip -- who moved between two rebalances when topics gained or lost partitions: la_assignment_moves_device
// with d_prev_part_off (lagassign.h).  The previous assignment has a layout of its own; today's topic t is topic prev_topic[t] of
// it (-1: the topic is new), so a (today, previous) PAIR of segments is joined on the partition id.  A current id without a
// previous entry is ADDED, a previous entry that no current id matched is REMOVED.
//
// The table is la_join.h's (table_insert / table_lookup unchanged), keyed by the id of the PREVIOUS entries.  After the lookups
// a live slot without the mark is a previous entry that nobody matched: the SWEEP walks the slots, not the previous entries
// again -- the payload is the mapped owner, so nothing but the table is read (8 B a slot in order), where a probe per previous
// entry would read its id again and touch a random line of the table each.
// A duplicate id is an error on either side.  On the previous side the insert finds it, on the current side the mark finds it
// when the id has a previous entry; two ADDED entries with one id both miss, so the missed ids are joined among themselves:
//
//   LDS form     pairs with both sides up to kMovesLdsMaxPartitions.  Persistent workgroups; per topic: clear the slots the pair
//                needs (2^ceil(log2(2 P_prev)): at most half full however many current ids miss), insert the previous segment,
//                barrier, look the current segment up, barrier, sweep.  table_lookup answers kStatusMoves both for an id that is
//                not there and for a hit that was marked before; table_has (a walk that marks nothing) tells them apart: the
//                keys do not change while lookups run.  A thread remembers which of its entries missed (one bit each); when the
//                topic has any, the same LDS is cleared again behind the sweep (2^ceil(log2(2 P_added)) slots: P_added <= the
//                hint, which sized the allocation) and the missed ids are inserted -- an equal id on the way is the duplicate.
//                Three 32-bit counters (moved, added, removed) per topic, one plain store each.  P_prev == 0: no first table,
//                everything is added.  P == 0: the insert still runs (duplicates and ranks are checked), then everything is
//                removed.
//   global form  pairs with a side beyond it, listed by the host from the host copies of both layouts and the map: a region of
//                the table each and three runs of workgroup steps (insert over the previous entries, lookup over the current
//                ones, sweep over the region's slots).  Three launches; their boundaries are the only grid-wide order.  Here
//                the region is sized from BOTH sides (2^ceil(log2(2 (P_prev + P)))) and a lookup that misses inserts its id
//                with the payload kAddedPayload: a second entry with that id then either hits it (lookup) or meets it on
//                its own insert -- kStatusMoves both ways, as is an insert that meets a previous id (the miss was a hit that
//                was marked before).  The sweep passes over those slots.
// Gained / lost go through la_moves.hip's LDS bins (la_moves_shared.h) while N + N_prev < 2^32 and the members fit.  Nothing is
// stored through a rank, an id or a map entry; no thread waits for another and every walk is bounded by the slot count.
// A current entry whose own rank is out of range is skipped BEFORE its lookup: its previous entry stays unmarked and is swept as
// removed.  The call is LA_EINVAL then and its numbers unspecified (lagassign.h); nothing is stored through the bad rank.
#include "la_moves_shared.h"

namespace la {

namespace {

// table + one copy of the bins (stride made odd) + two sets of the topic's three counters: what the LDS form asks for at most
constexpr size_t kLayoutsCounterBytes = 32;
constexpr size_t kLayoutsMaxLdsBytes =
    16 * (size_t)kMovesLdsMaxPartitions + 4 * (2 * (size_t)kMovesLdsMaxMembers + 1) + kLayoutsCounterBytes;
static_assert(kLayoutsMaxLdsBytes <= 160 * 1024, "table + bins fit one workgroup's LDS on gfx950");
static_assert(kMovesLdsMaxPartitions <= 32 * kMovesThreads, "a thread of the LDS form keeps one bit per entry of its own");
// global form: payload of an id that a lookup missed and inserted (no rank: n_members <= kMovesMaxMembers)
constexpr int32_t kAddedPayload = kMovesMaxMembers;

enum { kInsert = 0, kLookup = 1, kSweep = 2 };

struct LayoutsBig {             // one pair of the global form
    int64_t p0, n_part;         // today's entries
    int64_t q0, n_prev;         // the previous ones
    int64_t slot0;              // its region of the table
    int64_t chunk0[3];          // first workgroup step of the pair in each phase; a phase numbers its steps through all pairs
    int32_t topic, bits;        // today's topic; the region has 1 << bits slots: room for both sides at most half full
};

struct LayoutsArgs {
    MovesCall c;                // the one-layout fields
    int32_t n_prev_topics;
    int64_t n_prev_partitions;
    const int64_t* prev_part_off;
    const int32_t* prev_topic;
    int64_t *topic_added, *topic_removed, *added, *removed;
    uint32_t* status;
    int64_t cap;                // LDS form: partitions either side of a pair may have
    int32_t skip_large;         // pairs over `cap` belong to the global form: no error
    int32_t table_bits;         // LDS form: the table has 1 << table_bits slots
    int32_t tables, stride;     // bins: copies (a power of two) and their stride in counters (odd)
    uint64_t* table;            // global form
    const LayoutsBig* big;
    int32_t n_big;
    int64_t n_chunks[3];
};

// whether `id` is a key of the table; marks nothing
template <int SCOPE>
__device__ __forceinline__ bool table_has(uint64_t* table, int bits, int32_t id) {
    const uint64_t mask = (1ull << bits) - 1;
    uint64_t h = first_slot(id, bits);
    for (uint64_t n = 0; n <= mask; ++n) {
        const uint64_t w = __hip_atomic_load((unsigned long long*)(table + h), __ATOMIC_RELAXED, SCOPE);
        if (w == 0) return false;
        if ((uint32_t)w == (uint32_t)id) return true;
        h = (h + 1) & mask;
    }
    return false;
}

template <bool BINS>
__device__ __forceinline__ void count_gained(const MovesCall& c, uint32_t* mine, int32_t r) {
    if (r < 0) return;
    if (BINS) __hip_atomic_fetch_add(mine + r, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else if (c.member_gained) global_add(c.member_gained + r, 1);
}

template <bool BINS>
__device__ __forceinline__ void count_lost(const MovesCall& c, uint32_t* mine, int32_t r) {
    if (r < 0) return;
    if (BINS) __hip_atomic_fetch_add(mine + c.n_members + r, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else if (c.member_lost) global_add(c.member_lost + r, 1);
}

// one current entry: prev_owner[i], the gained / lost counts; *moved or *added += 1; returns status bits.  bits == 0: no table.
// *missed: the id has no previous entry.  INSERT_MISSES (the global form, whose region has room for them): such an id goes into
// the table; otherwise the caller joins the missed ids among themselves afterwards.
template <int SCOPE, bool BINS, bool INSERT_MISSES>
__device__ __forceinline__ uint32_t lookup_entry(const MovesCall& c, uint64_t* table, int bits, int64_t i, uint32_t* mine,
                                                 uint32_t* moved, uint32_t* added, bool* missed) {
    *missed = false;
    const int32_t id = __builtin_nontemporal_load(c.out_partition + i);
    const int32_t cur = __builtin_nontemporal_load(c.out_member_rank + i);
    if (cur < -1 || cur >= c.n_members) return kStatusMoves;
    int32_t q = kMovesNoPrevious;
    if (bits > 0) {
        const uint32_t st = table_lookup<SCOPE>(table, bits, id, &q);
        if (st == kStatusMoves) {                 // not there, or marked before: a duplicate in today's segment
            if (INSERT_MISSES) {
                const uint32_t st2 = table_insert<SCOPE>(table, bits, id, kAddedPayload);      // (meets the id if it is there)
                if (st2) return st2;
            } else if (table_has<SCOPE>(table, bits, id)) {
                return kStatusMoves;
            }
            q = kMovesNoPrevious;
        } else if (st) {
            return st;
        } else if (INSERT_MISSES && q == kAddedPayload) {
            return kStatusMoves;                  // an id that an earlier entry of today's segment missed and inserted
        }
    }
    if (c.prev_owner) __builtin_nontemporal_store(q, c.prev_owner + i);
    if (q == kMovesNoPrevious) {
        *missed = true;
        ++*added;
        count_gained<BINS>(c, mine, cur);
        return 0;
    }
    if (q == cur) return 0;
    ++*moved;
    count_gained<BINS>(c, mine, cur);
    count_lost<BINS>(c, mine, q);
    return 0;
}

// one slot behind the lookups: live without the mark = a previous entry that no current id matched
template <bool BINS>
__device__ __forceinline__ void sweep_slot(const MovesCall& c, uint64_t w, uint32_t* mine, uint32_t* removed) {
    if (w == 0 || (w & kSlotMark)) return;
    const int32_t q = (int32_t)((uint32_t)(w >> 32) & 0x7FFFFFFFu) - 2;
    if (q == kAddedPayload) return;              // (global form) an id of today's segment
    ++*removed;
    count_lost<BINS>(c, mine, q);
}

// LDS: [table: 1 << table_bits words][bins: tables x stride counters][moved, added, removed counts of a topic, two sets: a
// workgroup's pairs alternate between them, so that thread 0 zeroes the next pair's set while slower threads still read this one's]
template <bool BINS>
__global__ __launch_bounds__(kMovesThreads) void moves_layouts_lds_kernel(LayoutsArgs a) {
    extern __shared__ uint64_t layouts_lds[];
    constexpr int kScope = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int tid = (int)threadIdx.x;
    uint64_t* table = layouts_lds;
    uint32_t* bins = reinterpret_cast<uint32_t*>(layouts_lds + ((size_t)1 << a.table_bits));
    uint32_t* counts = bins + (BINS ? a.tables * a.stride : 0);
    uint32_t* mine = bins + (size_t)(tid & (a.tables - 1)) * a.stride;
    if (BINS) clear_bins(a, bins, tid);          // (the first pair's barriers order it before the first add; so does the flush's)
    uint32_t bad = 0;
    uint64_t total[3] = {0, 0, 0};               // thread 0: moved, added, removed entries of this workgroup's topics
    uint32_t* const both_counts = counts;
    int pairs_done = 0;
    for (int64_t t = blockIdx.x; t < a.c.n_topics; t += gridDim.x) {
        // workgroup-uniform, as all that follows from it
        const int64_t p0 = a.c.part_off[t], np = a.c.part_off[t + 1] - p0;
        const int32_t s = a.prev_topic ? a.prev_topic[t] : (int32_t)t;
        if (s < -1 || s >= a.n_prev_topics) {    // nothing is read through it
            bad |= kStatusMoves;
            continue;
        }
        int64_t q0 = 0, nq = 0;
        if (s >= 0) {
            q0 = a.prev_part_off[s];
            nq = a.prev_part_off[s + 1] - q0;
        }
        if (np == 0 && nq == 0) {
            if (tid == 0) {
                if (a.c.topic_moved) a.c.topic_moved[t] = 0;
                if (a.topic_added) a.topic_added[t] = 0;
                if (a.topic_removed) a.topic_removed[t] = 0;
            }
            continue;
        }
        if ((np > a.cap || nq > a.cap) && a.skip_large) continue;
        if (np < 0 || nq < 0 || np > a.cap || nq > a.cap || p0 < 0 || p0 + np > a.c.n_partitions || q0 < 0 ||
            q0 + nq > a.n_prev_partitions) {     // over the hint, or offsets that leave the arrays
            bad |= kStatusShape;
            continue;
        }
        const int bits = nq > 0 ? 32 - __builtin_clz((uint32_t)(2 * nq - 1)) : 0;      // 2^bits >= 2 nq: at most half full
        const int n_slots = nq > 0 ? 1 << bits : 0;
        counts = both_counts + 4 * (pairs_done++ & 1);
        for (int i = tid; i < n_slots; i += kMovesThreads) table[i] = 0;
        if (tid == 0) counts[0] = counts[1] = counts[2] = 0;
        __syncthreads();
        for (int64_t i = tid; i < nq; i += kMovesThreads) bad |= insert_entry<kScope>(a.c, table, bits, q0 + i);
        __syncthreads();
        uint32_t moved = 0, added = 0, removed = 0;
        uint32_t missed_mask = 0;                // bit k: this thread's k-th entry of the segment has no previous entry
        for (int64_t i = tid, k = 0; i < np; i += kMovesThreads, ++k) {
            bool missed;
            bad |= lookup_entry<kScope, BINS, false>(a.c, table, bits, p0 + i, mine, &moved, &added, &missed);
            if (missed) missed_mask |= 1u << k;
        }
        __syncthreads();
        for (int i = tid; i < n_slots; i += kMovesThreads) sweep_slot<BINS>(a.c, table[i], mine, &removed);
        moved = wave_sum_u32(moved);
        added = wave_sum_u32(added);
        removed = wave_sum_u32(removed);
        if ((tid & (kWave - 1)) == 0) {
            if (moved) __hip_atomic_fetch_add(counts + 0, moved, __ATOMIC_RELAXED, kScope);
            if (added) __hip_atomic_fetch_add(counts + 1, added, __ATOMIC_RELAXED, kScope);
            if (removed) __hip_atomic_fetch_add(counts + 2, removed, __ATOMIC_RELAXED, kScope);
        }
        __syncthreads();                         // (every sweep has read the table before the next clear)
        const uint32_t n_added = counts[1];      // workgroup-uniform
        if (n_added > 0) {                       // the added ids among themselves: a duplicate meets its twin on the insert
            const int bits2 = 32 - __builtin_clz(2 * n_added - 1);              // n_added <= np <= cap: within the allocation
            for (int i = tid; i < (1 << bits2); i += kMovesThreads) table[i] = 0;
            __syncthreads();
            for (int k = 0; missed_mask >> k; ++k)
                if ((missed_mask >> k) & 1)
                    bad |= table_insert<kScope>(table, bits2, __builtin_nontemporal_load(a.c.out_partition + p0 + tid + k * kMovesThreads), 0);
            __syncthreads();                     // (before the next pair's clear)
        }
        if (tid == 0) {
            const uint32_t m = counts[0], ad = n_added, rm = counts[2];
            if (a.c.topic_moved) a.c.topic_moved[t] = (int64_t)m;
            if (a.topic_added) a.topic_added[t] = (int64_t)ad;
            if (a.topic_removed) a.topic_removed[t] = (int64_t)rm;
            total[0] += m;
            total[1] += ad;
            total[2] += rm;
        }
    }
    if (tid == 0) {
        if (total[0] && a.c.moved) global_add(a.c.moved, total[0]);
        if (total[1] && a.added) global_add(a.added, total[1]);
        if (total[2] && a.removed) global_add(a.removed, total[2]);
    }
    if (BINS) {
        __syncthreads();
        flush_bins(a, bins, tid);
    }
    if (bad) atomicOr(a.status, bad);
}

// Global form, one launch per PHASE.  Workgroup steps of kMovesChunk items (previous entries, current entries, slots), numbered
// through all pairs of the list; a workgroup finds a step's pair by bisection of chunk0[PHASE] (a pair without steps in the
// phase shares its chunk0 with the next one, and the bisection lands behind it).
template <int PHASE, bool BINS>
__global__ __launch_bounds__(kMovesThreads) void moves_layouts_global_kernel(LayoutsArgs a) {
    extern __shared__ uint64_t layouts_lds[];
    constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
    const int tid = (int)threadIdx.x;
    uint32_t* bins = reinterpret_cast<uint32_t*>(layouts_lds);
    uint32_t* mine = bins + (size_t)(tid & (a.tables - 1)) * a.stride;
    if (PHASE != kInsert && BINS) {
        clear_bins(a, bins, tid);
        __syncthreads();
    }
    uint32_t bad = 0;
    uint64_t total[2] = {0, 0};                  // lookup: moved, added; sweep: removed
    for (int64_t chunk = blockIdx.x; chunk < a.n_chunks[PHASE]; chunk += gridDim.x) {
        int lo = 0, hi = a.n_big;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.big[mid].chunk0[PHASE] <= chunk) lo = mid;
            else hi = mid;
        }
        const LayoutsBig b = a.big[lo];
        uint64_t* table = a.table + b.slot0;
        const int64_t n_items = PHASE == kInsert ? b.n_prev : PHASE == kLookup ? b.n_part : (int64_t)1 << b.bits;
        const int64_t i0 = (chunk - b.chunk0[PHASE]) * kMovesChunk;
        uint32_t n0 = 0, n1 = 0;
        bool missed;
#pragma unroll
        for (int k = 0; k < kMovesChunk / kMovesThreads; ++k) {
            const int64_t i = i0 + k * kMovesThreads + tid;
            if (i >= n_items) continue;
            if (PHASE == kInsert) bad |= insert_entry<kScope>(a.c, table, b.bits, b.q0 + i);
            else if (PHASE == kLookup) bad |= lookup_entry<kScope, BINS, true>(a.c, table, b.bits, b.p0 + i, mine, &n0, &n1, &missed);
            else sweep_slot<BINS>(a.c, table[i], mine, &n0);
        }
        if (PHASE != kInsert) {                  // the topic counts were zeroed on the stream before
            n0 = wave_sum_u32(n0);
            n1 = wave_sum_u32(n1);
            if ((tid & (kWave - 1)) == 0) {
                int64_t* topic0 = PHASE == kLookup ? a.c.topic_moved : a.topic_removed;
                if (n0 && topic0) global_add(topic0 + b.topic, n0);
                if (n1 && a.topic_added) global_add(a.topic_added + b.topic, n1);
                total[0] += n0;
                total[1] += n1;
            }
        }
    }
    if (PHASE != kInsert) {
        int64_t* all0 = PHASE == kLookup ? a.c.moved : a.removed;
        if (total[0] && all0) global_add(all0, total[0]);
        if (total[1] && a.added) global_add(a.added, total[1]);
        if (BINS) {
            __syncthreads();
            flush_bins(a, bins, tid);
        }
    }
    if (bad) atomicOr(a.status, bad);
}

// a phase without steps launches nothing
template <int PHASE, bool BINS>
hipError_t launch_phase(const LayoutsArgs& a, size_t lds, hipStream_t stream) {
    return launch_resident<moves_layouts_global_kernel<PHASE, BINS>>(a.n_chunks[PHASE], kMovesThreads, lds, stream, a);
}

}  // namespace

hipError_t assignment_moves_layouts_launch(MovesScratch& s, const MovesLayoutsCall& c, const int64_t* h_part_off,
                                           const int64_t* h_prev_part_off, const int32_t* h_prev_topic, uint32_t* status,
                                           hipStream_t stream) {
    hipError_t e;
    const int64_t T = c.c.n_topics, N = c.c.n_partitions, NP = c.n_prev_partitions, M = c.c.n_members;
    const bool global_form = c.c.max_partitions_per_topic > kMovesLdsMaxPartitions;
    const bool work = T > 0 && (N > 0 || NP > 0);
    if (c.c.member_gained && M && (e = hipMemsetAsync(c.c.member_gained, 0, (size_t)M * 8, stream)) != hipSuccess) return e;
    if (c.c.member_lost && M && (e = hipMemsetAsync(c.c.member_lost, 0, (size_t)M * 8, stream)) != hipSuccess) return e;
    for (int64_t* total : {c.c.moved, c.added, c.removed})
        if (total && (e = hipMemsetAsync(total, 0, 8, stream)) != hipSuccess) return e;
    // per topic: a plain store from the LDS form; the global form adds to it, and a call without entries launches nothing
    if (T > 0 && (global_form || !work))
        for (int64_t* per_topic : {c.c.topic_moved, c.topic_added, c.topic_removed})
            if (per_topic && (e = hipMemsetAsync(per_topic, 0, (size_t)T * 8, stream)) != hipSuccess) return e;
    if (!work) return hipSuccess;

    LayoutsArgs a{};
    a.c = c.c;
    a.n_prev_topics = c.n_prev_topics;
    a.n_prev_partitions = NP;
    a.prev_part_off = c.prev_part_off;
    a.prev_topic = c.prev_topic;
    a.topic_added = c.topic_added;
    a.topic_removed = c.topic_removed;
    a.added = c.added;
    a.removed = c.removed;
    a.status = status;
    a.tables = a.stride = 1;
    const bool bins = (c.c.member_gained || c.c.member_lost) && M > 0 && M <= kMovesLdsMaxMembers && N + NP < kMovesMaxBinned;
    size_t bin_bytes = 0;
    if (bins) {
        tables_for(2 * M, kMovesFewBins, kMovesMaxTables, &a.tables, &a.stride);
        bin_bytes = (size_t)a.tables * a.stride * 4;
    }

    if (global_form) {
        // the pairs beyond the LDS form: a region of the table and a run of workgroup steps per phase each
        const auto pair_of = [&](int64_t t, int64_t* q0, int64_t* nq) {
            const int64_t sp = h_prev_topic ? h_prev_topic[t] : t;
            *q0 = sp < 0 ? 0 : h_prev_part_off[sp];
            *nq = sp < 0 ? 0 : h_prev_part_off[sp + 1] - *q0;
        };
        int64_t n_big = 0, q0, nq;
        for (int64_t t = 0; t < T; ++t) {
            pair_of(t, &q0, &nq);
            if (std::max(h_part_off[t + 1] - h_part_off[t], nq) > kMovesLdsMaxPartitions) ++n_big;
        }
        if (n_big > 0) {
            const size_t item_bytes = (size_t)n_big * sizeof(LayoutsBig);
            if ((e = s.list.reserve(item_bytes)) != hipSuccess) return e;
            LayoutsBig* items = static_cast<LayoutsBig*>(s.list.h);
            int64_t slots = 0, j = 0;
            for (int64_t t = 0; t < T; ++t) {
                const int64_t np = h_part_off[t + 1] - h_part_off[t];
                pair_of(t, &q0, &nq);
                if (std::max(np, nq) <= kMovesLdsMaxPartitions) continue;
                LayoutsBig& b = items[j++];
                b.p0 = h_part_off[t];
                b.n_part = np;
                b.q0 = q0;
                b.n_prev = nq;
                b.slot0 = slots;
                b.topic = (int32_t)t;
                b.bits = ceil_log2(2 * (nq + np));          // the previous ids and the current ones that miss (a large pair: > 0)
                const int64_t n_slots = (int64_t)1 << b.bits;
                const int64_t n_items[3] = {nq, np, n_slots};
                for (int ph = 0; ph < 3; ++ph) {
                    b.chunk0[ph] = a.n_chunks[ph];
                    a.n_chunks[ph] += (n_items[ph] + kMovesChunk - 1) / kMovesChunk;
                }
                slots += n_slots;
            }
            if ((e = grow_device(&s.table, &s.table_cap, (size_t)slots * 8)) != hipSuccess) return e;
            if ((e = s.list.upload(item_bytes, stream)) != hipSuccess) return e;
            if (slots && (e = hipMemsetAsync(s.table, 0, (size_t)slots * 8, stream)) != hipSuccess) return e;
            a.table = static_cast<uint64_t*>(s.table);
            a.big = static_cast<const LayoutsBig*>(s.list.d);
            a.n_big = (int32_t)n_big;
        }
    }

    {   // the LDS form: every pair within the limit, and every topic's map entry (pairs of the global form are passed over)
        a.cap = global_form ? kMovesLdsMaxPartitions : std::max<int64_t>(c.c.max_partitions_per_topic, 0);
        a.skip_large = global_form ? 1 : 0;
        a.table_bits = ceil_log2(2 * a.cap);
        const size_t lds = ((size_t)8 << a.table_bits) + bin_bytes + kLayoutsCounterBytes;
        e = bins ? launch_resident_lds<moves_layouts_lds_kernel<true>, kLayoutsMaxLdsBytes>(T, kMovesThreads, lds, stream, a)
                 : launch_resident_lds<moves_layouts_lds_kernel<false>, kLayoutsMaxLdsBytes>(T, kMovesThreads, lds, stream, a);
        if (e != hipSuccess) return e;
    }
    if ((e = launch_phase<kInsert, false>(a, 0, stream)) != hipSuccess) return e;
    e = bins ? launch_phase<kLookup, true>(a, bin_bytes, stream) : launch_phase<kLookup, false>(a, 0, stream);
    if (e != hipSuccess) return e;
    return bins ? launch_phase<kSweep, true>(a, bin_bytes, stream) : launch_phase<kSweep, false>(a, 0, stream);
}

}  // namespace la
