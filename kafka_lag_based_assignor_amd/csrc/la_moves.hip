// la_moves.hip -- who moved between two rebalances (la_assignment_moves_device, lagassign.h).
//
// Nothing in the reference computes it: its assignor is eager, every rebalance sorts each topic by lag again and deals the
// partitions out afresh (Main.java:204-266).  Both assignments come in ASSIGNMENT order (lag descending), which differs between
// the two, so the previous owner of an entry is found by a join on (topic, partition id) -- per topic an open-addressing hash
// table keyed by the id:
//
//     slot (one 64-bit word) = mark << 63 | (previous owner in today's ranks + 2) << 32 | (uint32) id        empty = 0
//
// (owner + 2 >= 1, so no live slot is 0; n_members < 2^30 keeps bit 63 free for the mark.)  INSERT is a 64-bit compare-and-swap
// on an empty slot, walking on from an occupied one -- an equal id on the way is a duplicate.  LOOKUP walks the same chain and
// sets the mark of its hit with an atomic OR: a hit that was marked already is a duplicate in the current assignment.  The
// table is at most half full (2^ceil(log2(2 P)) slots), so a walk always ends at a hit or an empty slot; every walk is bounded
// by the slot count all the same and raises kStatusInternal when it runs out.  No thread ever waits for another.
//
// The ONE probing routine (table_insert / table_lookup, la_join.h) runs in two address spaces:
//   LDS form     topics up to kMovesLdsMaxPartitions.  Persistent workgroups walk topics blockIdx.x, + gridDim.x, ...; per topic:
//                clear the slots the topic needs, insert the previous entries, barrier, look the current entries up, store
//                prev_owner, reduce the moved count, ONE plain store to topic_moved[t].  The table is sized from the call's
//                hint.  Gained / lost go to 32-bit bins beside the table (several copies of them while the members are few: 64
//                lanes on a handful of addresses would serialise), flushed once per workgroup as one 64-bit global atomic per
//                non-zero bin; beyond kMovesLdsMaxMembers they are 64-bit global atomics straight away.
//   global form  topics beyond that, all of a call side by side in one table in device memory (a region per topic, listed by
//                the host from h_part_off): one launch inserts, one looks up -- the order between the two is the launch
//                boundary.  The table is zeroed by a memset on the stream in front of them.
// Nothing is stored through a rank or an id: a rank out of range, a duplicate and a missing id raise kStatusMoves and the entry
// is skipped.  Every access is one element wide, so a view that starts at any element of a larger buffer takes the same path.
#include "la_moves_shared.h"

namespace la {

namespace {

// table + one copy of the bins (stride made odd) + the topic's counter: what the LDS form asks for at most
constexpr size_t kMovesMaxLdsBytes = 16 * (size_t)kMovesLdsMaxPartitions + 4 * (2 * (size_t)kMovesLdsMaxMembers + 1) + 8;
static_assert(kMovesMaxLdsBytes <= 160 * 1024, "table + bins fit one workgroup's LDS on gfx950");

struct MovesBig {               // one topic of the global form
    int64_t p0, n_part;         // its entries
    int64_t slot0;              // its region of the table
    int64_t chunk0;             // first workgroup step of the topic; the steps of all topics are numbered through
    int32_t topic, bits;        // the region has 1 << bits slots
};

struct MovesArgs {
    MovesCall c;
    uint32_t* status;
    int64_t cap;                // LDS form: partitions a topic may have (the hint, or the limit when larger topics go elsewhere)
    int32_t skip_large;         // topics over `cap` belong to the global form: no error
    int32_t table_bits;         // LDS form: the table has 1 << table_bits slots
    int32_t tables, stride;     // bins: copies (a power of two) and their stride in counters (odd)
    uint64_t* table;            // global form
    const MovesBig* big;
    int32_t n_big;
    int64_t n_chunks;
};

// one current entry: its previous owner, prev_owner[i], the gained / lost counts; *moved += 1 when it moved; returns status bits
template <int SCOPE, bool BINS>
__device__ __forceinline__ uint32_t lookup_entry(const MovesCall& c, uint64_t* table, int bits, int64_t i, uint32_t* mine,
                                                 uint32_t* moved) {
    const int32_t id = __builtin_nontemporal_load(c.out_partition + i);
    const int32_t cur = __builtin_nontemporal_load(c.out_member_rank + i);
    if (cur < -1 || cur >= c.n_members) return kStatusMoves;
    int32_t q;
    const uint32_t st = table_lookup<SCOPE>(table, bits, id, &q);
    if (st) return st;
    if (c.prev_owner) __builtin_nontemporal_store(q, c.prev_owner + i);
    if (q == cur) return 0;
    ++*moved;
    if (BINS) {
        if (cur >= 0) __hip_atomic_fetch_add(mine + cur, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (q >= 0) __hip_atomic_fetch_add(mine + c.n_members + q, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
        if (cur >= 0 && c.member_gained) global_add(c.member_gained + cur, 1);
        if (q >= 0 && c.member_lost) global_add(c.member_lost + q, 1);
    }
    return 0;
}

// LDS: [table: 1 << table_bits words][bins: tables x stride counters][the topic's moved count]
template <bool BINS>
__global__ __launch_bounds__(kMovesThreads) void moves_lds_kernel(MovesArgs a) {
    extern __shared__ uint64_t moves_lds[];
    constexpr int kScope = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int tid = (int)threadIdx.x;
    uint64_t* table = moves_lds;
    uint32_t* bins = reinterpret_cast<uint32_t*>(moves_lds + ((size_t)1 << a.table_bits));
    uint32_t* topic_count = bins + (BINS ? a.tables * a.stride : 0);
    uint32_t* mine = bins + (size_t)(tid & (a.tables - 1)) * a.stride;
    if (BINS) clear_bins(a, bins, tid);          // (the first topic's barriers order it before the first add; so does the flush's)
    uint32_t bad = 0;
    uint64_t total = 0;                          // thread 0: moved entries of this workgroup's topics
    for (int64_t t = blockIdx.x; t < a.c.n_topics; t += gridDim.x) {
        const int64_t p0 = a.c.part_off[t], np = a.c.part_off[t + 1] - p0;      // workgroup-uniform, as all that follows from it
        if (np == 0) {
            if (tid == 0 && a.c.topic_moved) a.c.topic_moved[t] = 0;
            continue;
        }
        if (np > a.cap && a.skip_large) continue;
        if (np < 0 || np > a.cap || p0 < 0 || p0 + np > a.c.n_partitions) {     // over the hint, or offsets that leave the arrays
            bad |= kStatusShape;
            continue;
        }
        const int bits = 32 - __builtin_clz((uint32_t)(2 * np - 1));           // 2^bits >= 2 np: at most half full
        for (int i = tid; i < (1 << bits); i += kMovesThreads) table[i] = 0;
        if (tid == 0) *topic_count = 0;
        __syncthreads();
        for (int64_t i = tid; i < np; i += kMovesThreads) bad |= insert_entry<kScope>(a.c, table, bits, p0 + i);
        __syncthreads();
        uint32_t moved = 0;
        for (int64_t i = tid; i < np; i += kMovesThreads) bad |= lookup_entry<kScope, BINS>(a.c, table, bits, p0 + i, mine, &moved);
        moved = wave_sum_u32(moved);
        if ((tid & (kWave - 1)) == 0 && moved) __hip_atomic_fetch_add(topic_count, moved, __ATOMIC_RELAXED, kScope);
        __syncthreads();
        if (tid == 0) {                          // (thread 0 also zeroes the counter for the next topic: no barrier in between)
            const uint32_t m = *topic_count;
            if (a.c.topic_moved) a.c.topic_moved[t] = (int64_t)m;
            total += m;
        }
    }
    if (tid == 0 && total && a.c.moved) global_add(a.c.moved, total);
    if (BINS) {
        __syncthreads();
        flush_bins(a, bins, tid);
    }
    if (bad) atomicOr(a.status, bad);
}

// Global form.  PHASE 0 inserts the previous entries, PHASE 1 looks the current ones up.  Workgroup steps of kMovesChunk entries,
// numbered through all topics of the list; a workgroup finds a step's topic by bisection of chunk0.
template <int PHASE, bool BINS>
__global__ __launch_bounds__(kMovesThreads) void moves_global_kernel(MovesArgs a) {
    extern __shared__ uint64_t moves_lds[];
    constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
    const int tid = (int)threadIdx.x;
    uint32_t* bins = reinterpret_cast<uint32_t*>(moves_lds);
    uint32_t* mine = bins + (size_t)(tid & (a.tables - 1)) * a.stride;
    if (PHASE == 1 && BINS) {
        clear_bins(a, bins, tid);
        __syncthreads();
    }
    uint32_t bad = 0;
    uint64_t total = 0;
    for (int64_t chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
        int lo = 0, hi = a.n_big;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.big[mid].chunk0 <= chunk) lo = mid;
            else hi = mid;
        }
        const MovesBig b = a.big[lo];
        uint64_t* table = a.table + b.slot0;
        const int64_t i0 = (chunk - b.chunk0) * kMovesChunk;
        uint32_t moved = 0;
#pragma unroll
        for (int k = 0; k < kMovesChunk / kMovesThreads; ++k) {
            const int64_t i = i0 + k * kMovesThreads + tid;
            if (i >= b.n_part) continue;
            if (PHASE == 0) bad |= insert_entry<kScope>(a.c, table, b.bits, b.p0 + i);
            else bad |= lookup_entry<kScope, BINS>(a.c, table, b.bits, b.p0 + i, mine, &moved);
        }
        if (PHASE == 1) {
            moved = wave_sum_u32(moved);
            if ((tid & (kWave - 1)) == 0 && moved) {
                if (a.c.topic_moved) global_add(a.c.topic_moved + b.topic, moved);      // zeroed on the stream before
                total += moved;
            }
        }
    }
    if (PHASE == 1) {
        if (total && a.c.moved) global_add(a.c.moved, total);
        if (BINS) {
            __syncthreads();
            flush_bins(a, bins, tid);
        }
    }
    if (bad) atomicOr(a.status, bad);
}

}  // namespace

void moves_scratch_release(MovesScratch& s) {
    s.list.release();
    if (s.table) (void)hipFree(s.table);
    s = MovesScratch{};
}

hipError_t assignment_moves_launch(MovesScratch& s, const MovesCall& c, const int64_t* h_part_off, uint32_t* status,
                                   hipStream_t stream) {
    hipError_t e;
    const int64_t T = c.n_topics, N = c.n_partitions, M = c.n_members;
    const bool global_form = c.max_partitions_per_topic > kMovesLdsMaxPartitions;
    if (c.member_gained && M && (e = hipMemsetAsync(c.member_gained, 0, (size_t)M * 8, stream)) != hipSuccess) return e;
    if (c.member_lost && M && (e = hipMemsetAsync(c.member_lost, 0, (size_t)M * 8, stream)) != hipSuccess) return e;
    if (c.moved && (e = hipMemsetAsync(c.moved, 0, 8, stream)) != hipSuccess) return e;
    // topic_moved: a plain store per topic from the LDS form; the global form adds to it, and a call without entries launches nothing
    if (c.topic_moved && T > 0 && (global_form || N <= 0) &&
        (e = hipMemsetAsync(c.topic_moved, 0, (size_t)T * 8, stream)) != hipSuccess)
        return e;
    if (T <= 0 || N <= 0) return hipSuccess;

    MovesArgs a{};
    a.c = c;
    a.status = status;
    a.tables = a.stride = 1;
    const bool bins = (c.member_gained || c.member_lost) && M > 0 && M <= kMovesLdsMaxMembers && N < kMovesMaxBinned;
    size_t bin_bytes = 0;
    if (bins) {
        tables_for(2 * M, kMovesFewBins, kMovesMaxTables, &a.tables, &a.stride);
        bin_bytes = (size_t)a.tables * a.stride * 4;
    }

    bool any_small = true;
    if (global_form) {
        // the topics beyond the LDS form: a region of the table and a run of workgroup steps each
        any_small = false;
        int64_t n_big = 0;
        for (int64_t t = 0; t < T; ++t) {
            const int64_t np = h_part_off[t + 1] - h_part_off[t];
            if (np > kMovesLdsMaxPartitions) ++n_big;
            else if (np > 0) any_small = true;
        }
        if (n_big > 0) {
            if (n_big > 0x7FFFFFFF) return hipErrorInvalidValue;
            const size_t item_bytes = (size_t)n_big * sizeof(MovesBig);
            if ((e = s.list.reserve(item_bytes)) != hipSuccess) return e;
            MovesBig* items = static_cast<MovesBig*>(s.list.h);
            int64_t slots = 0, chunks = 0, j = 0;
            for (int64_t t = 0; t < T; ++t) {
                const int64_t np = h_part_off[t + 1] - h_part_off[t];
                if (np <= kMovesLdsMaxPartitions) continue;
                MovesBig& b = items[j++];
                b.p0 = h_part_off[t];
                b.n_part = np;
                b.slot0 = slots;
                b.chunk0 = chunks;
                b.topic = (int32_t)t;
                b.bits = ceil_log2(2 * np);
                slots += (int64_t)1 << b.bits;
                chunks += (np + kMovesChunk - 1) / kMovesChunk;
            }
            if ((e = grow_device(&s.table, &s.table_cap, (size_t)slots * 8)) != hipSuccess) return e;
            if ((e = s.list.upload(item_bytes, stream)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(s.table, 0, (size_t)slots * 8, stream)) != hipSuccess) return e;
            a.table = static_cast<uint64_t*>(s.table);
            a.big = static_cast<const MovesBig*>(s.list.d);
            a.n_big = (int32_t)n_big;
            a.n_chunks = chunks;
        }
    }

    if (any_small) {
        a.cap = global_form ? kMovesLdsMaxPartitions : std::max<int64_t>(c.max_partitions_per_topic, 0);
        a.skip_large = global_form ? 1 : 0;
        a.table_bits = ceil_log2(2 * a.cap);
        const size_t lds = ((size_t)8 << a.table_bits) + bin_bytes + 8;
        e = bins ? launch_resident_lds<moves_lds_kernel<true>, kMovesMaxLdsBytes>(T, kMovesThreads, lds, stream, a)
                 : launch_resident_lds<moves_lds_kernel<false>, kMovesMaxLdsBytes>(T, kMovesThreads, lds, stream, a);
        if (e != hipSuccess) return e;
    }
    if (a.n_big > 0) {
        if ((e = launch_resident<moves_global_kernel<0, false>>(a.n_chunks, kMovesThreads, 0, stream, a)) != hipSuccess) return e;
        e = bins ? launch_resident<moves_global_kernel<1, true>>(a.n_chunks, kMovesThreads, bin_bytes, stream, a)
                 : launch_resident<moves_global_kernel<1, false>>(a.n_chunks, kMovesThreads, 0, stream, a);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace la
