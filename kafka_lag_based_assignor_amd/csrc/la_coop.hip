// la_coop.hip -- the cooperative form of a rebalance (la_cooperative_adjust_device, lagassign.h): the target assignment with every
// partition that changes hands between two live members withheld for this round.
//
// Nothing in the reference computes it: its protocol is eager, every rebalance revokes everything (Main.java:204-266).  The
// previous owners come as Kafka gives them -- each member's owned list, member by member, across topics -- so the entries of one
// topic are scattered over the whole input and the join is ONE open-addressing table over the call, keyed by (topic, id):
//
//     key slot (one 64-bit word) = (uint32)(topic + 1) << 32 | (uint32) id        empty = 0
//     payload slot (32 bits)     = the claiming member, stored by the thread whose compare-and-swap took the key slot
//
// (topic + 1 >= 1, so no live key is 0 -- not (topic 0, id 0) either.)  A key of topic plus id fills the 64-bit word, hence the
// payload array beside the key array: 12 B per slot, no limit on topics, ids or members beyond those of the call.  The table has
// 2^ceil(log2(2 n_owned)) slots, so it is at most half full and a walk ends at a hit or an empty slot; every walk is bounded by
// the slot count all the same and raises kStatusInternal when it runs out.  No thread ever waits for another: the order between
// insert and lookup is the launch boundary (which also makes the payloads visible), and the keys are zeroed by a memset on the
// stream in front of the insert launch.
//
//   launch 1 (insert)  workgroup steps of kMovesChunk positions of the owned arrays.  A position inside [off[0], off[M]) finds its
//                      member by bisection of the owned offsets (in LDS up to kMovesLdsMaxMembers members); an equal key met
//                      on the way is a duplicate claim.  Counts what it claimed (topic -1 entries included) into summary[4].
//   launch 2 (lookup)  workgroup steps over today's entries.  The step's range of topics comes from two bisections of part_off
//                      per workgroup step; a thread only settles its entry inside that range (a handful of topics).  Per-member
//                      counts go to 32-bit LDS bins flushed once per workgroup (64-bit global atomics beyond
//                      kMovesLdsMaxMembers); the hits are taken off summary[4], which leaves the stale entries: no sweep.
// Positions come from the loop counters alone, never from an offset: offsets that do not ascend inside the arrays raise
// kStatusShape and at worst name a wrong member or topic, both inside [0, M) / [0, T).  Nothing is stored or read through a rank
// or a topic out of range: such an entry raises kStatusCoop and is skipped.
#include "la_moves_shared.h"
#include "la_coop.h"

namespace la {

namespace {

constexpr size_t kCoopMaxBinBytes = 4 * (4 * (size_t)kMovesLdsMaxMembers + 1);      // one copy of the widest bins (stride made odd)
static_assert(kCoopMaxBinBytes <= 160 * 1024, "the bins fit one workgroup's LDS on gfx950");
static_assert(8 * ((size_t)kMovesLdsMaxMembers + 1) <= 64 * 1024, "the owned offsets fit the LDS a kernel gets without asking");

struct CoopArgs {
    CoopCall c;
    uint32_t* status;
    uint64_t* keys;             // null: nobody owns anything
    uint32_t* owners;
    int32_t bits;               // the table has 1 << bits slots
    int32_t tables, stride;     // bins: copies (a power of two) and their stride in counters (odd)
    int64_t* claimed;           // insert: where the count of claims goes (the adjust call: summary + 4); null: nowhere
    int64_t n_chunks;           // workgroup steps of the launch
};

// LDS (LDS_OFF): the owned offsets, M + 1 words
template <bool LDS_OFF>
__global__ __launch_bounds__(kMovesThreads) void coop_insert_kernel(CoopArgs a) {
    extern __shared__ uint64_t coop_lds[];
    const int tid = (int)threadIdx.x;
    const int64_t M = a.c.n_members, n = a.c.n_owned, T = a.c.n_topics;
    const uint64_t mask = (1ull << a.bits) - 1;
    uint32_t bad = 0;
    // the offsets ascend inside [0, n_owned]: every workgroup takes its share of the check
    for (int64_t r = (int64_t)blockIdx.x * kMovesThreads + tid; r <= M; r += (int64_t)gridDim.x * kMovesThreads) {
        const int64_t o = a.c.owned_off[r];
        if (o < 0 || o > n || (r < M && a.c.owned_off[r + 1] < o)) bad |= kStatusShape;
    }
    const int64_t* off = a.c.owned_off;
    if (LDS_OFF) {
        int64_t* l = reinterpret_cast<int64_t*>(coop_lds);
        for (int64_t r = tid; r <= M; r += kMovesThreads) l[r] = a.c.owned_off[r];
        __syncthreads();
        off = l;
    }
    const int64_t first = off[0], last = off[M];
    uint64_t claimed = 0;
    for (int64_t chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
#pragma unroll
        for (int k = 0; k < kMovesChunk / kMovesThreads; ++k) {
            const int64_t j = chunk * kMovesChunk + k * kMovesThreads + tid;
            if (j >= n || j < first || j >= last) continue;          // the head and the tail belong to nobody: not looked at
            const int32_t topic = __builtin_nontemporal_load(a.c.owned_topic + j);
            if (topic == -1) { ++claimed; continue; }                // a topic the host could not map: stale
            if (topic < -1 || topic >= T) { bad |= kStatusCoop; continue; }
            const int32_t id = __builtin_nontemporal_load(a.c.owned_partition + j);
            const uint32_t r = (uint32_t)last_not_above(off, 0, M, j);      // (first <= j < last: M >= 1)
            const uint64_t key = coop_key(topic, id);
            uint64_t h = coop_first_slot(key, a.bits);
            uint32_t st = kStatusInternal;
            for (uint64_t w = 0; w <= mask; ++w) {
                unsigned long long seen = 0;
                if (__hip_atomic_compare_exchange_strong((unsigned long long*)(a.keys + h), &seen, (unsigned long long)key,
                                                         __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    a.owners[h] = r;
                    st = 0;
                    break;
                }
                if (seen == key) { st = kStatusCoop; break; }        // claimed twice
                h = (h + 1) & mask;
            }
            if (st) bad |= st;
            else ++claimed;
        }
    }
    claimed = wave_sum_u64(claimed);
    if ((tid & (kWave - 1)) == 0 && claimed && a.claimed) global_add(a.claimed, claimed);
    if (bad) atomicOr(a.status, bad);
}

// the member that claimed (topic, id), or -1; *st |= kStatusInternal when the walk ran out
__device__ __forceinline__ int32_t coop_lookup(const CoopArgs& a, int32_t topic, int32_t id, uint32_t* st) {
    return coop_table_lookup(CoopTable{a.keys, a.owners, a.bits}, topic, id, st);
}

// the workgroup's bins into the outputs: one 64-bit global atomic per non-zero bin (behind a barrier)
__device__ __forceinline__ void coop_flush_bins(const CoopArgs& a, const uint32_t* bins, int tid) {
    const uint32_t m = (uint32_t)a.c.n_members;
    int64_t* const out[4] = {a.c.member_kept, a.c.member_fresh, a.c.member_pending, a.c.member_release};
    for (int w = 0; w < 4; ++w) {
        if (!out[w]) continue;
        for (uint32_t r = (uint32_t)tid; r < m; r += kMovesThreads) {
            uint64_t s = 0;
            for (int t = 0; t < a.tables; ++t) s += bins[(size_t)t * a.stride + (size_t)w * m + r];
            if (s) global_add(out[w] + r, s);
        }
    }
}

// LDS (BINS): tables x stride counters -- per copy [kept: M][fresh: M][pending: M][release: M]
template <bool BINS>
__global__ __launch_bounds__(kMovesThreads) void coop_lookup_kernel(CoopArgs a) {
    extern __shared__ uint64_t coop_lds[];
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1);
    const int64_t M = a.c.n_members, N = a.c.n_partitions, T = a.c.n_topics;
    uint32_t* bins = reinterpret_cast<uint32_t*>(coop_lds);
    uint32_t* mine = bins + (size_t)(tid & (a.tables - 1)) * a.stride;
    if (BINS) {
        clear_bins(a, bins, tid);
        __syncthreads();
    }
    uint32_t bad = 0;
    // part_off ascends from 0 to N: every workgroup takes its share of the check
    for (int64_t t = (int64_t)blockIdx.x * kMovesThreads + tid; t <= T; t += (int64_t)gridDim.x * kMovesThreads) {
        const int64_t o = a.c.part_off[t];
        if (o < 0 || o > N || (t == 0 && o != 0) || (t == T && o != N) || (t < T && a.c.part_off[t + 1] < o)) bad |= kStatusShape;
    }
    uint64_t kept = 0, fresh = 0, withheld = 0, dropped = 0;
    for (int64_t chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
        // the topics of this step: workgroup-uniform
        const int64_t i0 = chunk * kMovesChunk, i1 = (i0 + kMovesChunk < N ? i0 + kMovesChunk : N) - 1;
        const int64_t t_lo = last_not_above(a.c.part_off, 0, T, i0);
        const int64_t t_hi = last_not_above(a.c.part_off, t_lo, T, i1);
#pragma unroll
        for (int k = 0; k < kMovesChunk / kMovesThreads; ++k) {
            const int64_t i = i0 + k * kMovesThreads + tid;
            bool wh = false;
            int32_t topic = 0;
            if (i < N) {
                const int32_t id = __builtin_nontemporal_load(a.c.out_partition + i);
                const int32_t cur = __builtin_nontemporal_load(a.c.out_member_rank + i);
                if (cur < -1 || cur >= M) {
                    bad |= kStatusCoop;
                } else {
                    topic = (int32_t)last_not_above(a.c.part_off, t_lo, t_hi + 1, i);
                    const int32_t q = coop_lookup(a, topic, id, &bad);
                    if (a.c.prev_owner) __builtin_nontemporal_store(q, a.c.prev_owner + i);
                    if (a.c.coop_rank) __builtin_nontemporal_store((q == -1 || q == cur) ? cur : -1, a.c.coop_rank + i);
                    int which = -1;                                  // of the member arrays, by `cur`
                    if (cur >= 0) {
                        if (q == cur) { ++kept; which = 0; }
                        else if (q < 0) { ++fresh; which = 1; }
                        else { ++withheld; which = 2; wh = true; }
                    } else if (q >= 0) {
                        ++dropped;
                    }
                    const bool release = q >= 0 && q != cur;
                    if (BINS) {
                        if (which >= 0) __hip_atomic_fetch_add(mine + (size_t)which * M + cur, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (release) __hip_atomic_fetch_add(mine + (size_t)3 * M + q, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else {
                        int64_t* const by_cur = which == 0 ? a.c.member_kept : which == 1 ? a.c.member_fresh : a.c.member_pending;
                        if (which >= 0 && by_cur) global_add(by_cur + cur, 1);
                        if (release && a.c.member_release) global_add(a.c.member_release + q, 1);
                    }
                }
            }
            if (a.c.topic_withheld) {
                // neighbours mostly share a topic: one atomic per wavefront then, one per entry where they do not
                const uint64_t m = __ballot(wh);
                if (m) {
                    const int head = __ffsll((long long)m) - 1;
                    const int32_t t0 = __shfl(topic, head);
                    if (__ballot(wh && topic != t0) == 0) {
                        if (lane == head) global_add(a.c.topic_withheld + t0, (uint64_t)__popcll(m));
                    } else if (wh) {
                        global_add(a.c.topic_withheld + topic, 1);
                    }
                }
            }
        }
    }
    if (a.c.summary) {
        kept = wave_sum_u64(kept);
        fresh = wave_sum_u64(fresh);
        withheld = wave_sum_u64(withheld);
        dropped = wave_sum_u64(dropped);
        if (lane == 0) {
            if (kept) global_add(a.c.summary + 0, kept);
            if (fresh) global_add(a.c.summary + 1, fresh);
            if (withheld) global_add(a.c.summary + 2, withheld);
            if (dropped) global_add(a.c.summary + 3, dropped);
            const uint64_t hits = kept + withheld + dropped;
            if (hits) global_add(a.c.summary + 4, (uint64_t)0 - hits);      // claimed - hits = stale
            if (withheld + dropped)
                __hip_atomic_fetch_or((unsigned long long*)(a.c.summary + 5), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (BINS) {
        __syncthreads();
        coop_flush_bins(a, bins, tid);
    }
    if (bad) atomicOr(a.status, bad);
}

}  // namespace

void coop_scratch_release(CoopScratch& s) {
    if (s.table) (void)hipFree(s.table);
    if (s.ranks) (void)hipFree(s.ranks);
    if (s.prev) (void)hipFree(s.prev);
    if (s.stage_d) (void)hipFree(s.stage_d);
    if (s.stage_h) (void)hipHostFree(s.stage_h);
    s = CoopScratch{};
}

hipError_t coop_table_reserve(CoopScratch& s, int64_t n_owned, CoopTable* out) {
    *out = CoopTable{};
    if (n_owned <= 0) return hipSuccess;
    if (n_owned > kCoopMaxOwned) return hipErrorOutOfMemory;
    out->bits = ceil_log2(2 * n_owned);
    const size_t slots = (size_t)1 << out->bits;
    const hipError_t e = grow_device(&s.table, &s.table_cap, slots * 12);
    if (e != hipSuccess) return e;
    out->keys = static_cast<uint64_t*>(s.table);
    out->owners = reinterpret_cast<uint32_t*>(out->keys + slots);
    return hipSuccess;
}

hipError_t coop_table_insert_launch(const CoopTable& t, const CoopCall& c, int64_t* claimed, uint32_t* status, hipStream_t stream) {
    const int64_t M = c.n_members, n = c.n_owned;
    if (n <= 0) return hipSuccess;
    hipError_t e;
    CoopArgs a{};
    a.c = c;
    a.status = status;
    a.tables = a.stride = 1;
    a.keys = t.keys;
    a.owners = t.owners;
    a.bits = t.bits;
    a.claimed = claimed;
    if ((e = hipMemsetAsync(a.keys, 0, (size_t)8 << a.bits, stream)) != hipSuccess) return e;
    a.n_chunks = (n + kMovesChunk - 1) / kMovesChunk;
    // (the grid also shares the check of the M + 1 offsets: a few owned entries of very many members get workgroups for it)
    const int64_t want = std::max<int64_t>(a.n_chunks, M / kMovesThreads + 1);
    return M <= kMovesLdsMaxMembers ? launch_resident<coop_insert_kernel<true>>(want, kMovesThreads, (size_t)(M + 1) * 8, stream, a)
                                    : launch_resident<coop_insert_kernel<false>>(want, kMovesThreads, 0, stream, a);
}

hipError_t cooperative_adjust_launch(CoopScratch& s, const CoopCall& c, uint32_t* status, hipStream_t stream) {
    hipError_t e;
    const int64_t T = c.n_topics, N = c.n_partitions, M = c.n_members;
    CoopArgs a{};
    a.c = c;
    a.status = status;
    a.tables = a.stride = 1;
    // the table first: when it cannot be had nothing has been enqueued
    CoopTable table{};
    if ((e = coop_table_reserve(s, c.n_owned, &table)) != hipSuccess) return e;
    a.keys = table.keys;
    a.owners = table.owners;
    a.bits = table.bits;
    for (int64_t* p : {c.member_kept, c.member_fresh, c.member_pending, c.member_release})
        if (p && M && (e = hipMemsetAsync(p, 0, (size_t)M * 8, stream)) != hipSuccess) return e;
    if (c.topic_withheld && T && (e = hipMemsetAsync(c.topic_withheld, 0, (size_t)T * 8, stream)) != hipSuccess) return e;
    if (c.summary && (e = hipMemsetAsync(c.summary, 0, 6 * 8, stream)) != hipSuccess) return e;

    if ((e = coop_table_insert_launch(table, c, c.summary ? c.summary + 4 : nullptr, status, stream)) != hipSuccess) return e;
    if (T > 0 && N > 0) {
        a.n_chunks = (N + kMovesChunk - 1) / kMovesChunk;
        const int64_t want = std::max<int64_t>(a.n_chunks, T / kMovesThreads + 1);      // (as above, for the T + 1 part offsets)
        const bool bins = (c.member_kept || c.member_fresh || c.member_pending || c.member_release) && M > 0 &&
                          M <= kMovesLdsMaxMembers && N < kMovesMaxBinned;
        if (!bins) return launch_resident<coop_lookup_kernel<false>>(want, kMovesThreads, 0, stream, a);
        tables_for(4 * M, kMovesFewBins, kMovesMaxTables, &a.tables, &a.stride);
        const size_t lds = (size_t)a.tables * a.stride * 4;
        return launch_resident_lds<coop_lookup_kernel<true>, kCoopMaxBinBytes>(want, kMovesThreads, lds, stream, a);
    }
    return hipSuccess;
}

}  // namespace la
