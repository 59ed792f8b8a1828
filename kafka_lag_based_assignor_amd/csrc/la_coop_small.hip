// la_coop_small.hip -- the cooperative round in one call (la_cooperative_round_device, lagassign.h): the adjusted assignment of
// la_coop.hip AND every member's list of it.
//
// What a group leader sends is a few hundred to a few thousand partitions.  For that the two-launch form of la_coop.hip pays a
// growable table in device memory, up to seven memsets and two launches, and the lists cost a third launch behind them.  Within
// the four limits of la_coop.h everything the round needs fits ONE workgroup's LDS, so the round is ONE launch of 1 024 threads
// whose phases are separated by __syncthreads() alone -- no memset (the workgroup writes every counting output in full, zeros
// included), no allocation, nothing in device memory beside the caller's arrays:
//
//   stage    every global input is read once, coalesced, all loads of a thread back to back: the target's ids and ranks, the
//            T + 1 part offsets and the M + 1 owned offsets into LDS, the owned entries into registers (thread k holds the owned
//            positions k and k + 1 024 and is the one that inserts them).  Both offset arrays are checked from their LDS copies
//            (kStatusShape).  The topic of every target entry: +1 at every topic's first position, an inclusive scan -- the form
//            of group_small_body_staged.  Positions come from the loop counters alone.
//   insert   coop_key / coop_first_slot of la_coop.h into an LDS key array (64-bit compare-and-swap) with the payload array
//            beside it, 2^ceil(log2(2 n_owned)) slots; the member of an owned position by bisection of the offsets in LDS.
//            Every walk is bounded by the slot count (kStatusInternal); an equal key met on the way is a duplicate claim
//            (kStatusCoop).
//   lookup   every entry is KEPT, FRESH, WITHHELD, DROPPED or IDLE; prev_owner / coop_rank go out where they are wanted, the
//            adjusted rank stays in LDS (the lists need it whether the caller wants it or not); per-member, per-topic and summary
//            counts are 32-bit LDS counters (at most 2 048 entries each), written out in full afterwards.
//   lists    group_small_body_staged (la_group_small.h) on the adjusted ranks, the ids and the part offsets AS THEY LIE IN LDS;
//            its seven arrays and its cursors reuse the LDS of the table, the owned offsets and the counters.  Its order is the
//            one it has: chunks in order by in-order returning LDS atomics, no spin, no wait on another thread.
//
// Any other call -- or one with LA_COOP_FORCE_TABLE -- is cooperative_adjust_launch followed by group_by_member_launch.
//
// The kernel has a second, FINISHING form (kFinish: la_assign_batch_cooperative, fused): the last launch of a
// zero-copy host call.  The target comes from device memory, the offsets, the owned arrays and every output lie in the call's
// mapped staging buffer, the target is handed on to the host from the stage phase where it is wanted, and the launch ends with
// `done | status` in the word the calling thread spins on.  kFinish == false is the kernel as it was.
#include "la_coop.h"

#include <type_traits>

namespace la {

namespace {

constexpr int NT = kCoopSmallThreads;
constexpr int kSlotsMax = 2 * kCoopSmallOwned;                       // 2^ceil(log2(2 n_owned)) at the limit
static_assert((kCoopSmallOwned & (kCoopSmallOwned - 1)) == 0, "twice the limit is the largest table");
static_assert(kCoopSmallOwned % NT == 0, "a thread holds n_owned / threads owned entries in registers");
static_assert(kCoopSmallEntries <= kSmallGroupN, "group_small_body_staged scans the topic starts of kSmallGroupN entries");
static_assert(kCoopSmallMembers + 2 <= kTailGroupM && kTailGroupM % NT == 0, "the list builder's groups: members, nobody, the clamp");
static_assert(kCoopSmallMembers + 1 < (1 << (kSmallGroupBits + 1)), "a group id fits the ballots of the list builder");

constexpr size_t up8(size_t x) { return (x + 7) & ~(size_t)7; }

// ---- LDS, in bytes.  A: what lives from the stage to the lists.  B: stage to the counters' flush.  C: the lists, over B. ----
constexpr size_t kOffPartOff = 0;                                                          // int64 [T + 1]
constexpr size_t kOffPid = up8(kOffPartOff + 8 * ((size_t)kCoopSmallTopics + 1));          // int32 [N]  the target's ids
constexpr size_t kOffRank = kOffPid + 4 * (size_t)kCoopSmallEntries;                       // int32 [N]  target rank, then adjusted rank
constexpr size_t kOffMisc = kOffRank + 4 * (size_t)kCoopSmallEntries;                      // uint32 [64]: sums, status, turn, wsum
constexpr size_t kOffB = up8(kOffMisc + 4 * 64);
constexpr size_t kOffKeys = kOffB;                                                         // uint64 [slots]
constexpr size_t kOffOwners = kOffKeys + 8 * (size_t)kSlotsMax;                            // uint32 [slots]
constexpr size_t kOffOwnedOff = up8(kOffOwners + 4 * (size_t)kSlotsMax);                   // int64 [M + 1]
constexpr size_t kOffCnt = up8(kOffOwnedOff + 8 * ((size_t)kCoopSmallMembers + 1));        // uint32 [4 M]: kept, fresh, pending, release
constexpr size_t kOffWithheld = kOffCnt + 4 * 4 * (size_t)kCoopSmallMembers;               // uint32 [T]
constexpr size_t kOffTopic = kOffWithheld + 4 * (size_t)kCoopSmallTopics;                  // int32 [N]  topic of every entry
constexpr size_t kEndB = kOffTopic + 4 * (size_t)kCoopSmallEntries;
constexpr size_t kOffStart = kOffB;                                                        // uint32 [kTailGroupM]  the lists' cursors
constexpr size_t kOffLists = kOffStart + 4 * (size_t)kTailGroupM;                          // 7 x int32 [N]
constexpr size_t kEndC = kOffLists + 7 * 4 * (size_t)kCoopSmallEntries;
constexpr size_t kCoopSmallLdsBytes = kEndB > kEndC ? kEndB : kEndC;
static_assert(kEndB <= 160 * 1024, "stage, insert and lookup fit one workgroup's LDS on gfx950");
static_assert(kEndC <= 160 * 1024, "the lists fit one workgroup's LDS on gfx950");
static_assert(kOffKeys % 8 == 0 && kOffOwnedOff % 8 == 0 && kOffPartOff % 8 == 0, "64-bit words on 8-byte boundaries");
static_assert(kOffStart >= kOffMisc + 4 * 64, "the lists leave the ids, the adjusted ranks and the part offsets alone");

// words of the misc area
constexpr int kSumKept = 0, kSumFresh = 1, kSumWithheld = 2, kSumDropped = 3, kSumClaimed = 4, kSumBad = 5, kTurn = 6, kWsum = 16;

struct CoopSmallArgs {
    CoopRoundCall r;
    uint32_t* status;
    int32_t bits;               // the table has 1 << bits slots (n_owned > 0)
};

// The finishing form (la_assign_batch_cooperative, fused: la_host.hip, assign_small_zc).  The target lies in device memory, the
// part offsets, the owned arrays and EVERY output in the call's staging buffer -- coherent host memory mapped into the device,
// read and written in place over the link -- and the launch is the call's last: it ends with `done | status` in fin_flag.
struct CoopSmallFinishArgs : CoopSmallArgs {
    int32_t *target_partition, *target_rank;      // [N] in the staging buffer, or both null: the target as the caller wants it
    uint32_t* fin_flag;                            // host word the calling thread spins on
};

template <bool kFinish>
__global__ __launch_bounds__(NT) void coop_round_small_kernel(std::conditional_t<kFinish, CoopSmallFinishArgs, CoopSmallArgs> a) {
    extern __shared__ uint64_t coop_small_lds[];
    char* const lds = reinterpret_cast<char*>(coop_small_lds);
    int64_t* const l_part_off = reinterpret_cast<int64_t*>(lds + kOffPartOff);
    int32_t* const e_pid = reinterpret_cast<int32_t*>(lds + kOffPid);
    int32_t* const e_rank = reinterpret_cast<int32_t*>(lds + kOffRank);
    uint32_t* const misc = reinterpret_cast<uint32_t*>(lds + kOffMisc);
    uint64_t* const keys = reinterpret_cast<uint64_t*>(lds + kOffKeys);
    uint32_t* const owners = reinterpret_cast<uint32_t*>(lds + kOffOwners);
    int64_t* const l_owned_off = reinterpret_cast<int64_t*>(lds + kOffOwnedOff);
    uint32_t* const cnt = reinterpret_cast<uint32_t*>(lds + kOffCnt);
    uint32_t* const held = reinterpret_cast<uint32_t*>(lds + kOffWithheld);
    int32_t* const e_topic = reinterpret_cast<int32_t*>(lds + kOffTopic);

    const CoopCall& c = a.r.c;
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int N = (int)c.n_partitions, n = (int)c.n_owned, M = c.n_members, T = c.n_topics;
    const int Tn = N > 0 ? T : 0;                    // part_off is not looked at by a call without entries (it may be null)
    const int slots = n > 0 ? 1 << a.bits : 0;
    const uint32_t mask = (uint32_t)slots - 1u;
    uint32_t bad = 0;

    // ---- stage: zeros, then every global input once -------------------------------------------------------------------------
    for (int k = tid; k < slots; k += NT) keys[k] = 0;
    for (int k = tid; k < 4 * M; k += NT) cnt[k] = 0;
    for (int k = tid; k < T; k += NT) held[k] = 0;
    for (int k = tid; k < N; k += NT) e_topic[k] = 0;
    if (tid < 8) misc[tid] = 0;
    if constexpr (!kFinish) {
        for (int i = tid; i < N; i += NT) {
            e_pid[i] = c.out_partition[i];
            e_rank[i] = c.out_member_rank[i];
        }
    } else {
        // the target on its way from device memory to LDS: where the caller wants it, it goes to the staging buffer from here,
        // while the thread holds both words (afterwards the adjusted rank overwrites the LDS copy) -- no trip of its own
        for (int i = tid; i < N; i += NT) {
            const int32_t id = c.out_partition[i], rank = c.out_member_rank[i];
            e_pid[i] = id;
            e_rank[i] = rank;
            if (a.target_partition) {
                a.target_partition[i] = id;
                a.target_rank[i] = rank;
            }
        }
    }
    if (Tn > 0)
        for (int t = tid; t <= Tn; t += NT) l_part_off[t] = c.part_off[t];
    constexpr int PERO = kCoopSmallOwned / NT;
    int32_t o_topic[PERO], o_id[PERO];
    if (n > 0) {
        for (int r = tid; r <= M; r += NT) l_owned_off[r] = c.owned_off[r];
#pragma unroll
        for (int u = 0; u < PERO; ++u) {
            const int j = u * NT + tid;
            o_topic[u] = j < n ? c.owned_topic[j] : -1;
            o_id[u] = j < n ? c.owned_partition[j] : 0;
        }
    }
    __syncthreads();
    // both offset arrays, from LDS: part_off ascends from 0 to N, the owned offsets ascend inside [0, n_owned]; topic starts
    for (int t = tid; t <= Tn && Tn > 0; t += NT) {
        const int64_t o = l_part_off[t];
        if (o < 0 || o > N || (t == 0 && o != 0) || (t == Tn && o != N) || (t < Tn && l_part_off[t + 1] < o)) bad |= kStatusShape;
        if (t < Tn && o >= 0 && o < N) atomicAdd(reinterpret_cast<uint32_t*>(&e_topic[o]), 1u);
    }
    if (n > 0)
        for (int r = tid; r <= M; r += NT) {
            const int64_t o = l_owned_off[r];
            if (o < 0 || o > n || (r < M && l_owned_off[r + 1] < o)) bad |= kStatusShape;
        }

    // ---- insert -------------------------------------------------------------------------------------------------------------
    if (n > 0) {
        const int64_t first = l_owned_off[0], last = l_owned_off[M];
        uint32_t claimed = 0;
#pragma unroll
        for (int u = 0; u < PERO; ++u) {
            const int j = u * NT + tid;
            if (j >= n || j < first || j >= last) continue;          // the head and the tail belong to nobody
            const int32_t topic = o_topic[u];
            if (topic == -1) { ++claimed; continue; }                // a topic the host could not map: stale
            if (topic < -1 || topic >= T) { bad |= kStatusCoop; continue; }
            const uint32_t r = (uint32_t)last_not_above(l_owned_off, 0, M, j);      // (first <= j < last: M >= 1)
            const uint64_t key = coop_key(topic, o_id[u]);
            uint32_t h = (uint32_t)coop_first_slot(key, a.bits);
            uint32_t st = kStatusInternal;
            for (int w = 0; w < slots; ++w) {
                unsigned long long seen = 0;
                if (__hip_atomic_compare_exchange_strong((unsigned long long*)(keys + h), &seen, (unsigned long long)key,
                                                         __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                    owners[h] = r;
                    st = 0;
                    break;
                }
                if (seen == key) { st = kStatusCoop; break; }        // claimed twice
                h = (h + 1) & mask;
            }
            if (st) bad |= st;
            else ++claimed;
        }
        claimed = wave_sum_u32(claimed);
        if (lane == 0 && claimed) atomicAdd(&misc[kSumClaimed], claimed);
    }

    // ---- the topic of every entry: an inclusive scan of the topic starts, two consecutive entries per thread ------------------------
    constexpr int PERT = kCoopSmallEntries / NT;
    static_assert(kCoopSmallEntries % NT == 0, "entries over threads");
    __syncthreads();                                                 // (the topic starts are in; so are the table and its payloads)
    {
        uint32_t tv[PERT], run = 0;
#pragma unroll
        for (int r = 0; r < PERT; ++r) {
            const int i = PERT * tid + r;
            tv[r] = i < N ? (uint32_t)e_topic[i] : 0u;
            run += tv[r];
        }
        uint32_t incl = run;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == kWave - 1) misc[kWsum + wave] = incl;
        __syncthreads();
        uint32_t base = incl - run;
        for (int w = 0; w < wave; ++w) base += misc[kWsum + w];
#pragma unroll
        for (int r = 0; r < PERT; ++r) {
            const int i = PERT * tid + r;
            base += tv[r];
            if (i < N) e_topic[i] = (int32_t)base - 1;
        }
    }
    __syncthreads();

    // ---- lookup -------------------------------------------------------------------------------------------------------------
    {
        uint32_t kept = 0, fresh = 0, withheld = 0, dropped = 0;
        for (int i = tid; i < N; i += NT) {
            const int32_t id = e_pid[i], cur = e_rank[i];
            if (cur < -1 || cur >= M) {                              // never stored through; the lists file it under "nobody"
                bad |= kStatusCoop;
                e_rank[i] = -1;
                continue;
            }
            int32_t topic = e_topic[i];                              // in [-1, T): -1 only with part offsets that do not start at 0
            topic = topic < 0 ? 0 : topic;
            int32_t q = -1;
            if (n > 0) {
                const uint64_t key = coop_key(topic, id);
                uint32_t h = (uint32_t)coop_first_slot(key, a.bits);
                int w = 0;
                for (; w < slots; ++w) {
                    const uint64_t seen = keys[h];
                    if (seen == 0) break;
                    if (seen == key) { q = (int32_t)owners[h]; break; }
                    h = (h + 1) & mask;
                }
                if (w == slots) bad |= kStatusInternal;
            }
            const int32_t coop = (q == -1 || q == cur) ? cur : -1;
            if (c.prev_owner) c.prev_owner[i] = q;
            if (c.coop_rank) c.coop_rank[i] = coop;
            e_rank[i] = coop;
            if (cur >= 0) {
                if (q == cur) { ++kept; atomicAdd(&cnt[cur], 1u); }
                else if (q < 0) { ++fresh; atomicAdd(&cnt[M + cur], 1u); }
                else { ++withheld; atomicAdd(&cnt[2 * M + cur], 1u); atomicAdd(&held[topic], 1u); }
            } else if (q >= 0) {
                ++dropped;
            }
            if (q >= 0 && q != cur) atomicAdd(&cnt[3 * M + q], 1u);
        }
        kept = wave_sum_u32(kept);
        fresh = wave_sum_u32(fresh);
        withheld = wave_sum_u32(withheld);
        dropped = wave_sum_u32(dropped);
        if (lane == 0) {
            if (kept) atomicAdd(&misc[kSumKept], kept);
            if (fresh) atomicAdd(&misc[kSumFresh], fresh);
            if (withheld) atomicAdd(&misc[kSumWithheld], withheld);
            if (dropped) atomicAdd(&misc[kSumDropped], dropped);
        }
        if (bad) atomicOr(&misc[kSumBad], bad);
    }
    __syncthreads();

    // ---- the counting outputs, in full ------------------------------------------------------------------------------------------
    {
        int64_t* const out[4] = {c.member_kept, c.member_fresh, c.member_pending, c.member_release};
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (out[w])
                for (int r = tid; r < M; r += NT) out[w][r] = (int64_t)cnt[w * M + r];
        if (c.topic_withheld)
            for (int t = tid; t < T; t += NT) c.topic_withheld[t] = (int64_t)held[t];
        if (tid == 0) {
            const int64_t k = misc[kSumKept], f = misc[kSumFresh], w = misc[kSumWithheld], d = misc[kSumDropped];
            if (c.summary) {
                c.summary[0] = k;
                c.summary[1] = f;
                c.summary[2] = w;
                c.summary[3] = d;
                c.summary[4] = (int64_t)misc[kSumClaimed] - (k + w + d);      // claimed - hits = stale
                c.summary[5] = w + d > 0 ? 1 : 0;
            }
            if constexpr (!kFinish)
                if (misc[kSumBad]) atomicOr(a.status, misc[kSumBad]);
        }
    }
    __syncthreads();                                                 // (the table and the counters are done with: the lists take their LDS)

    // ---- lists ---------------------------------------------------------------------------------------------------------------
    int32_t* const l = reinterpret_cast<int32_t*>(lds + kOffLists);
    constexpr int E = kCoopSmallEntries;
    group_small_body_staged<NT, kTailGroupM>(N, M, Tn, l_part_off, e_pid, e_rank, a.r.member_off, N > 0 ? a.r.grouped_topic : nullptr,
                                             a.r.grouped_partition, nullptr, reinterpret_cast<uint32_t*>(lds + kOffStart),
                                             misc + kWsum, misc + kTurn, l, l + E, l + 2 * E, l + 3 * E, l + 4 * E,
                                             reinterpret_cast<uint32_t*>(l + 5 * E), reinterpret_cast<uint32_t*>(l + 6 * E));
    if constexpr (kFinish) {
        // The call ends here, in the order of the finishing form of group_small_kernel (la_group.hip): every thread releases
        // what it stored into the host's memory, the workgroup meets, ONE thread stores `done | status` where the calling thread
        // spins.  The status is what the assignment kernels left in the lane's device word plus this round's own bits (kept in
        // LDS: the list builder leaves the misc words below kWsum alone but for its turn counter); the device word goes back to
        // zero HERE, so a call that ends in an error leaves nothing behind for the next one.  The host copies the outputs out
        // of the staging buffer only when the status is zero: that alone leaves the caller's arrays untouched on an error.
        __threadfence_system();
        __syncthreads();
        if (tid == 0) {
            uint32_t st = __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) | misc[kSumBad];
            if (st) __hip_atomic_store(a.status, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.fin_flag, 0x80000000u | st, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace

hipError_t cooperative_round_launch(CoopScratch& s, LargeScratch& large, const CoopRoundCall& r, bool force_table, uint32_t* status,
                                    hipStream_t stream) {
    hipError_t e;
    if (!force_table && coop_round_is_small(r.c)) {
        CoopSmallArgs a{};
        a.r = r;
        a.status = status;
        a.bits = r.c.n_owned > 0 ? ceil_log2(2 * r.c.n_owned) : 1;
        if ((e = opt_in_lds<coop_round_small_kernel<false>, kCoopSmallLdsBytes>()) != hipSuccess) return e;
        return launch_grid<coop_round_small_kernel<false>>(1, NT, kCoopSmallLdsBytes, stream, a);
    }
    // the general form: the table in device memory, then the grouping of the adjusted ranks
    CoopCall c = r.c;
    if (!c.coop_rank && c.n_partitions > 0) {
        // the ranks first: when they cannot be had nothing has been enqueued
        if ((e = grow_device(&s.ranks, &s.ranks_cap, (size_t)c.n_partitions * 4)) != hipSuccess) return e;
        c.coop_rank = static_cast<int32_t*>(s.ranks);
    }
    if ((e = cooperative_adjust_launch(s, c, status, stream)) != hipSuccess) return e;
    return group_by_member_launch(large, c.n_partitions, c.n_members, c.n_topics, c.part_off, c.out_partition, c.coop_rank,
                                  r.member_off, r.grouped_topic, r.grouped_partition, nullptr, status, stream);
}

// The finishing form: `r` within coop_round_is_small, the target in device memory, everything else (and fin_flag) in the mapped
// staging buffer of a zero-copy call.  Exactly one launch, nothing else enqueued.
hipError_t cooperative_round_finish_launch(const CoopRoundCall& r, int32_t* target_partition, int32_t* target_rank,
                                           uint32_t* status, uint32_t* fin_flag, hipStream_t stream) {
    if (!coop_round_is_small(r.c) || !fin_flag || (target_partition == nullptr) != (target_rank == nullptr)) return hipErrorInvalidValue;
    CoopSmallFinishArgs a{};
    a.r = r;
    a.status = status;
    a.bits = r.c.n_owned > 0 ? ceil_log2(2 * r.c.n_owned) : 1;
    a.target_partition = target_partition;
    a.target_rank = target_rank;
    a.fin_flag = fin_flag;
    const hipError_t e = opt_in_lds<coop_round_small_kernel<true>, kCoopSmallLdsBytes>();
    if (e != hipSuccess) return e;
    return launch_grid<coop_round_small_kernel<true>>(1, NT, kCoopSmallLdsBytes, stream, a);
}

}  // namespace la
