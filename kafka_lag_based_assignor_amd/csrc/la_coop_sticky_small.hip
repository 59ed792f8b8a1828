// la_coop_sticky_small.hip -- the cooperative round WITH sticky ties in one call (la_cooperative_round_sticky_device,
// lagassign.h): what la_cooperative_adjust_device, la_sticky_ties_device and la_cooperative_round_device write when they are
// chained on one stream, bit for bit.
//
// Within the four limits of la_coop.h (kCoopSticky*) the call is ONE launch of ONE workgroup of 1 024 threads whose phases are
// separated by __syncthreads() alone -- no memset, no allocation, nothing in device memory beside the caller's arrays.  The
// pieces are those of la_coop_small.hip (stage, the owned join, the classes, the lists) and of la_sticky.hip (the lag join, the
// re-matching); what both sticky kernels share lies in la_sticky_match.h.
//
//   stage      as in the round: the target's ids and ranks, the T + 1 part offsets and the M + 1 owned offsets into LDS, the
//              owned entries and the input ids into registers; both offset arrays are checked from their LDS copies; the topic
//              of every position from the +1-and-scan.  A topic over the batch's hint is marked here (kStatusShape).
//   lag join   a table of the input (topic, id) pairs, coop_key of la_coop.h, payload = the input's index.  Every target
//              position looks its id up and marks its hit; lag_of of that input goes into LDS.  A duplicate input id, an
//              output id that misses or hits a marked slot: the TOPIC is bad (kStatusSticky) and passed through.
//   owned join the round's insert and lookup into the SAME LDS (cleared in between): q at every target position.
//   re-match   la_sticky.hip's phases 4 to 7 over the whole call as one sequence: a run head is a position whose lag differs
//              from the one before OR where a topic starts, so no run crosses a topic; key = run start << 44 | member << 12 |
//              position with positions of the call (2 048 fit the 12 bits); keyS and keyW through one bitonic sort, the
//              bisections, the packed scan.  The positions of a bad topic get no key: left over as partition and as place alike,
//              in order, they pair with themselves.
//   classify   at destination d the partition is pid[src], its previous owner q[src] -- it travels with the partition, no second
//              lookup -- the owner rank[d].  KEPT, FRESH, WITHHELD, DROPPED or IDLE as in the round; kept before / after per
//              topic and every counter are 32-bit LDS words, written out in full.
//   lists      group_small_body_staged on the adjusted ranks and the sticky ids as they lie in LDS.
//
// Every index comes from a loop counter, a join payload, a bisection or a scan, never from an id or a rank; every walk and loop
// is bounded; no thread waits for another except at a barrier; accesses are one element wide.
//
// Any other call -- or one with LA_COOP_FORCE_TABLE -- is the chain itself through the existing launchers, the intermediate
// d_prev_owner in a buffer of the shard's own.
//
// The kernel has a second, FINISHING form (kFinish: la_assign_batch_cooperative_sticky, fused): the last launch of a
// zero-copy host call, as coop_round_small_kernel<true> is of la_assign_batch_cooperative.  The target comes from device memory
// and is handed on to the host from the stage phase where it is wanted; the part offsets, the input ids, the lag source, the owned
// arrays and every output lie in the call's mapped staging buffer, over the link.  There a gather costs a transaction per word,
// so the lag of input j is computed BY INDEX at stage time -- coalesced -- by the thread that holds in_id of j, and travels to
// its target position through LDS after the lookup (pos_of, in the LDS of q, which is idle until the owned join).  The launch
// ends with `done | status` in the word the calling thread spins on.  kFinish == false is the kernel as it was.
#include "la_coop.h"
#include "la_sticky_match.h"

#include <type_traits>

namespace la {

namespace {

constexpr int NT = kCoopSmallThreads;
constexpr int E = kCoopStickyEntries, TT = kCoopStickyTopics, MM = kCoopStickyMembers;
constexpr int kSlotsMax = 2 * (kCoopStickyEntries > kCoopStickyOwned ? kCoopStickyEntries : kCoopStickyOwned);
static_assert((E & (E - 1)) == 0 && (kCoopStickyOwned & (kCoopStickyOwned - 1)) == 0, "twice the limit is the largest table; the sort takes E keys");
static_assert(E % NT == 0 && kCoopStickyOwned % NT == 0, "a thread holds entries / threads of each input in registers");
static_assert(E <= (int)kKeyPosMask + 1 && E < kNoPos, "positions in 12 bits of a key (la_sticky_match.h), 16-bit indices");
static_assert(E <= kSmallGroupN, "group_small_body_staged scans the topic starts of kSmallGroupN entries");
static_assert(MM + 2 <= kTailGroupM && kTailGroupM % NT == 0, "the list builder's groups: members, nobody, the clamp");
static_assert(MM + 1 < (1 << (kSmallGroupBits + 1)), "a group id fits the ballots of the list builder");
static_assert(NT / kWave <= 16, "wave totals of a scan: misc words kWsum ..");

constexpr size_t up8(size_t x) { return (x + 7) & ~(size_t)7; }

// ---- LDS, in bytes.  A: stage to lists.  B: stage to the counters' flush.  X: one region, a tenant per phase.  C: the lists, over B.
constexpr size_t kOffPartOff = 0;                                                  // A  int64 [T + 1]
constexpr size_t kOffPid = up8(kOffPartOff + 8 * ((size_t)TT + 1));                // A  int32 [N]  the target's ids
constexpr size_t kOffRank = kOffPid + 4 * (size_t)E;                               // A  int32 [N]  target rank, then adjusted rank
constexpr size_t kOffMisc = kOffRank + 4 * (size_t)E;                              // A  uint32 [64]: sums, status, turn, wave totals
constexpr size_t kOffB = up8(kOffMisc + 4 * 64);
constexpr size_t kOffTopic = kOffB;                                                // B  int32 [N]  topic of every position
constexpr size_t kOffQ = kOffTopic + 4 * (size_t)E;                                // B  int32 [N]  previous owner at every TARGET position
constexpr size_t kOffLag = up8(kOffQ + 4 * (size_t)E);                             // B  int64 [N]; once the keys are built:
constexpr size_t kOffPlaced = kOffLag;                                             //    uint16 [N] placed | loose | hole_rank
constexpr size_t kOffTflag = kOffLag + 8 * (size_t)E;                              // B  uint32 [T]  kTopicBad | kTopicChanged
constexpr size_t kOffBefore = kOffTflag + 4 * (size_t)TT;                          // B  uint32 [T]  kept before
constexpr size_t kOffAfter = kOffBefore + 4 * (size_t)TT;                          // B  uint32 [T]  kept after
constexpr size_t kOffSrc = kOffAfter + 4 * (size_t)TT;                             // B  uint16 [N]  src_of
constexpr size_t kOffX = up8(kOffSrc + 2 * (size_t)E);                             // X
constexpr size_t kOffKeys = kOffX;                                                 //    joins: uint64 [slots] keys ...
constexpr size_t kOffPayload = kOffKeys + 8 * (size_t)kSlotsMax;                   //    ... uint32 [slots] payloads
constexpr size_t kEndJoin = kOffPayload + 4 * (size_t)kSlotsMax;
constexpr size_t kOffKeyS = kOffX;                                                 //    re-match: uint64 [n2] keyS | [n2] keyW
constexpr size_t kEndSort = kOffKeyS + 2 * 8 * (size_t)E;
constexpr size_t kOffCnt = kOffX;                                                  //    classify: uint32 [4 M] kept, fresh, pending, release
constexpr size_t kOffWithheld = kOffCnt + 4 * 4 * (size_t)MM;                      //    uint32 [T]
constexpr size_t kOffSticky = kOffWithheld + 4 * (size_t)TT;                       //    int32 [N]  the sticky ids (live through the lists)
constexpr size_t kEndClassify = kOffSticky + 4 * (size_t)E;
constexpr size_t kEndX = kEndJoin;
constexpr size_t kOffOwnedOff = up8(kEndX);                                        // B  int64 [M + 1]
constexpr size_t kEndB = kOffOwnedOff + 8 * ((size_t)MM + 1);
constexpr size_t kOffStart = kOffB;                                                // C  uint32 [kTailGroupM]  the lists' cursors
constexpr size_t kOffLists = kOffStart + 4 * (size_t)kTailGroupM;                  // C  7 x int32 [N]
constexpr size_t kEndC = kOffLists + 7 * 4 * (size_t)E;
constexpr size_t kCoopStickyLdsBytes = kEndB;
static_assert(kEndB <= 160 * 1024, "stage and both joins fit one workgroup's LDS on gfx950");
static_assert(kEndSort <= kEndX && 3 * 2 * (size_t)E <= 8 * (size_t)E, "the re-match: two key arrays in the table, three 16-bit arrays in the lags");
static_assert(kEndClassify <= kEndX, "classify: the counters and the sticky ids in the table");
static_assert(kEndC <= kOffSticky && kEndC <= 160 * 1024, "the lists fit, and leave the sticky ids alone");
static_assert(kOffStart >= kOffMisc + 4 * 64, "the lists leave the part offsets, the adjusted ranks and the misc words alone");
static_assert(kOffPartOff % 8 == 0 && kOffLag % 8 == 0 && kOffKeys % 8 == 0 && kOffOwnedOff % 8 == 0, "64-bit words on 8-byte boundaries");
// the finishing form borrows the LDS of q between the lag join's lookup and the owned join: the target position of every input
constexpr size_t kOffPosOf = kOffQ;                                                // B  uint16 [N]  pos_of, until q is written
static_assert(kOffPosOf + 2 * (size_t)E <= kOffQ + 4 * (size_t)E, "pos_of lies inside q");
static_assert(kOffPosOf + 2 * (size_t)E <= kOffLag && kOffPosOf >= kOffTopic + 4 * (size_t)E, "pos_of leaves the topics and the lags alone");
static_assert(kNoPos >= E && kNoPos <= 0xFFFF, "kNoPos is no position and fits pos_of");
static_assert(kCoopStickyLdsBytes == 160000, "the LDS of both forms (DESIGN 4.13)");

// words of the misc area
constexpr int kSumKept = 0, kSumFresh = 1, kSumWithheld = 2, kSumDropped = 3, kSumClaimed = 4, kSumBad = 5, kTurn = 6, kTies = 7,
              kStBefore = 8, kStAfter = 9, kStChanged = 10, kStPassed = 11, kWsum = 16;
constexpr uint32_t kTopicBad = 1u, kTopicChanged = 4u;
constexpr uint32_t kHitMark = 0x80000000u;          // of a lag-join payload: looked up already

struct CoopStickySmallArgs {
    CoopStickyCall k;
    uint32_t* status;
    int32_t bits_join;          // the lag join has 1 << bits_join slots (N > 0)
    int32_t bits_owned;         // the owned join has 1 << bits_owned slots (n_owned > 0)
    int32_t cap_p;              // partitions of a topic the batch's hint allows
};

// The finishing form (la_assign_batch_cooperative_sticky, fused: la_host.hip, assign_small_zc).  The target lies in device memory;
// the part offsets, the input ids, the lag source, the owned arrays and EVERY output in the call's staging buffer -- coherent host
// memory mapped into the device, read and written in place over the link -- and the launch is the call's last: it ends with
// `done | status` in fin_flag.  Every optional output may be null, the sticky ids included.
struct CoopStickySmallFinishArgs : CoopStickySmallArgs {
    int32_t *target_partition, *target_rank;      // [N] in the staging buffer, or both null: the target as the caller wants it
    uint32_t* fin_flag;                            // host word the calling thread spins on
};

template <bool kFinish>
__global__ __launch_bounds__(NT) void coop_sticky_small_kernel(std::conditional_t<kFinish, CoopStickySmallFinishArgs, CoopStickySmallArgs> a) {
    extern __shared__ uint64_t coop_sticky_lds[];
    constexpr int kScope = __HIP_MEMORY_SCOPE_WORKGROUP;
    char* const lds = reinterpret_cast<char*>(coop_sticky_lds);
    int64_t* const l_part_off = reinterpret_cast<int64_t*>(lds + kOffPartOff);
    int32_t* const e_pid = reinterpret_cast<int32_t*>(lds + kOffPid);
    int32_t* const e_rank = reinterpret_cast<int32_t*>(lds + kOffRank);
    uint32_t* const misc = reinterpret_cast<uint32_t*>(lds + kOffMisc);
    int32_t* const e_topic = reinterpret_cast<int32_t*>(lds + kOffTopic);
    int32_t* const e_q = reinterpret_cast<int32_t*>(lds + kOffQ);
    uint16_t* const pos_of = reinterpret_cast<uint16_t*>(lds + kOffPosOf);      // (kFinish)
    int64_t* const lag = reinterpret_cast<int64_t*>(lds + kOffLag);
    uint16_t* const placed = reinterpret_cast<uint16_t*>(lds + kOffPlaced);
    uint16_t* const loose = placed + E;
    uint16_t* const hole_rank = loose + E;
    uint32_t* const tflag = reinterpret_cast<uint32_t*>(lds + kOffTflag);
    uint32_t* const before = reinterpret_cast<uint32_t*>(lds + kOffBefore);
    uint32_t* const after = reinterpret_cast<uint32_t*>(lds + kOffAfter);
    uint16_t* const src_of = reinterpret_cast<uint16_t*>(lds + kOffSrc);
    uint64_t* const keys = reinterpret_cast<uint64_t*>(lds + kOffKeys);
    uint32_t* const payload = reinterpret_cast<uint32_t*>(lds + kOffPayload);
    uint32_t* const cnt = reinterpret_cast<uint32_t*>(lds + kOffCnt);
    uint32_t* const held = reinterpret_cast<uint32_t*>(lds + kOffWithheld);
    int32_t* const e_sticky = reinterpret_cast<int32_t*>(lds + kOffSticky);
    int64_t* const l_owned_off = reinterpret_cast<int64_t*>(lds + kOffOwnedOff);

    const CoopCall& c = a.k.r.c;
    const StickyCall& s = a.k.s;
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int N = (int)c.n_partitions, n = (int)c.n_owned, M = c.n_members, T = c.n_topics;
    const int jslots = N > 0 ? 1 << a.bits_join : 0, oslots = n > 0 ? 1 << a.bits_owned : 0;
    uint32_t bad = 0;

    // ---- stage: zeros, then every global input once -------------------------------------------------------------------------
    for (int k = tid; k < jslots; k += NT) keys[k] = 0;
    for (int t = tid; t < T; t += NT) {
        tflag[t] = 0;
        before[t] = 0;
        after[t] = 0;
    }
    for (int k = tid; k < N; k += NT) e_topic[k] = 0;
    if (tid < 16) misc[tid] = 0;
    if constexpr (!kFinish) {
        for (int i = tid; i < N; i += NT) {
            e_pid[i] = c.out_partition[i];
            e_rank[i] = c.out_member_rank[i];
        }
    } else {
        // the target on its way from device memory to LDS: where the caller wants it, it goes to the staging buffer from here,
        // while the thread holds both words (coop_round_small_kernel<true>) -- no trip of its own
        for (int i = tid; i < N; i += NT) {
            const int32_t id = c.out_partition[i], rank = c.out_member_rank[i];
            e_pid[i] = id;
            e_rank[i] = rank;
            if (a.target_partition) {
                a.target_partition[i] = id;
                a.target_rank[i] = rank;
            }
            pos_of[i] = (uint16_t)kNoPos;
        }
    }
    for (int t = tid; t <= T && T > 0; t += NT) l_part_off[t] = c.part_off[t];
    constexpr int PERE = E / NT, PERO = kCoopStickyOwned / NT;
    int32_t in_id[PERE], o_topic[PERO], o_id[PERO];
    [[maybe_unused]] int64_t in_lag[PERE];      // (kFinish) the lag of input j, read by index beside its id: one coalesced pass
#pragma unroll
    for (int u = 0; u < PERE; ++u) {
        const int j = u * NT + tid;
        in_id[u] = j < N ? s.pid[j] : 0;
        if constexpr (kFinish) in_lag[u] = j < N ? lag_of(s, (int64_t)j) : 0;
    }
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
    // both offset arrays, from LDS: part_off ascends from 0 to N, the owned offsets ascend inside [0, n_owned]; topic starts;
    // a topic over the hint is passed through
    for (int t = tid; t <= T && T > 0; t += NT) {
        const int64_t o = l_part_off[t];
        if (o < 0 || o > N || (t == 0 && o != 0) || (t == T && o != N) || (t < T && l_part_off[t + 1] < o)) bad |= kStatusShape;
        if (t < T && o >= 0 && o < N) atomicAdd(reinterpret_cast<uint32_t*>(&e_topic[o]), 1u);
        // (unsigned: offsets that are out of range anyway must not overflow the difference)
        if (t < T && l_part_off[t + 1] >= o && (uint64_t)l_part_off[t + 1] - (uint64_t)o > (uint64_t)a.cap_p) {
            bad |= kStatusShape;
            tflag[t] = kTopicBad;
        }
    }
    if (n > 0)
        for (int r = tid; r <= M; r += NT) {
            const int64_t o = l_owned_off[r];
            if (o < 0 || o > n || (r < M && l_owned_off[r + 1] < o)) bad |= kStatusShape;
        }

    // ---- the topic of every position: an inclusive scan of the topic starts, consecutive positions per thread ---------------------
    __syncthreads();
    {
        uint32_t tv[PERE], run = 0;
#pragma unroll
        for (int r = 0; r < PERE; ++r) {
            const int i = PERE * tid + r;
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
        for (int r = 0; r < PERE; ++r) {
            const int i = PERE * tid + r;
            base += tv[r];
            if (i < N) e_topic[i] = (int32_t)base - 1 < 0 ? 0 : (int32_t)base - 1;      // in [0, T): -1 only with offsets that do not start at 0
        }
    }
    __syncthreads();

    // ---- lag join: the inputs in, payload = the input's index ------------------------------------------------------------------
    {
        const uint32_t mask = (uint32_t)jslots - 1u;
#pragma unroll
        for (int u = 0; u < PERE; ++u) {
            const int j = u * NT + tid;
            if (j >= N) continue;
            const int32_t topic = e_topic[j];
            const uint64_t key = coop_key(topic, in_id[u]);
            uint32_t h = (uint32_t)coop_first_slot(key, a.bits_join);
            uint32_t st = kStatusInternal;
            for (int w = 0; w < jslots; ++w) {
                unsigned long long seen = 0;
                if (__hip_atomic_compare_exchange_strong((unsigned long long*)(keys + h), &seen, (unsigned long long)key,
                                                         __ATOMIC_RELAXED, __ATOMIC_RELAXED, kScope)) {
                    payload[h] = (uint32_t)j;
                    st = 0;
                    break;
                }
                if (seen == key) { st = kStatusSticky; break; }      // the id twice in the topic's input segment
                h = (h + 1) & mask;
            }
            if (st & kStatusSticky) __hip_atomic_fetch_or(&tflag[topic], kTopicBad, __ATOMIC_RELAXED, kScope);
            bad |= st;
        }
        __syncthreads();
        // every target position looks its id up and marks the hit; the lag of that input
        for (int i = tid; i < N; i += NT) {
            const int32_t topic = e_topic[i];
            const uint64_t key = coop_key(topic, e_pid[i]);
            uint32_t h = (uint32_t)coop_first_slot(key, a.bits_join);
            uint32_t st = kStatusInternal;
            int64_t l = 0;
            for (int w = 0; w < jslots; ++w) {
                const uint64_t seen = keys[h];
                if (seen == 0) { st = kStatusSticky; break; }       // no input id of the topic
                if (seen == key) {
                    const uint32_t old = __hip_atomic_fetch_or(&payload[h], kHitMark, __ATOMIC_RELAXED, kScope);
                    if (old & kHitMark) st = kStatusSticky;         // the output id twice
                    else if (old < (uint32_t)N) {
                        st = 0;
                        if constexpr (kFinish) pos_of[old] = (uint16_t)i;      // (a marked slot is hit once: one writer per input)
                        else l = lag_of(s, (int64_t)old);
                    }
                    break;
                }
                h = (h + 1) & mask;
            }
            if (st & kStatusSticky) __hip_atomic_fetch_or(&tflag[topic], kTopicBad, __ATOMIC_RELAXED, kScope);
            bad |= st;
            lag[i] = l;
        }
    }
    __syncthreads();

    // ---- owned join, in the same LDS: insert, then q at every target position ---------------------------------------------------
    for (int k = tid; k < oslots; k += NT) keys[k] = 0;
    if constexpr (kFinish) {
        // the lag of input j to the position that looked it up (every position holds 0 since the lookup: a miss keeps it); q is
        // written two barriers from here
#pragma unroll
        for (int u = 0; u < PERE; ++u) {
            const int j = u * NT + tid;
            if (j >= N) continue;
            const uint32_t p = pos_of[j];
            if (p < (uint32_t)N) lag[p] = in_lag[u];
        }
    }
    __syncthreads();
    if (n > 0) {
        const uint32_t mask = (uint32_t)oslots - 1u;
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
            uint32_t h = (uint32_t)coop_first_slot(key, a.bits_owned);
            uint32_t st = kStatusInternal;
            for (int w = 0; w < oslots; ++w) {
                unsigned long long seen = 0;
                if (__hip_atomic_compare_exchange_strong((unsigned long long*)(keys + h), &seen, (unsigned long long)key,
                                                         __ATOMIC_RELAXED, __ATOMIC_RELAXED, kScope)) {
                    payload[h] = r;
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
    __syncthreads();
    for (int i = tid; i < N; i += NT) {
        int32_t q = -1;
        if (n > 0) {
            const uint32_t mask = (uint32_t)oslots - 1u;
            const uint64_t key = coop_key(e_topic[i], e_pid[i]);
            uint32_t h = (uint32_t)coop_first_slot(key, a.bits_owned);
            int w = 0;
            for (; w < oslots; ++w) {
                const uint64_t seen = keys[h];
                if (seen == 0) break;
                if (seen == key) { q = (int32_t)payload[h]; break; }
                h = (h + 1) & mask;
            }
            if (w == oslots) bad |= kStatusInternal;
            if (q < 0 || q >= M) q = -1;                             // (what this call's insert stored: a member)
        }
        e_q[i] = q;
        if (q >= 0 && q == e_rank[i]) atomicAdd(&before[e_topic[i]], 1u);
    }
    __syncthreads();

    // ---- re-match: la_sticky.hip 4 to 7, the call as one sequence ------------------------------------------------------------
    // 4: thread by thread a contiguous chunk of positions, so that a scan over the threads is a scan over the positions
    int n2 = 1;
    while (n2 < N) n2 <<= 1;                                          // what the bitonic sort takes
    uint64_t* const key_s = reinterpret_cast<uint64_t*>(lds + kOffKeyS);
    uint64_t* const key_w = key_s + n2;
    const int per = (N + NT - 1) / NT;
    const int i0 = tid * per < N ? tid * per : N, i1 = i0 + per < N ? i0 + per : N;
    const auto same_run = [&](int i) { return i > 0 && lag[i] == lag[i - 1] && e_topic[i] == e_topic[i - 1]; };
    {
        uint32_t head = 0;
        bool ties = false;
        for (int i = i0; i < i1; ++i) {
            if (same_run(i)) ties = true;
            else head = (uint32_t)i;
        }
        if (ties) __hip_atomic_fetch_or(&misc[kTies], 1u, __ATOMIC_RELAXED, kScope);
        uint32_t unused = 0;
        uint32_t run = workgroup_excl_scan<true>(head, misc + kWsum, tid, NT, &unused);      // (its barriers: the flag is there)
        const bool any_ties = misc[kTies] != 0;     // workgroup-uniform; without a run of two every partition stays where it is
        // 5 (both joins are done with the table)
        if (any_ties) {
            for (int i = i0; i < i1; ++i) {
                if (!same_run(i)) run = (uint32_t)i;
                const int32_t ci = e_rank[i], qi = e_q[i];
                const bool pass = (tflag[e_topic[i]] & kTopicBad) != 0;
                const uint64_t at = ((uint64_t)run << kKeyRunShift) | (uint64_t)i;
                key_s[i] = (ci >= 0 && !pass) ? at | ((uint64_t)(uint32_t)ci << kKeyMemberShift) : kNoKey;
                key_w[i] = (qi >= 0 && !pass) ? at | ((uint64_t)(uint32_t)qi << kKeyMemberShift) : kNoKey;
            }
            for (int i = N + tid; i < n2; i += NT) {
                key_s[i] = kNoKey;
                key_w[i] = kNoKey;
            }
        }
        __syncthreads();
        for (int i = tid; i < N; i += NT) {         // (the lags are dead since that barrier)
            src_of[i] = kNoPos;
            placed[i] = 0;
        }
        __syncthreads();
        if (any_ties) {
            // The bitonic network of la_sticky.hip; at most E / 2 = NT pairs, so thread p IS pair p in every stage.  The pairs of
            // one wavefront, 64 p .. 64 p + 63, at distance j <= 64 lie inside the 128 keys from 128 p on, which no other
            // wavefront touches before the next distance > 64: those stages need no workgroup barrier (66 barriers at the
            // limit become 15), only the order in which a wavefront's own LDS accesses execute.
            static_assert(E / 2 <= NT && kWave == 64, "a pair per thread; the pairs of a wavefront at distance <= 64 share 128 keys");
            const auto exchange = [&](int j, int k) {
                const int p = tid;
                if (p >= n2 / 2) return;
                const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo | j;
                const bool asc = (lo & k) == 0;
                const uint64_t s0 = key_s[lo], s1 = key_s[hi];
                if ((s0 > s1) == asc) {
                    key_s[lo] = s1;
                    key_s[hi] = s0;
                }
                const uint64_t w0 = key_w[lo], w1 = key_w[hi];
                if ((w0 > w1) == asc) {
                    key_w[lo] = w1;
                    key_w[hi] = w0;
                }
            };
            for (int k = 2; k <= n2; k <<= 1) {
                int j = k >> 1;
                for (; j > kWave; j >>= 1) {
                    exchange(j, k);
                    __syncthreads();
                }
                for (; j > 0; j >>= 1) {
                    exchange(j, k);
                    wave_lds_fence();
                }
                if (k >= 2 * kWave) __syncthreads();                // (the next k starts at a distance > 64, or the sort is done)
            }
            __syncthreads();
            for (int x = tid; x < n2; x += NT) {
                const uint64_t kw = key_w[x];
                if (kw == kNoKey) continue;
                const uint64_t group = kw & ~kKeyPosMask;                           // (run, member), position 0
                const int k = x - first_not_below(key_w, n2, group);
                const int s0 = first_not_below(key_s, n2, group), s1 = first_not_below(key_s, n2, group + kKeyPosMask + 1);
                if (k >= 0 && k < s1 - s0) {
                    const int src = (int)(kw & kKeyPosMask), dst = (int)(key_s[s0 + k] & kKeyPosMask);
                    if (src < N && dst < N) {           // (positions this call put into its keys)
                        src_of[dst] = (uint16_t)src;
                        placed[src] = 1;
                    }
                }
            }
        }
        __syncthreads();
    }
    // 6 (the keys are dead: the counters of the classes take their LDS)
    for (int k = tid; k < 4 * M; k += NT) cnt[k] = 0;
    for (int t = tid; t < T; t += NT) held[t] = 0;
    uint32_t counts = 0;                            // partitions not placed | positions not filled << 16
    for (int i = i0; i < i1; ++i) counts += (placed[i] ? 0u : 1u) + (src_of[i] == kNoPos ? 1u << 16 : 0u);
    uint32_t totals = 0;
    const uint32_t ranks = workgroup_excl_scan<false>(counts, misc + kWsum, tid, NT, &totals);
    {
        uint32_t r_loose = ranks & 0xFFFFu, r_hole = ranks >> 16;
        for (int i = i0; i < i1; ++i) {
            if (!placed[i] && r_loose < (uint32_t)N) loose[r_loose++] = (uint16_t)i;
            if (src_of[i] == kNoPos) hole_rank[i] = (uint16_t)r_hole++;
        }
    }
    const bool sound = (totals & 0xFFFFu) == (totals >> 16);                   // as many left over as places left
    if (!sound) bad |= kStatusInternal;
    __syncthreads();

    // ---- classify: the partition at d comes from src, its previous owner with it ------------------------------------------------
    {
        uint32_t kept = 0, fresh = 0, withheld = 0, dropped = 0;
        for (int d = tid; d < N; d += NT) {
            uint32_t src = src_of[d];
            if (src == kNoPos) {
                const uint32_t r = hole_rank[d];
                src = r < (totals & 0xFFFFu) ? loose[r] : kNoPos;
            }
            if (!sound || src >= (uint32_t)N) src = (uint32_t)d;
            const int32_t id = e_pid[src], q = e_q[src], cur = e_rank[d], topic = e_topic[d];
            if (!kFinish || s.sticky) s.sticky[d] = id;
            e_sticky[d] = id;
            if (q >= 0 && q == cur) atomicAdd(&after[topic], 1u);
            if (src != (uint32_t)d) __hip_atomic_fetch_or(&tflag[topic], kTopicChanged, __ATOMIC_RELAXED, kScope);
            if (cur < -1 || cur >= M) {                              // never stored through; the lists file it under "nobody"
                bad |= kStatusCoop;
                e_rank[d] = -1;
                continue;
            }
            const int32_t coop = (q == -1 || q == cur) ? cur : -1;
            if (c.prev_owner) c.prev_owner[d] = q;
            if (c.coop_rank) c.coop_rank[d] = coop;
            e_rank[d] = coop;
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
        uint32_t sb = 0, sa = 0, changed = 0, passed = 0;
        for (int t = tid; t < T; t += NT) {
            const uint32_t b = before[t], f = tflag[t];
            const uint32_t k = (f & kTopicBad) ? b : after[t];      // passed through: a copy, kept as before
            if (c.topic_withheld) c.topic_withheld[t] = (int64_t)held[t];
            if (s.topic_kept) s.topic_kept[t] = (int64_t)k;
            if (s.topic_saved) s.topic_saved[t] = (int64_t)k - (int64_t)b;
            sb += b;
            sa += k;
            changed += (f & kTopicChanged) ? 1u : 0u;
            passed += (f & kTopicBad) ? 1u : 0u;
        }
        sb = wave_sum_u32(sb);
        sa = wave_sum_u32(sa);
        changed = wave_sum_u32(changed);
        passed = wave_sum_u32(passed);
        if (lane == 0) {
            if (sb) atomicAdd(&misc[kStBefore], sb);
            if (sa) atomicAdd(&misc[kStAfter], sa);
            if (changed) atomicAdd(&misc[kStChanged], changed);
            if (passed) atomicAdd(&misc[kStPassed], passed);
        }
    }
    __syncthreads();
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
        if (s.summary) {
            s.summary[0] = (int64_t)misc[kStBefore];
            s.summary[1] = (int64_t)misc[kStAfter];
            s.summary[2] = (int64_t)misc[kStChanged];
            s.summary[3] = (int64_t)misc[kStPassed];
        }
        if constexpr (!kFinish)
            if (misc[kSumBad]) atomicOr(a.status, misc[kSumBad]);
    }
    __syncthreads();                                                 // (everything but A and the sticky ids is done with: the lists take the LDS)

    // ---- lists ---------------------------------------------------------------------------------------------------------------
    int32_t* const l = reinterpret_cast<int32_t*>(lds + kOffLists);
    group_small_body_staged<NT, kTailGroupM>(N, M, T, l_part_off, e_sticky, e_rank, a.k.r.member_off, N > 0 ? a.k.r.grouped_topic : nullptr,
                                             a.k.r.grouped_partition, nullptr, reinterpret_cast<uint32_t*>(lds + kOffStart),
                                             misc + kWsum, misc + kTurn, l, l + E, l + 2 * E, l + 3 * E, l + 4 * E,
                                             reinterpret_cast<uint32_t*>(l + 5 * E), reinterpret_cast<uint32_t*>(l + 6 * E));
    if constexpr (kFinish) {
        // The call ends here, in the order of coop_round_small_kernel<true>: every thread releases what it stored into the host's
        // memory, the workgroup meets, ONE thread stores `done | status` where the calling thread spins.  The status is what the
        // assignment kernels left in the lane's device word plus this round's own bits (kept in LDS: the list builder leaves the
        // misc words below kWsum alone but for its turn counter); the device word goes back to zero HERE, so a call that ends in
        // an error leaves nothing behind for the next one.
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

hipError_t cooperative_round_sticky_launch(CoopScratch& sc, StickyScratch& sticky, LargeScratch& large, const CoopStickyCall& k, bool force_table,
                                           uint32_t* status, hipStream_t stream) {
    hipError_t e;
    const CoopCall& c = k.r.c;
    if (!force_table && coop_sticky_is_small(c)) {
        const int64_t hint = k.s.max_partitions_per_topic;
        CoopStickySmallArgs a{};
        a.k = k;
        a.status = status;
        a.bits_join = c.n_partitions > 0 ? ceil_log2(2 * c.n_partitions) : 1;
        a.bits_owned = c.n_owned > 0 ? ceil_log2(2 * c.n_owned) : 1;
        a.cap_p = (int32_t)(hint <= 0 || hint > kVerifyMaxPartitions ? kVerifyMaxPartitions : hint);      // as sticky_ties_launch
        if ((e = opt_in_lds<coop_sticky_small_kernel<false>, kCoopStickyLdsBytes>()) != hipSuccess) return e;
        return launch_grid<coop_sticky_small_kernel<false>>(1, NT, kCoopStickyLdsBytes, stream, a);
    }
    // the general form, the chain itself.  Both buffers of the shard's own first: when they cannot be had nothing has been enqueued
    const int64_t N = c.n_partitions;
    if (N > 0) {
        if ((e = grow_device(&sc.prev, &sc.prev_cap, (size_t)N * 4)) != hipSuccess) return e;
        if (!c.coop_rank && (e = grow_device(&sc.ranks, &sc.ranks_cap, (size_t)N * 4)) != hipSuccess) return e;
    }
    const bool sticky_large = k.h_part_off != nullptr && k.s.n_topics > 0;
    if (sticky_large && (e = sticky_large_reserve(sticky, k.s, k.h_part_off)) != hipSuccess) return e;
    CoopCall first = c;                             // the target against the owned lists, wanting only the previous owners
    first.prev_owner = static_cast<int32_t*>(sc.prev);
    first.coop_rank = nullptr;
    first.member_kept = first.member_fresh = first.member_pending = first.member_release = first.topic_withheld = first.summary = nullptr;
    if ((e = cooperative_adjust_launch(sc, first, status, stream)) != hipSuccess) return e;
    StickyCall s = k.s;
    s.prev_owner = static_cast<const int32_t*>(sc.prev);
    if ((e = sticky_ties_launch(s, status, stream, sticky_large ? &sticky : nullptr, k.h_part_off, true)) != hipSuccess) return e;
    CoopRoundCall r = k.r;                          // the round on the sticky order
    r.c.out_partition = s.sticky;
    return cooperative_round_launch(sc, large, r, force_table, status, stream);
}

// The finishing form: `k` within coop_sticky_is_small, the target in device memory, everything else (and fin_flag) in the mapped
// staging buffer of a zero-copy call.  Exactly one launch, nothing else enqueued.
hipError_t cooperative_round_sticky_finish_launch(const CoopStickyCall& k, int32_t* target_partition, int32_t* target_rank,
                                                  uint32_t* status, uint32_t* fin_flag, hipStream_t stream) {
    const CoopCall& c = k.r.c;
    if (!coop_sticky_is_small(c) || !fin_flag || (target_partition == nullptr) != (target_rank == nullptr)) return hipErrorInvalidValue;
    const int64_t hint = k.s.max_partitions_per_topic;
    CoopStickySmallFinishArgs a{};
    a.k = k;
    a.status = status;
    a.bits_join = c.n_partitions > 0 ? ceil_log2(2 * c.n_partitions) : 1;
    a.bits_owned = c.n_owned > 0 ? ceil_log2(2 * c.n_owned) : 1;
    a.cap_p = (int32_t)(hint <= 0 || hint > kVerifyMaxPartitions ? kVerifyMaxPartitions : hint);      // as sticky_ties_launch
    a.target_partition = target_partition;
    a.target_rank = target_rank;
    a.fin_flag = fin_flag;
    const hipError_t e = opt_in_lds<coop_sticky_small_kernel<true>, kCoopStickyLdsBytes>();
    if (e != hipSuccess) return e;
    return launch_grid<coop_sticky_small_kernel<true>>(1, NT, kCoopStickyLdsBytes, stream, a);
}

}  // namespace la
