// la_sticky.hip -- sticky ties: among partitions of equal lag the previous owner decides (la_sticky_ties_device, lagassign.h).
//
// The reference hands a topic's partitions out by (lag descending, id ascending).  Inside a RUN of equal lag the greedy cannot
// tell the partitions apart: permuting them leaves the owner at every position, every count and every total as they are.  So
// inside each run, per member c: S_c = the positions c owns, W_c = the positions whose partition c owned before, both
// ascending; the partition at W_c[k] goes to S_c[k] for k < min(|S_c|, |W_c|), and the partitions left over fill the positions
// left over, both in ascending order.  That keeps sum_c min(|S_c|, |W_c|) partitions with their owner, the most any
// permutation inside the runs can.
//
// One workgroup per topic, persistent workgroups walk topics blockIdx.x, + gridDim.x, ...  Per topic, in LDS:
//   [A: the table, 2^ceil(log2(2 P)) words; once the lookups are done: keyS[n2] | keyW[n2], n2 = half the table >= P]
//   [lag[P]; once the keys are built: placed[P] | loose[P] | hole_rank[P] of 16 bits] [own[P]] [prev[P]] [src_of[P] of 16 bits]
//   [two 64-bit counters, the topic's flags, the scans' wave totals]
//   1  clear the table
//   2  insert the input ids, payload = the input's index (a duplicate: the topic is BAD)
//   3  look every output id up (a miss or a second hit: BAD), lag[i] from the input entry; own[i], prev[i]; count kept before
//   4  run heads by a max-scan over (i where lag[i] != lag[i-1]); no two neighbours equal: the topic is copied, done
//   5  key = run start << 44 | (uint32) member << 12 | position: keyS over own >= 0, keyW over prev >= 0, everything else all
//      ones; both arrays through one bitonic sort.  Slot a of keyW bisects the start of its (run, member) group in keyW -> its
//      index k in the group, and the group's range in keyS; k below that range's size: src_of[S position] = W position
//   6  one scan over (partition not placed, position not filled), packed in one word: loose[rank] = source, hole_rank[position];
//      the two counts agree inside every run, so the k-th of one pairs with the k-th of the other across the topic
//   7  sticky[d] = out_partition[src_of[d], or loose[hole_rank[d]]]; count kept after
//   8  per-topic counts by plain stores (thread 0), the summary once per workgroup
// A BAD topic, one over the limit and one over the hint are PASSED THROUGH: sticky = a copy, kept after = kept before.
// With LA_FLAG_STICKY_LARGE the topics over the limit that the host listed have been re-matched by the global form
// (la_sticky_large.hip) in front of this kernel: for those it only stores the counts that form left and adds them to the summary.
// Every phase is safe on any content: an index comes from the join's own payload, a bisection or a scan, never from an id or a
// rank; a topic leaves nothing behind -- every word a later topic reads it has written itself behind a barrier.  Accesses are
// one element wide.  No thread waits for another except at a barrier; every loop is bounded.
#include <algorithm>

#include "la_kernels.h"
#include "la_device.h"
#include "la_join.h"
#include "la_sticky_match.h"

namespace la {

namespace {

constexpr int kStickyThreads = 256;
constexpr int kStickyFewThreads = 64;               // topics up to kStickyFewPartitions: one wavefront, barriers cost nothing
constexpr int64_t kStickyFewPartitions = 256;
constexpr int64_t kStickyMaxPartitions = kVerifyMaxPartitions;
constexpr uint32_t kTopicBad = 1u, kTopicTies = 2u, kTopicChanged = 4u;
static_assert(kStickyMaxPartitions <= (int64_t)kKeyPosMask + 1 && kStickyMaxPartitions < kNoPos, "positions in 12 bits of a key (la_sticky_match.h), 16-bit indices");

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

struct StickyArgs {
    StickyCall c;
    uint32_t* status;
    StickyWork g;               // n_big == 0: no topic went through the global form (la_sticky_large.hip)
    int32_t large;              // LA_FLAG_STICKY_LARGE: a topic the global form takes that is not in its list is a shape error
    int32_t cap_p;              // partitions of a topic the LDS request holds
    uint32_t off_lag, off_own, off_prev, off_src, off_ctl;      // byte offsets of the regions behind A
};

struct StickyLayout {
    uint32_t off_lag, off_own, off_prev, off_src, off_ctl;
    size_t bytes;
};

constexpr size_t kStickyCtlBytes = 48;              // kept before, kept after (64 bits each) | flags | pad | 4 wave totals

inline StickyLayout layout_for(int64_t cap_p) {
    StickyLayout l{};
    size_t at = up16((size_t)8 << ceil_log2(2 * cap_p));
    l.off_lag = (uint32_t)at;   at += up16(8 * (size_t)cap_p);
    l.off_own = (uint32_t)at;   at += up16(4 * (size_t)cap_p);
    l.off_prev = (uint32_t)at;  at += up16(4 * (size_t)cap_p);
    l.off_src = (uint32_t)at;   at += up16(2 * (size_t)cap_p);
    l.off_ctl = (uint32_t)at;   at += kStickyCtlBytes;
    l.bytes = at;
    return l;
}
constexpr size_t kStickyMaxLdsBytes = 8 * 2 * (size_t)kStickyMaxPartitions + 8 * (size_t)kStickyMaxPartitions +
                                      2 * 4 * (size_t)kStickyMaxPartitions + 2 * (size_t)kStickyMaxPartitions + kStickyCtlBytes;
static_assert((kStickyMaxPartitions & (kStickyMaxPartitions - 1)) == 0, "2 x the limit is the table of the largest topic");
static_assert(kStickyMaxLdsBytes <= 160 * 1024, "one workgroup's LDS on gfx950");
static_assert(kStickyThreads / kWave <= 4, "wave totals of a scan");

struct StickyTally {            // thread 0: what this workgroup's topics add to the summary
    uint64_t before = 0, after = 0, changed = 0, passed = 0;
};

__global__ __launch_bounds__(kStickyThreads) void sticky_kernel(StickyArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sticky_lds[];
    constexpr int kScope = __HIP_MEMORY_SCOPE_WORKGROUP;
    const StickyCall& c = a.c;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    uint64_t* table = reinterpret_cast<uint64_t*>(sticky_lds);
    int64_t* lag = reinterpret_cast<int64_t*>(sticky_lds + a.off_lag);
    uint16_t* placed = reinterpret_cast<uint16_t*>(sticky_lds + a.off_lag);      // lag's region again, once the keys are built
    uint16_t* loose = placed + a.cap_p;
    uint16_t* hole_rank = loose + a.cap_p;
    int32_t* own = reinterpret_cast<int32_t*>(sticky_lds + a.off_own);
    int32_t* prev = reinterpret_cast<int32_t*>(sticky_lds + a.off_prev);
    uint16_t* src_of = reinterpret_cast<uint16_t*>(sticky_lds + a.off_src);
    unsigned long long* kept = reinterpret_cast<unsigned long long*>(sticky_lds + a.off_ctl);      // [0] before, [1] after
    uint32_t* topic_flags = reinterpret_cast<uint32_t*>(sticky_lds + a.off_ctl + 16);
    uint32_t* wave_tot = reinterpret_cast<uint32_t*>(sticky_lds + a.off_ctl + 32);
    if (tid == 0) {
        kept[0] = 0;
        kept[1] = 0;
        *topic_flags = 0;
    }
    __syncthreads();
    uint32_t bad = 0;
    StickyTally tally;

    // The topic's last step, every thread calling: thread 0 stores its counts and clears the words for the next topic.
    // copied: sticky is out_partition as it came, so kept after is kept before; passed: the topic counts as passed through.
    const auto finish = [&](int64_t t, bool copied, bool passed) {
        __syncthreads();                            // (also: every thread is done with this topic's LDS)
        if (tid == 0) {
            const uint64_t before = kept[0], after = copied ? before : kept[1];
            if (c.topic_kept) c.topic_kept[t] = (int64_t)after;
            if (c.topic_saved) c.topic_saved[t] = (int64_t)(after - before);
            tally.before += before;
            tally.after += after;
            tally.changed += (*topic_flags & kTopicChanged) ? 1 : 0;
            tally.passed += passed ? 1 : 0;
            kept[0] = 0;
            kept[1] = 0;
            *topic_flags = 0;
        }
        __syncthreads();
    };
    // sticky <- out_partition over [p0, p0 + np); with count: the positions kept as they are -> kept[0]
    const auto copy_topic = [&](int64_t p0, int64_t np, bool count) {
        unsigned long long n = 0;
        for (int64_t i = tid; i < np; i += nt) {
            c.sticky[p0 + i] = c.out_pid[p0 + i];
            if (count) {
                const int32_t ci = c.out_rank[p0 + i];
                n += (ci >= 0 && c.prev_owner[p0 + i] == ci) ? 1 : 0;
            }
        }
        if (n) __hip_atomic_fetch_add(kept, n, __ATOMIC_RELAXED, kScope);
    };

    for (int64_t t = blockIdx.x; t < c.n_topics; t += gridDim.x) {
        // workgroup-uniform, as all that follows from it
        const int64_t p0 = c.part_off[t], p1 = c.part_off[t + 1];
        const int64_t np = p1 - p0;
        if (p0 < 0 || p1 < p0 || p1 > c.n_partitions) {      // nothing is read through such offsets, nothing written
            bad |= kStatusShape;
            continue;
        }
        if (a.g.n_big > 0) {                        // a topic of the host's list: the global form has written its order and left its counts
            int lo = 0, hi = a.g.n_big;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)a.g.big[mid].topic <= t) lo = mid;
                else hi = mid;
            }
            if ((int64_t)a.g.big[lo].topic == t) {
                if (a.g.big[lo].p0 != p0 || a.g.big[lo].np != np) {      // it worked from the host's offsets, these are others
                    bad |= kStatusShape;
                    continue;
                }
                if (tid == 0) {
                    const uint32_t bits = (uint32_t)a.g.ctr[4 * lo + 2];
                    kept[0] = a.g.ctr[4 * lo + 0];
                    kept[1] = a.g.ctr[4 * lo + 1];
                    if (bits & kStickyBigChanged) *topic_flags = kTopicChanged;
                    if (bits & kStickyBigBad) bad |= kStatusSticky;
                }
                const bool big_bad = (a.g.ctr[4 * lo + 2] & kStickyBigBad) != 0;
                finish(t, big_bad, big_bad);
                continue;
            }
        }
        if (np > a.cap_p) {                         // over the limit: data; within the limit but over the hint: an error as well
            if (np <= kStickyMaxPartitions || (a.large && np <= kStickyGlobalMaxPartitions)) bad |= kStatusShape;      // (the host's list would have held it)
            copy_topic(p0, np, true);
            finish(t, true, true);
            continue;
        }
        const int P = (int)np;
        const int bits = P > 0 ? 32 - __builtin_clz((uint32_t)(2 * P - 1)) : 1;      // 2^bits >= 2 P: at most half full
        const int n2 = 1 << (bits - 1);             // >= P: what the bitonic sort takes, two arrays of it are the table
        uint64_t* key_s = table;
        uint64_t* key_w = table + n2;
        uint32_t f = 0;

        // 1
        if (P > 0)
            for (int i = tid; i < (1 << bits); i += nt) table[i] = 0;
        __syncthreads();

        // 2
        for (int j = tid; j < P; j += nt) {
            const uint32_t st = table_insert<kScope>(table, bits, c.pid[p0 + j], j);
            if (st) f |= kTopicBad;
            bad |= st & kStatusInternal;
        }
        __syncthreads();

        // 3
        unsigned long long n_kept = 0;
        for (int i = tid; i < P; i += nt) {
            int32_t j = 0;
            const uint32_t st = table_lookup<kScope>(table, bits, c.out_pid[p0 + i], &j);
            int64_t l = 0;
            if (st) {
                f |= kTopicBad;
                bad |= st & kStatusInternal;
            } else if (j >= 0 && j < P) {           // (the payload this topic's insert stored)
                l = lag_of(c, p0 + j);
            } else {
                f |= kTopicBad;
                bad |= kStatusInternal;
            }
            lag[i] = l;
            const int32_t ci = c.out_rank[p0 + i], qi = c.prev_owner[p0 + i];
            own[i] = ci;
            prev[i] = qi;
            n_kept += (ci >= 0 && qi == ci) ? 1 : 0;
        }
        if (f) __hip_atomic_fetch_or(topic_flags, f, __ATOMIC_RELAXED, kScope);
        if (n_kept) __hip_atomic_fetch_add(kept, n_kept, __ATOMIC_RELAXED, kScope);
        __syncthreads();
        if (*topic_flags & kTopicBad) {
            bad |= kStatusSticky;
            copy_topic(p0, np, false);
            finish(t, true, true);
            continue;
        }

        // 4: thread by thread a contiguous chunk of positions, so that a scan over the threads is a scan over the positions
        const int per = (P + nt - 1) / nt;
        const int i0 = tid * per < P ? tid * per : P, i1 = i0 + per < P ? i0 + per : P;
        uint32_t head = 0;
        bool ties = false;
        for (int i = i0; i < i1; ++i) {
            if (i > 0 && lag[i] == lag[i - 1]) ties = true;
            else head = (uint32_t)i;
        }
        if (ties) __hip_atomic_fetch_or(topic_flags, kTopicTies, __ATOMIC_RELAXED, kScope);
        uint32_t unused = 0;
        uint32_t run = workgroup_excl_scan<true>(head, wave_tot, tid, nt, &unused);      // (its barriers: the flag is there)
        if (!(*topic_flags & kTopicTies)) {         // no run of two: every partition stays where it is
            copy_topic(p0, np, false);
            finish(t, true, false);
            continue;
        }

        // 5 (the table is dead since 3's barrier)
        for (int i = i0; i < i1; ++i) {
            if (!(i > 0 && lag[i] == lag[i - 1])) run = (uint32_t)i;
            const int32_t ci = own[i], qi = prev[i];
            const uint64_t at = ((uint64_t)run << kKeyRunShift) | (uint64_t)i;
            key_s[i] = ci >= 0 ? at | ((uint64_t)(uint32_t)ci << kKeyMemberShift) : kNoKey;
            key_w[i] = qi >= 0 ? at | ((uint64_t)(uint32_t)qi << kKeyMemberShift) : kNoKey;
        }
        for (int i = P + tid; i < n2; i += nt) {
            key_s[i] = kNoKey;
            key_w[i] = kNoKey;
        }
        __syncthreads();
        for (int i = tid; i < P; i += nt) {         // (lag is dead since that barrier)
            src_of[i] = kNoPos;
            placed[i] = 0;
        }
        for (int k = 2; k <= n2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int p = tid; p < n2 / 2; p += nt) {
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
                }
                __syncthreads();
            }
        }
        __syncthreads();
        for (int x = tid; x < n2; x += nt) {
            const uint64_t kw = key_w[x];
            if (kw == kNoKey) continue;
            const uint64_t group = kw & ~kKeyPosMask;                           // (run, member), position 0
            const int k = x - first_not_below(key_w, n2, group);
            const int s0 = first_not_below(key_s, n2, group), s1 = first_not_below(key_s, n2, group + kKeyPosMask + 1);
            if (k >= 0 && k < s1 - s0) {
                const int src = (int)(kw & kKeyPosMask), dst = (int)(key_s[s0 + k] & kKeyPosMask);
                if (src < P && dst < P) {           // (positions this topic put into its keys)
                    src_of[dst] = (uint16_t)src;
                    placed[src] = 1;
                }
            }
        }
        __syncthreads();

        // 6
        uint32_t counts = 0;                        // partitions not placed | positions not filled << 16
        for (int i = i0; i < i1; ++i) counts += (placed[i] ? 0u : 1u) + (src_of[i] == kNoPos ? 1u << 16 : 0u);
        uint32_t totals = 0;
        const uint32_t ranks = workgroup_excl_scan<false>(counts, wave_tot, tid, nt, &totals);
        uint32_t r_loose = ranks & 0xFFFFu, r_hole = ranks >> 16;
        for (int i = i0; i < i1; ++i) {
            if (!placed[i] && r_loose < (uint32_t)P) loose[r_loose++] = (uint16_t)i;
            if (src_of[i] == kNoPos) hole_rank[i] = (uint16_t)r_hole++;
        }
        const bool sound = (totals & 0xFFFFu) == (totals >> 16);               // as many left over as places left
        if (!sound) bad |= kStatusInternal;
        __syncthreads();

        // 7
        f = 0;
        n_kept = 0;
        for (int d = tid; d < P; d += nt) {
            uint32_t src = src_of[d];
            if (src == kNoPos) {
                const uint32_t r = hole_rank[d];
                src = r < (totals & 0xFFFFu) ? loose[r] : kNoPos;
            }
            if (!sound || src >= (uint32_t)P) src = (uint32_t)d;
            c.sticky[p0 + d] = c.out_pid[p0 + src];
            const int32_t qs = prev[src];
            n_kept += (qs >= 0 && qs == own[d]) ? 1 : 0;
            if (src != (uint32_t)d) f |= kTopicChanged;
        }
        if (f) __hip_atomic_fetch_or(topic_flags, f, __ATOMIC_RELAXED, kScope);
        if (n_kept) __hip_atomic_fetch_add(kept + 1, n_kept, __ATOMIC_RELAXED, kScope);

        // 8
        finish(t, false, false);
    }
    if (tid == 0 && c.summary) {
        if (tally.before) global_add(c.summary + 0, tally.before);
        if (tally.after) global_add(c.summary + 1, tally.after);
        if (tally.changed) global_add(c.summary + 2, tally.changed);
        if (tally.passed) global_add(c.summary + 3, tally.passed);
    }
    if (bad) atomicOr(a.status, bad);
}

}  // namespace

hipError_t sticky_ties_launch(const StickyCall& c, uint32_t* status, hipStream_t stream, StickyScratch* large,
                              const int64_t* h_part_off, bool reserved) {
    hipError_t e;
    StickyWork g{};
    // the global form first: the LDS kernel behind it stores and counts its topics' results too
    if (large && c.n_topics > 0) {
        if (!reserved && (e = sticky_large_reserve(*large, c, h_part_off)) != hipSuccess) return e;
        if ((e = sticky_large_enqueue(*large, c, status, stream, &g)) != hipSuccess) return e;
    }
    if (c.summary && (e = hipMemsetAsync(c.summary, 0, 32, stream)) != hipSuccess) return e;
    if (c.n_topics <= 0) return hipSuccess;

    // the hint sizes the LDS request and nothing else; without a usable one the request is the limit's
    const int64_t hint = c.max_partitions_per_topic;
    StickyArgs a{};
    a.c = c;
    a.status = status;
    a.g = g;
    a.large = large ? 1 : 0;
    a.cap_p = (int32_t)(hint <= 0 || hint > kStickyMaxPartitions ? kStickyMaxPartitions : hint);
    const StickyLayout l = layout_for(a.cap_p);
    a.off_lag = l.off_lag;
    a.off_own = l.off_own;
    a.off_prev = l.off_prev;
    a.off_src = l.off_src;
    a.off_ctl = l.off_ctl;
    const int threads = a.cap_p <= kStickyFewPartitions ? kStickyFewThreads : kStickyThreads;
    return launch_resident_lds<sticky_kernel, kStickyMaxLdsBytes>(c.n_topics, threads, l.bytes, stream, a);
}

}  // namespace la
