// lag_based_partition_assignor.cpp -- see the header.  Host-side container/string work only;
// all arithmetic goes through the C ABI (include/lagassign.h) to the HIP kernels.
#include "lag_based_partition_assignor.hpp"

#include <cctype>

#include <algorithm>
#include <functional>
#include <mutex>
#include <numeric>
#include <unordered_map>

#include "../../../include/lagassign.h"
#include "java_compat.hpp"

namespace kafka_lag {

namespace {

// One process-wide native context for the static entry points (the reference's statics carry
// no state either); guarded because la_ctx is single-threaded.
std::mutex g_ctx_mutex;
la_ctx* g_ctx = nullptr;

la_ctx* shared_ctx_locked() {
    if (!g_ctx) {
        int rc = la_create_multi(&g_ctx, 0, nullptr, 0);      // every GPU of the node, like the Java host
        if (rc != LA_OK) {
            g_ctx = nullptr;
            throw std::runtime_error(std::string("liblagassign: ") + la_last_error(nullptr));
        }
    }
    return g_ctx;
}

// Whether the list order of the last static assign() on this thread is the modelled HashMap's exact order
// (false: a bucket of consumersPerTopic reached tree-bin size: the order is java_compat.hpp's restatement of TreeNode's list
// handling, unverified against a JVM).
thread_local bool t_last_order_exact = true;
thread_local LagBasedPartitionAssignor::NativeCallStats t_last_native;
thread_local LagBasedPartitionAssignor::MemberLoads t_last_loads;
thread_local LagBasedPartitionAssignor::CooperativeRound t_last_coop;

void check(la_ctx* ctx, int rc) {
    if (rc == LA_OK) return;
    const std::string msg = std::string("liblagassign error ") + std::to_string(rc) + ": " + la_last_error(ctx);
    if (rc == LA_EINVAL) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
}

// The subscription side of one rebalance, resolved to ranks and topic order.
struct Plan {
    std::vector<std::string> members;              // unique memberIds, caller's iteration order
    std::vector<int32_t> rank_of_member;           // String.compareTo rank of members[i]
    std::vector<int> member_of_rank;
    std::vector<std::string> topics;               // consumersPerTopic.entrySet() order
    std::vector<std::vector<int32_t>> topic_ranks; // per topic: sorted unique subscriber ranks
    std::vector<std::vector<int>> topic_members;   // per topic: subscriber member indices in consumers-list order
    bool order_exact = true;
};

Plan make_plan(const GroupSubscription& subscriptions) {
    Plan p;
    std::unordered_map<std::string, int> member_index;
    std::vector<const std::vector<std::string>*> member_topics;
    for (const auto& kv : subscriptions) {                      // a Map has unique keys: last wins
        auto it = member_index.find(kv.first);
        if (it == member_index.end()) {
            member_index.emplace(kv.first, (int)p.members.size());
            p.members.push_back(kv.first);
            member_topics.push_back(&kv.second);
        } else {
            member_topics[it->second] = &kv.second;
        }
    }
    p.rank_of_member = rankMembers(p.members);
    p.member_of_rank.assign(p.members.size(), 0);
    for (size_t i = 0; i < p.members.size(); ++i) p.member_of_rank[p.rank_of_member[i]] = (int)i;

    // consumersPerTopic, Main.java:410-426: HashMap + computeIfAbsent, walked in entry order
    JavaHashMapOrder order;
    std::unordered_map<std::string, int> topic_index;
    std::vector<std::string> names;
    std::vector<std::vector<int32_t>> ranks;
    std::vector<std::vector<int>> members_of;
    for (size_t m = 0; m < p.members.size(); ++m) {
        for (const std::string& topic : *member_topics[m]) {
            auto it = topic_index.find(topic);
            int ti;
            if (it == topic_index.end()) {
                ti = (int)names.size();
                topic_index.emplace(topic, ti);
                names.push_back(topic);
                ranks.emplace_back();
                members_of.emplace_back();
                order.compute_if_absent_new(ti, topic);
            } else {
                ti = it->second;
            }
            ranks[ti].push_back(p.rank_of_member[m]);          // duplicates allowed here ...
            members_of[ti].push_back((int)m);
        }
    }
    for (int ti : order.order()) {
        std::vector<int32_t> r = ranks[ti];
        std::sort(r.begin(), r.end());
        r.erase(std::unique(r.begin(), r.end()), r.end());     // ... the keyed bins de-dup, Main.java:216-225
        p.topics.push_back(names[ti]);
        p.topic_ranks.push_back(std::move(r));
        p.topic_members.push_back(members_of[ti]);
    }
    p.order_exact = order.order_exact();
    return p;
}

// Per-topic partition data in SoA form, ready for the C ABI.
struct TopicData {
    std::vector<int32_t> partition;
    std::vector<std::string> element_topic;   // TopicPartitionLag.topic of each element (Main.java:264)
    std::vector<int64_t> lag;                 // lag mode
    std::vector<int64_t> begin, end, committed;   // offset mode
};

struct Flat {
    std::vector<int64_t> part_off{0}, cons_off{0};
    std::vector<int32_t> pid, cons_rank;
    std::vector<int64_t> lag, end, committed;
    // the beginning offset is read only where a partition has no committed offset (Main.java:384-396): it crosses the
    // boundary as (position, begin) pairs for those partitions alone (la_assign_batch_grouped_sparse)
    std::vector<int64_t> none_index, none_begin;
    // what the marshalling loop sees on its way (Main.java:344-356 walks every partition's offsets): the largest end offset /
    // lag and partition id, and whether any offset, lag or id is negative -- la_hint_next_call's bounds
    int64_t max_value = 0, max_id = 0;
    bool any_negative = false;
    void see(int64_t value, int32_t id) {
        if (value > max_value) max_value = value;
        if (id > max_id) max_id = id;
        any_negative |= (value < 0) | (id < 0);
    }
};

// The bounds of the next call, when the marshaller can vouch for them: with no negative offset a lag never exceeds its end
// offset (computePartitionLag, Main.java:376-404: end - committed / end - begin / 0, clamped at 0).  One launch per chunk of
// tile-sized topics instead of two; a caller that saw a negative value promises nothing.
void hint_bounds(la_ctx* ctx, const Flat& f) {
    t_last_native = LagBasedPartitionAssignor::NativeCallStats{};
    t_last_loads = LagBasedPartitionAssignor::MemberLoads{};     // (a call that fails leaves no roll-up of an earlier one behind)
    if (f.any_negative || f.pid.empty()) return;
    la_call_hints h{};
    h.struct_size = (int32_t)sizeof h;
    h.flags = LA_HINT_BOUNDS;
    h.max_lag = f.max_value;
    h.max_partition_id = f.max_id;
    if (la_hint_next_call(ctx, &h) != LA_OK) return;          // a refused hint is no hint: the call itself decides
    t_last_native.hinted = true;
    t_last_native.max_lag = h.max_lag;
    t_last_native.max_partition_id = h.max_partition_id;
}

Assignment run_native(const Plan& plan, const std::vector<const TopicData*>& data, bool offsets_mode,
                      int32_t reset_mode, std::map<std::string, std::map<std::string, int64_t>>* totals_out,
                      const std::function<void(const std::string&)>* debug = nullptr, const OwnedArrays* owned = nullptr,
                      bool sticky = false, bool sticky_large = false, bool pinned = false, bool pinned_large = false) {
    Flat f;
    for (size_t t = 0; t < plan.topics.size(); ++t) {
        const TopicData* d = data[t];
        if (d) {
            f.pid.insert(f.pid.end(), d->partition.begin(), d->partition.end());
            if (offsets_mode) {
                const int64_t base = (int64_t)f.end.size();
                for (size_t i = 0; i < d->committed.size(); ++i) {
                    f.see(d->end[i], d->partition[i]);
                    if (d->committed[i] < 0) {                        // partitionMetadata == null, Main.java:384
                        f.none_index.push_back(base + (int64_t)i);
                        f.none_begin.push_back(d->begin[i]);
                        f.any_negative |= d->begin[i] < 0;
                    }
                }
                f.end.insert(f.end.end(), d->end.begin(), d->end.end());
                f.committed.insert(f.committed.end(), d->committed.begin(), d->committed.end());
            } else {
                for (size_t i = 0; i < d->lag.size(); ++i) f.see(d->lag[i], d->partition[i]);
                f.lag.insert(f.lag.end(), d->lag.begin(), d->lag.end());
            }
        }
        f.part_off.push_back((int64_t)f.pid.size());
        f.cons_rank.insert(f.cons_rank.end(), plan.topic_ranks[t].begin(), plan.topic_ranks[t].end());
        f.cons_off.push_back((int64_t)f.cons_rank.size());
    }
    const size_t n = f.pid.size(), k = f.cons_rank.size();
    // The assignment stays on the device (out_partition = out_member_rank = NULL) and crosses PCIe once, already
    // grouped: every member's list in the reference's order (topic by topic as consumersPerTopic iterates, inside a
    // topic in assignment order, Main.java:171-174 and :264); the host only wraps it.
    std::vector<int64_t> out_total(k);
    const int32_t n_members = (int32_t)plan.members.size();
    std::vector<int64_t> member_off((size_t)n_members + 1, 0);
    std::vector<int32_t> grouped_topic(n), grouped_pid(n);
    // assignCooperative: the lists above are those of the ADJUSTED assignment; the target itself (for the roll-up) and, with the
    // debug hook set, its eager lists (for the summary) come beside them
    std::vector<int32_t> target_pid(owned ? n : 0), target_rank(owned ? n : 0), eager_topic, eager_pid;
    std::vector<int64_t> eager_off;
    if (owned) t_last_coop = LagBasedPartitionAssignor::CooperativeRound{};
    if (owned && !plan.topics.empty()) {
        const size_t M = (size_t)n_members, T = plan.topics.size();
        std::vector<int64_t> counts(4 * M), withheld(T), summary(6);
        std::lock_guard<std::mutex> lock(g_ctx_mutex);
        la_ctx* ctx = shared_ctx_locked();
        hint_bounds(ctx, f);
        la_assign_coop_args a{};
        a.struct_size = (int32_t)sizeof a;
        a.n_topics = (int32_t)T;
        a.reset_mode = reset_mode;
        a.part_off = f.part_off.data();
        a.partition_id = f.pid.data();
        a.end_off = f.end.data();                                // begin_off stays NULL: the sparse list
        a.committed_off = f.committed.data();
        a.n_none = (int64_t)f.none_index.size();
        a.none_index = f.none_index.data();
        a.none_begin = f.none_begin.data();
        a.cons_off = f.cons_off.data();
        a.cons_rank = f.cons_rank.data();
        a.n_members = n_members;
        a.n_owned = (int64_t)owned->topic.size();
        a.owned_member_off = owned->member_off.data();
        a.owned_topic = owned->topic.data();
        a.owned_partition = owned->partition.data();
        a.member_off = member_off.data();
        a.grouped_topic = grouped_topic.data();
        a.grouped_partition = grouped_pid.data();
        a.out_total_lag = out_total.data();
        a.out_partition = target_pid.data();
        a.out_member_rank = target_rank.data();
        a.member_kept = counts.data();
        a.member_fresh = counts.data() + M;
        a.member_pending = counts.data() + 2 * M;
        a.member_release = counts.data() + 3 * M;
        a.topic_withheld = withheld.data();
        a.summary = summary.data();
        std::vector<int64_t> sticky_summary(4, 0);
        if (pinned) {
            // lag.assignor.cooperative.followup = pinned, and this IS a follow-up: what is owned stays, only the rest is dealt
            // out (LA_COOP_PINNED; the sticky entry does not take the flag, and there is nothing left for it to re-match).  A
            // topic over the limits, should one get here, sends the call through the full form below.
            a.flags |= LA_COOP_PINNED | (pinned_large ? LA_COOP_PINNED_LARGE : 0);      // (.followup.large: topics of any size)
            const int rc = la_assign_batch_cooperative(ctx, &a);
            if (rc == LA_ESHAPE) {
                pinned = false;
                a.flags &= ~(LA_COOP_PINNED | LA_COOP_PINNED_LARGE);
                hint_bounds(ctx, f);
            } else {
                check(ctx, rc);
            }
        }
        if (!pinned && sticky) {                                 // lag.assignor.sticky.ties: the lists are those of the sticky order
            la_assign_sticky_args sa{};
            sa.struct_size = (int32_t)sizeof sa;
            sa.coop = a;
            if (sticky_large) sa.coop.flags |= LA_COOP_STICKY_LARGE;      // lag.assignor.sticky.ties.large: topics of any size
            sa.sticky_summary = sticky_summary.data();
            check(ctx, la_assign_batch_cooperative_sticky(ctx, &sa));
        } else if (!pinned) {
            check(ctx, la_assign_batch_cooperative(ctx, &a));
        }
        t_last_native.pipeline = la_last_pipeline(ctx);
        t_last_native.launches = la_last_launches(ctx);
        if (debug && *debug) {                                   // (only then: the target's eager lists)
            eager_off.assign(M + 1, 0);
            eager_topic.resize(n);
            eager_pid.resize(n);
            if (pinned) {
                // the pinned call keeps nothing on the device: the same stable grouping by rank, from the target it returned
                std::vector<int64_t> at(M + 2, 0);               // [0]: nobody's, [r + 1]: member r's
                for (size_t i = 0; i < n; ++i) ++at[(size_t)(target_rank[i] + 1) + 1];
                for (size_t r = 1; r < M + 2; ++r) at[r] += at[r - 1];
                for (size_t r = 0; r <= M; ++r) eager_off[r] = at[r + 1];
                for (size_t t = 0; t < T; ++t)
                    for (int64_t i = f.part_off[t]; i < f.part_off[t + 1]; ++i) {
                        const int64_t j = at[(size_t)(target_rank[(size_t)i] + 1)]++;
                        eager_topic[(size_t)j] = (int32_t)t;
                        eager_pid[(size_t)j] = target_pid[(size_t)i];
                    }
            } else if (n > 0) {                                  // still on the device
                check(ctx, la_group_last_by_member(ctx, n_members, eager_off.data(), eager_topic.data(), eager_pid.data()));
            }
        }
        for (size_t r = 0; r < M; ++r)
            t_last_coop.per_member[plan.members[plan.member_of_rank[r]]] = {counts[r], counts[M + r], counts[2 * M + r], counts[3 * M + r]};
        for (size_t t = 0; t < T; ++t) t_last_coop.topic_withheld[plan.topics[t]] = withheld[t];
        t_last_coop.kept = summary[0]; t_last_coop.fresh = summary[1]; t_last_coop.withheld = summary[2];
        t_last_coop.dropped = summary[3]; t_last_coop.stale = summary[4]; t_last_coop.followup = summary[5] != 0;
        t_last_coop.sticky_kept_before = sticky_summary[0]; t_last_coop.sticky_kept_after = sticky_summary[1];
        t_last_coop.sticky_topics_passed_through = sticky_summary[3];
        // a pinned target keeps exactly its pinned partitions, and its foreign ones are what the round withholds or drops
        t_last_coop.pinned = pinned;
        t_last_coop.pinned_free = pinned ? (int64_t)n - summary[0] : 0;
        t_last_coop.pinned_foreign = pinned ? summary[2] + summary[3] : 0;
    } else if (!plan.topics.empty()) {
        std::lock_guard<std::mutex> lock(g_ctx_mutex);       // one lock over both calls: the second reads the first's results
        la_ctx* ctx = shared_ctx_locked();
        hint_bounds(ctx, f);
        if (offsets_mode) {
            // assign(Cluster, GroupSubscription): both steps in ONE native call -- for a rebalance of ordinary size one
            // upload, one download, one wait (la_assign_batch_grouped_sparse: `begin` only where it is read)
            check(ctx, la_assign_batch_grouped_sparse(ctx, (int32_t)plan.topics.size(), f.part_off.data(), f.pid.data(),
                                                      f.end.data(), f.committed.data(), reset_mode,
                                                      (int64_t)f.none_index.size(), f.none_index.data(), f.none_begin.data(),
                                                      f.cons_off.data(), f.cons_rank.data(), n_members, member_off.data(),
                                                      grouped_topic.data(), grouped_pid.data(), out_total.data()));
        } else {
            check(ctx, la_assign_batch_lags(ctx, (int32_t)plan.topics.size(), f.part_off.data(), f.pid.data(), f.lag.data(),
                                            f.cons_off.data(), f.cons_rank.data(), nullptr, nullptr, out_total.data()));
            t_last_native.pipeline = la_last_pipeline(ctx);
            t_last_native.launches = la_last_launches(ctx);
            check(ctx, la_group_last_by_member(ctx, n_members, member_off.data(), grouped_topic.data(), grouped_pid.data()));
            t_last_native.launches += la_last_launches(ctx);
        }
        if (offsets_mode) {
            t_last_native.pipeline = la_last_pipeline(ctx);
            t_last_native.launches = la_last_launches(ctx);
        }
    }
    // the call's roll-up per member (lastMemberLoads): counts from the lists' offsets, lags as wrapping sums of the K totals
    {
        LagBasedPartitionAssignor::MemberLoads loads;
        std::vector<uint64_t> lag_of((size_t)n_members, 0);
        for (size_t c = 0; c < k; ++c) lag_of[(size_t)f.cons_rank[c]] += (uint64_t)out_total[c];
        std::vector<int64_t> held((size_t)n_members + 1, 0);     // [0]: nobody's.  Of the TARGET: from its ranks where the lists are adjusted ones
        if (owned)
            for (size_t i = 0; i < n; ++i) ++held[(size_t)(target_rank[i] + 1)];
        else
            for (int32_t r = 0; r <= n_members; ++r) held[(size_t)r] = r == 0 ? member_off[0] : member_off[r] - member_off[r - 1];
        for (int32_t r = 0; r < n_members; ++r)
            loads.per_member[plan.members[plan.member_of_rank[r]]] = {held[(size_t)r + 1], (int64_t)lag_of[(size_t)r]};
        loads.unassigned = held[0];
        t_last_loads = std::move(loads);
    }
    // partition id -> the element's own topic string (normally the map key), per topic
    std::vector<std::unordered_map<int32_t, const std::string*>> topic_of(plan.topics.size());
    for (size_t t = 0; t < plan.topics.size(); ++t)
        if (const TopicData* d = data[t])
            for (size_t i = 0; i < d->partition.size(); ++i) topic_of[t].emplace(d->partition[i], &d->element_topic[i]);
    Assignment assignment;
    for (int32_t r = 0; r < n_members; ++r) {
        auto& list = assignment[plan.members[plan.member_of_rank[r]]];     // a list for EVERY member, :171-174
        for (int64_t j = member_off[r]; j < member_off[r + 1]; ++j)
            list.push_back(TopicPartition{*topic_of[grouped_topic[j]].at(grouped_pid[j]), grouped_pid[j]});   // :264
    }
    if (debug && *debug && (!owned || !eager_off.empty())) {
        // Main.java:279-306.  consumerTotalLags is a HashMap filled with put() in consumers-list order (:216-225).
        // (after assignCooperative the message describes the target: its eager lists)
        const std::vector<int64_t>& d_off = owned ? eager_off : member_off;
        const std::vector<int32_t>&d_topic = owned ? eager_topic : grouped_topic, &d_pid = owned ? eager_pid : grouped_pid;
        for (size_t t = 0; t < plan.topics.size(); ++t) {
            JavaHashMapOrder order(plan.topic_members[t].size());          // new HashMap<>(consumers.size()), :216
            std::vector<int> uniq;
            for (int m : plan.topic_members[t])
                if (std::find(uniq.begin(), uniq.end(), m) == uniq.end()) {
                    order.put_new((int)uniq.size(), plan.members[m]);
                    uniq.push_back(m);
                }
            std::string summary;
            for (int u : order.order()) {
                const int m = uniq[u];
                const int32_t r = plan.rank_of_member[m];
                int64_t total = 0;
                for (int64_t c = f.cons_off[t]; c < f.cons_off[t + 1]; ++c)
                    if (f.cons_rank[c] == r) total = out_total[c];
                summary += "\t" + plan.members[m] + " (total_lag=" + std::to_string(total) + ")\n";
                for (int64_t j = d_off[r]; j < d_off[r + 1]; ++j) {
                    if ((size_t)d_topic[j] > t) break;                     // the map as it stood after this topic
                    summary += "\t\t" + *topic_of[d_topic[j]].at(d_pid[j]) + "-" +
                               std::to_string(d_pid[j]) + "\n";          // TopicPartition.toString()
                }
            }
            (*debug)("Assignment for " + plan.topics[t] + ":\n" + summary);
        }
    }
    if (totals_out) {
        for (size_t t = 0; t < plan.topics.size(); ++t) {
            auto& per = (*totals_out)[plan.topics[t]];
            for (int64_t c = f.cons_off[t]; c < f.cons_off[t + 1]; ++c)
                per[plan.members[plan.member_of_rank[f.cons_rank[c]]]] = out_total[c];
        }
    }
    return assignment;
}

}  // namespace

// String.compareTo ranks (0 = smallest).  Equal ids share a rank slot order by position, but
// callers pass unique ids.
std::vector<int32_t> rankMembers(const std::vector<std::string>& memberIds) {
    std::vector<std::u16string> u;
    u.reserve(memberIds.size());
    for (const auto& m : memberIds) u.push_back(utf8_to_utf16(m));
    std::vector<int> idx(memberIds.size());
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return java_compare(u[a], u[b]) < 0; });
    std::vector<int32_t> rank(memberIds.size());
    for (size_t r = 0; r < idx.size(); ++r) rank[idx[r]] = (int32_t)r;
    return rank;
}

std::vector<std::string> consumersPerTopicOrder(const GroupSubscription& subscriptions) {
    return make_plan(subscriptions).topics;
}

bool LagBasedPartitionAssignor::lastStaticOrderExact() { return t_last_order_exact; }
LagBasedPartitionAssignor::NativeCallStats LagBasedPartitionAssignor::lastNativeCall() { return t_last_native; }
LagBasedPartitionAssignor::MemberLoads LagBasedPartitionAssignor::lastMemberLoads() { return t_last_loads; }

LagBasedPartitionAssignor::LagBasedPartitionAssignor() = default;
LagBasedPartitionAssignor::~LagBasedPartitionAssignor() = default;

void LagBasedPartitionAssignor::configure(const std::map<std::string, std::string>& configs) {
    consumer_group_props_ = configs;                                             // Main.java:101-104
    auto gid = consumer_group_props_.find("group.id");
    if (gid == consumer_group_props_.end())                                      // :107-113
        throw std::invalid_argument("group.id cannot be null when using partition.assignment.strategy=" +
                                    std::string("LagBasedPartitionAssignor"));
    metadata_consumer_props_ = consumer_group_props_;                            // :116-120
    metadata_consumer_props_["enable.auto.commit"] = "false";
    metadata_consumer_props_["client.id"] = gid->second + ".assignor";
    // lag.assignor.sticky.ties: a boolean as Boolean.parseBoolean reads it ("true" in any case), default false -- whether
    // assignCooperative keeps partitions of equal lag with their previous owner (la_assign_batch_cooperative_sticky)
    auto sticky = consumer_group_props_.find("lag.assignor.sticky.ties");
    sticky_ties_ = false;
    if (sticky != consumer_group_props_.end()) {
        std::string v = sticky->second;
        for (char& ch : v) ch = (char)std::tolower((unsigned char)ch);
        sticky_ties_ = v == "true";
    }
    // lag.assignor.sticky.ties.large: read the same way, default false, no effect unless the key above is on -- topics of more
    // than 4096 partitions are re-matched too (LA_COOP_STICKY_LARGE) instead of keeping the reference's order
    auto sticky_large = consumer_group_props_.find("lag.assignor.sticky.ties.large");
    sticky_ties_large_ = false;
    if (sticky_large != consumer_group_props_.end()) {
        std::string v = sticky_large->second;
        for (char& ch : v) ch = (char)std::tolower((unsigned char)ch);
        sticky_ties_large_ = v == "true";
    }
    // lag.assignor.cooperative.followup: "full" (the default: every rebalance computes the reference's assignment over fresh
    // lags) or "pinned" -- a follow-up rebalance deals out only what nobody owns (LA_COOP_PINNED), so that it settles
    auto followup = consumer_group_props_.find("lag.assignor.cooperative.followup");
    followup_pinned_ = false;
    if (followup != consumer_group_props_.end()) {
        std::string v = followup->second;
        for (char& ch : v) ch = (char)std::tolower((unsigned char)ch);
        if (v != "full" && v != "pinned")
            throw std::invalid_argument("lag.assignor.cooperative.followup must be full or pinned, not " + followup->second);
        followup_pinned_ = v == "pinned";
    }
    // lag.assignor.cooperative.followup.large: false (the default) or true -- the pinned follow-up takes topics of up to
    // LA_PINNED_LARGE_MAX_PARTITIONS partitions (LA_COOP_PINNED_LARGE) instead of falling back to the full form from 4097 on;
    // no effect unless the key above is "pinned"
    auto followup_large = consumer_group_props_.find("lag.assignor.cooperative.followup.large");
    followup_pinned_large_ = false;
    if (followup_large != consumer_group_props_.end()) {
        std::string v = followup_large->second;
        for (char& ch : v) ch = (char)std::tolower((unsigned char)ch);
        if (v != "false" && v != "true")
            throw std::invalid_argument("lag.assignor.cooperative.followup.large must be false or true, not " + followup_large->second);
        followup_pinned_large_ = v == "true";
    }
    last_followup_ = false;
    last_subscription_.clear();
}

int64_t LagBasedPartitionAssignor::computePartitionLag(const std::optional<OffsetAndMetadata>& partitionMetadata,
                                                       int64_t beginOffset, int64_t endOffset,
                                                       const std::string& autoOffsetResetMode) {
    const int64_t committed = partitionMetadata ? partitionMetadata->offset : LA_NO_COMMITTED;
    const int32_t mode = equals_ignore_case_latest(autoOffsetResetMode) ? LA_RESET_LATEST : LA_RESET_EARLIEST;
    int64_t lag = 0;
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    la_ctx* ctx = shared_ctx_locked();
    check(ctx, la_compute_lag(ctx, 1, &beginOffset, &endOffset, &committed, mode, &lag));
    return lag;
}

Assignment LagBasedPartitionAssignor::assign(const OrderedMap<std::vector<TopicPartitionLag>>& partitionLagPerTopic,
                                             const GroupSubscription& subscriptions) {
    const Plan plan = make_plan(subscriptions);
    std::unordered_map<std::string, TopicData> by_topic;
    for (const auto& kv : partitionLagPerTopic) {
        TopicData d;
        for (const TopicPartitionLag& e : kv.second) {
            d.partition.push_back(e.partition);
            d.element_topic.push_back(e.topic);
            d.lag.push_back(e.lag);
        }
        by_topic[kv.first] = std::move(d);                                       // later duplicate key wins
    }
    std::vector<const TopicData*> data;
    for (const std::string& t : plan.topics) {
        auto it = by_topic.find(t);
        data.push_back(it == by_topic.end() ? nullptr : &it->second);            // getOrDefault(..., emptyList()), :182
    }
    t_last_order_exact = plan.order_exact;
    return run_native(plan, data, false, LA_RESET_LATEST, nullptr);
}

LagBasedPartitionAssignor::CooperativeRound LagBasedPartitionAssignor::lastCooperativeRound() { return t_last_coop; }

OwnedArrays cooperativeOwnedArrays(const std::vector<std::string>& memberIds, const std::vector<std::string>& topics,
                                   const std::vector<std::vector<TopicPartition>>& ownedPerMember) {
    if (ownedPerMember.size() != memberIds.size()) throw std::invalid_argument("one owned list per member");
    std::unordered_map<std::string, int32_t> topic_index;
    for (size_t t = 0; t < topics.size(); ++t) topic_index.emplace(topics[t], (int32_t)t);
    const std::vector<int32_t> rank = rankMembers(memberIds);
    std::vector<size_t> member_of_rank(memberIds.size());
    for (size_t i = 0; i < memberIds.size(); ++i) member_of_rank[(size_t)rank[i]] = i;
    OwnedArrays o;
    o.member_off.push_back(0);
    for (size_t r = 0; r < memberIds.size(); ++r) {              // in rank order: the layout la_group_by_member writes
        for (const TopicPartition& tp : ownedPerMember[member_of_rank[r]]) {
            auto it = topic_index.find(tp.topic);
            o.topic.push_back(it == topic_index.end() ? -1 : it->second);    // not in this rebalance: a stale claim
            o.partition.push_back(tp.partition);
        }
        o.member_off.push_back((int64_t)o.topic.size());
    }
    return o;
}

Assignment LagBasedPartitionAssignor::assign(const Cluster& metadata, const GroupSubscription& subscriptions,
                                             OffsetSource& offsets) {
    return assignImpl(metadata, subscriptions, offsets, nullptr);
}

Assignment LagBasedPartitionAssignor::assignCooperative(const Cluster& metadata, const CooperativeSubscription& subscriptions,
                                                        OffsetSource& offsets) {
    GroupSubscription topics;
    OrderedMap<std::vector<TopicPartition>> owned;
    for (const auto& kv : subscriptions) {
        topics.emplace_back(kv.first, kv.second.topics);
        owned.emplace_back(kv.first, kv.second.ownedPartitions);
    }
    return assignImpl(metadata, topics, offsets, &owned);
}

Assignment LagBasedPartitionAssignor::assignImpl(const Cluster& metadata, const GroupSubscription& subscriptions,
                                                 OffsetSource& offsets, const OrderedMap<std::vector<TopicPartition>>* owned) {
    // Everything is cold when a rebalance comes (Kafka calls the leader's assign() minutes apart): la_wake runs a one-partition
    // rebalance through the real path NOW (~95 us, cold) -- the three broker round trips below (Main.java:147 -> :317-365)
    // take milliseconds before there is an offset to hand over, and the call that matters then runs warm (at the C ABI a
    // 100-partition call 34 us instead of 85, profiles/r06_p_cold_c.txt).  Best effort: a failure here is the assign call's to report.
    {
        std::lock_guard<std::mutex> lock(g_ctx_mutex);
        try { (void)la_wake(shared_ctx_locked()); } catch (const std::exception&) {}
    }
    // topicSubscriptions is a HashMap<memberId, topics> filled with put (Main.java:141-146);
    // the static assign then walks it in HashMap order.
    GroupSubscription hashed;
    {
        JavaHashMapOrder order;
        std::unordered_map<std::string, int> seen;
        std::vector<const std::pair<std::string, std::vector<std::string>>*> entries;
        for (const auto& kv : subscriptions) {
            auto it = seen.find(kv.first);
            if (it == seen.end()) {
                seen.emplace(kv.first, (int)entries.size());
                order.put_new((int)entries.size(), kv.first);
                entries.push_back(&kv);
            } else {
                entries[it->second] = &kv;
            }
        }
        for (int i : order.order()) hashed.push_back(*entries[i]);
        last_order_exact_ = order.order_exact();
    }
    const Plan plan = make_plan(hashed);
    last_order_exact_ = last_order_exact_ && plan.order_exact;
    if (!last_order_exact_)
        warn("a HashMap bucket reached tree-bin size (>= 9 colliding keys in a >= 64-slot table): the list order follows the "
             "C++ host's restatement of java.util.HashMap's tree bins, which no JVM has confirmed here; the partition -> "
             "member map is unaffected");

    // readTopicPartitionLags, Main.java:317-365 -- batched: one request per kind for all topics
    std::vector<TopicPartition> all;
    std::unordered_map<std::string, TopicData> by_topic;
    for (const std::string& topic : plan.topics) {
        auto it = metadata.find(topic);
        if (it == metadata.end() || it->second.empty()) {
            warn("Skipping assignment for topic " + topic + " since no metadata is available");   // :359
            continue;
        }
        TopicData d;
        for (int32_t p : it->second) {
            d.partition.push_back(p);
            d.element_topic.push_back(topic);
            all.push_back(TopicPartition{topic, p});
        }
        by_topic[topic] = std::move(d);
    }
    const auto begin = offsets.beginningOffsets(all);                            // :339
    const auto end = offsets.endOffsets(all);                                    // :340
    const auto committed = offsets.committed(all);                               // :342
    for (auto& kv : by_topic) {
        TopicData& d = kv.second;
        for (int32_t p : d.partition) {
            const TopicPartition tp{kv.first, p};
            auto b = begin.find(tp);
            auto e = end.find(tp);
            auto c = committed.find(tp);
            d.begin.push_back(b == begin.end() ? 0 : b->second);                 // getOrDefault(.., 0L), :350
            d.end.push_back(e == end.end() ? 0 : e->second);                     // :351
            d.committed.push_back(c == committed.end() || !c->second ? LA_NO_COMMITTED : c->second->offset);
        }
    }
    auto mode_it = consumer_group_props_.find("auto.offset.reset");              // default "latest", :346-347
    const std::string mode = mode_it == consumer_group_props_.end() ? "latest" : mode_it->second;
    const int32_t reset = equals_ignore_case_latest(mode) ? LA_RESET_LATEST : LA_RESET_EARLIEST;

    std::vector<const TopicData*> data;
    for (const std::string& t : plan.topics) {
        auto it = by_topic.find(t);
        data.push_back(it == by_topic.end() ? nullptr : &it->second);
    }
    last_totals_.clear();
    if (owned) {
        // what every member owns, in the plan's member order (a Map has unique keys: the last entry of a member wins, as above)
        std::unordered_map<std::string, const std::vector<TopicPartition>*> of;
        for (const auto& kv : *owned) of[kv.first] = &kv.second;
        std::vector<std::vector<TopicPartition>> per_member;
        for (const std::string& m : plan.members) per_member.push_back(*of.at(m));
        const OwnedArrays arrays = cooperativeOwnedArrays(plan.members, plan.topics, per_member);
        // lag.assignor.cooperative.followup = pinned: this rebalance is the follow-up of the last one when that one asked for
        // it and the group is the same -- member ids and every member's topic list -- and the pinned form takes every topic
        std::map<std::string, std::vector<std::string>> subscription;
        for (const auto& kv : hashed) subscription[kv.first] = kv.second;
        bool pinned = followup_pinned_ && last_followup_ && subscription == last_subscription_;
        for (size_t t = 0; pinned && t < plan.topics.size(); ++t)
            pinned = (!data[t] || data[t]->partition.size() <= (followup_pinned_large_ ? (size_t)LA_PINNED_LARGE_MAX_PARTITIONS
                                                                                        : (size_t)LA_PINNED_MAX_PARTITIONS)) &&
                     plan.topic_ranks[t].size() <= (size_t)LA_PINNED_MAX_CONSUMERS;
        last_followup_ = false;                                      // (a call that throws leaves no follow-up behind)
        Assignment assignment = run_native(plan, data, true, reset, &last_totals_, &debug, &arrays, sticky_ties_,
                                           sticky_ties_ && sticky_ties_large_, pinned, pinned && followup_pinned_large_);
        last_followup_ = t_last_coop.followup;
        last_subscription_ = std::move(subscription);
        return assignment;
    }
    return run_native(plan, data, true, reset, &last_totals_, &debug);           // wrap: :152-156
}

}  // namespace kafka_lag
