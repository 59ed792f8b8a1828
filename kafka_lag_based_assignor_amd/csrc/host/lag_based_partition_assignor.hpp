// lag_based_partition_assignor.hpp -- C++ host mirror of the reference's plugin class.
//
// The real drop-in host is Java (java/ in this repo, JNI over include/lagassign.h); no JVM
// exists in the build image, so this C++ class is the host that is compiled, run and tested
// here.  It keeps the reference's names, argument meaning and error behaviour:
//
//   reference (Main.java)                                   here
//   ------------------------------------------------------  ------------------------------------
//   class LagBasedPartitionAssignor            :83          kafka_lag::LagBasedPartitionAssignor
//   void configure(Map<String,?>)              :97-130      configure(map)   throws invalid_argument
//   String name() -> "lag"                     :132-135     name()
//   GroupAssignment assign(Cluster, GroupSubscription)      assign(cluster, subscriptions)
//                                              :137-157
//   static assign(Map lags, Map subscriptions) :166-188     static assign(lags, subscriptions)
//   static computePartitionLag(...)            :376-404     static computePartitionLag(...)
//   readTopicPartitionLags                     :317-365     (inside assign; ONE batched offset
//                                                            request for all topics)
//   TopicPartitionLag                          :431-455     struct TopicPartitionLag
//
// Everything string- or container-shaped happens here; every number is computed by the HIP
// kernels behind the C ABI (there is no host arithmetic fallback).
#pragma once
#include <array>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace kafka_lag {

struct TopicPartition {
    std::string topic;
    int32_t partition = 0;
    bool operator==(const TopicPartition& o) const { return partition == o.partition && topic == o.topic; }
    bool operator<(const TopicPartition& o) const { return topic != o.topic ? topic < o.topic : partition < o.partition; }
};

struct TopicPartitionLag {                    // Main.java:431-455
    std::string topic;
    int32_t partition = 0;
    int64_t lag = 0;
};

struct OffsetAndMetadata {                    // org.apache.kafka.clients.consumer.OffsetAndMetadata
    int64_t offset = 0;
    explicit OffsetAndMetadata(int64_t off) : offset(off) {
        if (off < 0) throw std::invalid_argument("Invalid negative offset");   // as the Kafka class does
    }
};

// Insertion-ordered String -> V map: what the caller's java.util.Map iterates like.
template <typename V>
using OrderedMap = std::vector<std::pair<std::string, V>>;

// Stand-in for the side KafkaConsumer the reference builds lazily (Main.java:89, :322-324).
// One call per kind for ALL requested partitions (the reference issues three per topic).
struct OffsetSource {
    virtual ~OffsetSource() = default;
    // Missing keys mean "lookup failed" and default to 0 (Main.java:350-351).
    virtual std::map<TopicPartition, int64_t> beginningOffsets(const std::vector<TopicPartition>& tps) = 0;
    virtual std::map<TopicPartition, int64_t> endOffsets(const std::vector<TopicPartition>& tps) = 0;
    // Missing keys / nullopt mean "no committed offset" (partitionMetadata == null, :384).
    virtual std::map<TopicPartition, std::optional<OffsetAndMetadata>> committed(const std::vector<TopicPartition>& tps) = 0;
};

// Cluster.partitionsForTopic (Main.java:329): topic -> partition ids; absent or empty = no metadata.
using Cluster = std::map<std::string, std::vector<int32_t>>;
// GroupSubscription: memberId -> subscribed topics, in the caller's iteration order.
using GroupSubscription = OrderedMap<std::vector<std::string>>;
// GroupAssignment / the static assign's result: memberId -> partitions in the reference's list order.
using Assignment = std::map<std::string, std::vector<TopicPartition>>;
// What a member sends when the group speaks the COOPERATIVE protocol (ConsumerPartitionAssignor.Subscription): its topics
// and ownedPartitions() -- what it consumes right now.  Nothing in the reference, whose protocol is eager.
struct MemberSubscription {
    std::vector<std::string> topics;
    std::vector<TopicPartition> ownedPartitions;
};
using CooperativeSubscription = OrderedMap<MemberSubscription>;

class LagBasedPartitionAssignor {
 public:
    LagBasedPartitionAssignor();
    ~LagBasedPartitionAssignor();

    // Main.java:97-130.  Requires group.id (std::invalid_argument == IllegalArgumentException).
    void configure(const std::map<std::string, std::string>& configs);
    std::string name() const { return "lag"; }            // Main.java:132-135

    // Main.java:137-157.  `offsets` plays the metadata consumer.
    Assignment assign(const Cluster& metadata, const GroupSubscription& subscriptions, OffsetSource& offsets);

    // ConsumerPartitionAssignor.supportedProtocols(): cooperative first -- the group picks the first protocol every member
    // supports, so a group of these assignors rebalances cooperatively and one with an eager member still finds EAGER
    // (INTEGRATION.md 3.1, step 1).
    static std::vector<std::string> supportedProtocols() { return {"COOPERATIVE", "EAGER"}; }

    // The cooperative form of assign(Cluster, GroupSubscription): the same plan, offsets and lags, ONE native call
    // (la_assign_batch_cooperative) that also joins every member's ownedPartitions against the new assignment.  Returned is
    // the ADJUSTED assignment -- a partition that changes hands between two live members is in nobody's list this round; its
    // owner revokes it and a follow-up rebalance (lastCooperativeRound().followup) hands it over.  A list for every member.
    // With nothing owned anywhere it is assign().  std::invalid_argument when two members (or one, twice) claim a partition.
    Assignment assignCooperative(const Cluster& metadata, const CooperativeSubscription& subscriptions, OffsetSource& offsets);

    // What the last assignCooperative on the calling thread did.  per_member: memberId -> {kept, fresh, pending, release}
    // (pending: what the follow-up will bring; release: what the member revokes now); topic_withheld: withheld per topic;
    // then the call's totals (stale: owned partitions the new assignment does not have) and whether a follow-up is needed.
    struct CooperativeRound {
        std::map<std::string, std::array<int64_t, 4>> per_member;
        std::map<std::string, int64_t> topic_withheld;
        int64_t kept = 0, fresh = 0, withheld = 0, dropped = 0, stale = 0;
        bool followup = false;
        // lag.assignor.sticky.ties: kept before / after the re-matching of equal-lag partitions (0 / 0 with the key off) and the
        // topics that kept the reference's order although the key is on
        int64_t sticky_kept_before = 0, sticky_kept_after = 0, sticky_topics_passed_through = 0;
        // lag.assignor.cooperative.followup = pinned: whether this call was a pinned follow-up (LA_COOP_PINNED) and, if so, how
        // many partitions it dealt out and how many of those a member that does not consume their topic still claims
        bool pinned = false;
        int64_t pinned_free = 0, pinned_foreign = 0;
    };
    static CooperativeRound lastCooperativeRound();

    // Main.java:166-188 (package-private static in the reference; the seam its tests use).
    static Assignment assign(const OrderedMap<std::vector<TopicPartitionLag>>& partitionLagPerTopic,
                             const GroupSubscription& subscriptions);

    // Main.java:376-404.
    static int64_t computePartitionLag(const std::optional<OffsetAndMetadata>& partitionMetadata,
                                       int64_t beginOffset, int64_t endOffset,
                                       const std::string& autoOffsetResetMode);

    // Properties the side consumer would get (Main.java:116-120), for inspection/tests.
    const std::map<std::string, std::string>& metadataConsumerProps() const { return metadata_consumer_props_; }
    // lag.assignor.sticky.ties as configure() read it (default false)
    bool stickyTies() const { return sticky_ties_; }
    // lag.assignor.sticky.ties.large as configure() read it (default false; it has no effect unless stickyTies())
    bool stickyTiesLarge() const { return sticky_ties_large_; }
    // lag.assignor.cooperative.followup as configure() read it: false = "full" (the default), true = "pinned".  With pinned,
    // assignCooperative deals out only the unowned partitions (la_assign_batch_cooperative with LA_COOP_PINNED) when the
    // previous assignCooperative on this instance reported a follow-up, the member ids and every member's topic list are
    // unchanged since then and no topic exceeds LA_PINNED_MAX_PARTITIONS / LA_PINNED_MAX_CONSUMERS; in every other case, and
    // after an LA_ESHAPE, it is the full form, sticky or not as configured.
    bool cooperativeFollowupPinned() const { return followup_pinned_; }
    // lag.assignor.cooperative.followup.large as configure() read it (default false; it has no effect unless the key above is
    // "pinned"): the partition limit of the pinned follow-up is LA_PINNED_LARGE_MAX_PARTITIONS (LA_COOP_PINNED_LARGE)
    bool cooperativeFollowupPinnedLarge() const { return followup_pinned_large_; }

    // The accessors below describe the TARGET (the eager assignment) after assignCooperative, exactly as after assign().
    // Per-topic consumer totals of the last instance-level assign (the debug summary's
    // numbers, Main.java:279-306): topic -> (memberId -> total lag).
    const std::map<std::string, std::map<std::string, int64_t>>& lastTopicTotals() const { return last_totals_; }

    // List order (parity level P2, SURVEY 8a note 4) follows HashMap iteration order, which this C++ host reproduces
    // with a model of OpenJDK's HashMap (java_compat.hpp), tree bins included since round 5 (treeify / putTreeVal /
    // moveRootToFront / split).  false = the last assign met a bucket that a real HashMap treeifies (>= 9 colliding keys in a
    // >= 64-slot table): who-gets-what is exact as always, and the ORDER of topics inside the members' lists is the one the
    // restated TreeNode code gives -- definite, equal to the oracle's independent restatement, but confirmed by no JVM (none
    // in the image).  The instance-level assign also says so through `warn`.  (The Java host uses the real HashMap.)
    bool lastOrderExact() const { return last_order_exact_; }
    static bool lastStaticOrderExact();            // same, for the last static assign() on the calling thread

    // What the last native assign call on the calling thread was given and did (diagnostics / tests): whether the marshalling
    // loop could vouch for bounds (la_hint_next_call: no negative offset, lag or id) and which, the library's pipeline and the
    // number of kernel launches of the call (la_last_pipeline / la_last_launches).
    struct NativeCallStats {
        bool hinted = false;
        int64_t max_lag = 0, max_partition_id = 0;
        int pipeline = -1;
        int64_t launches = 0;
    };
    static NativeCallStats lastNativeCall();

    // Per-member roll-up of the last assign (either form) on the calling thread: memberId -> (partitions, total lag) over all
    // its topics -- the cross-topic sum of what the debug summary prints per topic (Main.java:283-291), total lag in Java long
    // arithmetic.  Every member of the subscription appears, also one that got nothing (Main.java:171-174).  `unassigned` =
    // partitions of topics without consumers (Main.java:211-213).  Host arithmetic over the K totals of the call; the device
    // form for resident results is la_member_loads_device.
    struct MemberLoads {
        std::map<std::string, std::pair<int64_t, int64_t>> per_member;
        int64_t unassigned = 0;
    };
    static MemberLoads lastMemberLoads();

    // Hook for log lines the reference emits through slf4j (warn on missing metadata, :359).
    std::function<void(const std::string&)> warn = [](const std::string&) {};

    // LOGGER.debug of Main.java:279-306, one message per topic ("Assignment for <topic>:\n<summary>"), in the
    // reference's format and order: consumers in consumerTotalLags' HashMap order, each followed by every
    // partition that consumer holds SO FAR (the reference prints the cumulative assignment map, :296).
    // Unset (the default) = isDebugEnabled() false: nothing is formatted.
    std::function<void(const std::string&)> debug;

 private:
    Assignment assignImpl(const Cluster& metadata, const GroupSubscription& subscriptions, OffsetSource& offsets,
                          const OrderedMap<std::vector<TopicPartition>>* owned);
    std::map<std::string, std::string> consumer_group_props_;
    std::map<std::string, std::string> metadata_consumer_props_;
    bool sticky_ties_ = false;                                           // lag.assignor.sticky.ties
    bool sticky_ties_large_ = false;                                     // lag.assignor.sticky.ties.large
    bool followup_pinned_ = false;                                       // lag.assignor.cooperative.followup = pinned
    bool followup_pinned_large_ = false;                                 // lag.assignor.cooperative.followup.large
    bool last_followup_ = false;                                         // the last assignCooperative asked for a follow-up ...
    std::map<std::string, std::vector<std::string>> last_subscription_;  // ... of this group: memberId -> its topic list
    std::map<std::string, std::map<std::string, int64_t>> last_totals_;
    bool last_order_exact_ = true;
};

// Exposed for tests of the host-side string logic (no GPU involved).
std::vector<int32_t> rankMembers(const std::vector<std::string>& memberIds);
std::vector<std::string> consumersPerTopicOrder(const GroupSubscription& subscriptions);
// The owned lists as la_assign_batch_cooperative takes them.  memberIds[i] owns ownedPerMember[i]; members are walked in
// String.compareTo rank order (member_off[r] = entries of the ranks below r); topic[j] is the index of the owned topic in
// `topics` (this rebalance's list), or -1 when it is not there: deleted, without metadata or subscriber -- a stale claim.
struct OwnedArrays {
    std::vector<int64_t> member_off;
    std::vector<int32_t> topic, partition;
};
OwnedArrays cooperativeOwnedArrays(const std::vector<std::string>& memberIds, const std::vector<std::string>& topics,
                                   const std::vector<std::vector<TopicPartition>>& ownedPerMember);

}  // namespace kafka_lag
