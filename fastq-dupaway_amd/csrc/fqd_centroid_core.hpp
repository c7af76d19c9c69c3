// fqd_centroid_core.hpp — FQD_FAST_CENTROID=abundant of the `--fast` mode: which member of a merged cluster is written.  The
// rule, its proofs, and what the tiers of fqd_centroid.hip share (the size classes, the slot choice of the two tables, the
// packed key of the table in scratch, the saturation and the masked scores).  Plain C++ that compiles on the host
// (tests/native/centroid_check.cpp) and in the device code.
//
// THE RULE.  A final cluster C is a run of (perm, head) as fqd_group_owners leaves it — the state after every merge and
// after the optical split — with its members in input order.  For a member i
//     label[i]   the first record of the whole input with i's exact key (its exact owner),
//     weight[i]  1, or what the record stands for (FQD_FAST_SIZEIN=1),
//     S(i)       { j in C : label[j] = label[i] }, i's SUB-CLUSTER.  It is cut to C: FQD_FAST_OPTICAL deals one exact
//                cluster to several groups, so one label can stand in several runs, and a count per label alone would add
//                the members of other runs,
//     a(i)       the sum of weight[j] over S(i), i's ABUNDANCE, summed in 64 bits.
// The CENTROID of C is the member with the largest a(i), among equals the earliest in input order (better()).
//
// SATURATION.  a(i) is stored in 32 bits as min(a(i), 2^32 - 1) (saturate()).  With weights of 1 a(i) <= n < 2^31 and never
// saturates.  With FQD_FAST_SIZEIN the whole cluster's weight is at least a(i), and fqd_cluster_weights ends the run for a
// cluster above 2^31 - 1 before any output exists: a saturated value — two sub-clusters above 2^32 - 2 would compare equal —
// never decides an output.
//
// PROOFS.
// (1) The centroid is the first member of its sub-cluster.  All members of S(i) have the same a; of equal values the
//     earliest wins; the first member of S(i) stands in front of the others.
// (2) Among sub-clusters of equal abundance the one whose first member stands earliest wins: by (1) the candidates are the
//     first members of the sub-clusters of the largest abundance, and the earliest of those is taken.
// (3) The centroid is the cluster's first member exactly when that member's sub-cluster is among the maxima: if it is, no
//     member is earlier and none has a larger a; if it is not, a member with a larger a exists and better() prefers it.  A
//     cluster of a single sub-cluster has all a equal, so its first member stays: it is never touched.
// (4) The result does not depend on scheduling.  a(i) is a sum of integers in 64 bits — at most 2^31 - 1 members of at most
//     2^32 - 1 each, below 2^63, so no sum wraps — and integer addition commutes: whichever lane, wave or workgroup adds
//     a weight first, and whichever slot of a table a label comes to lie in, the sums are the same.  saturate() is applied
//     once to the finished sum.  The pick over the stored values is fqd_seq_pick_best's, which fqd_seq_pick_core.hpp proves
//     independent of its cut into lanes and tiles.
// (5) FQD_FAST_KEEP=best inside the winning sub-cluster.  fqd_seq_pick_best exchanges perm[head place] and perm[the
//     centroid's place] and touches nothing else.  The centroid is the FIRST member of S (1), so behind the exchange it stands at
//     the head place and the other members of S stand where they stood, in input order, all behind the head place; the
//     former first member now stands at the centroid's old place but is no member of S (where it is, nothing was exchanged).
//     masked_score() is score + 1 (so that it is above 0) for the members of S and 0 for every other member, so a second
//     "highest, earliest among equals" pick over it takes a member of S — S is not empty — namely the one with the highest
//     score, and among equals the earliest in the order, which inside S is input order.  min(score, 2^32 - 2) + 1 is
//     monotone; scores 2^32 - 1 and 2^32 - 2 fall together, as they only can where fqd_seq_scores has saturated.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FQD_CENTROID_HD __host__ __device__ __forceinline__
#else
#define FQD_CENTROID_HD inline
#endif

namespace fqdcentroid {

// ---- the size classes (fqd_centroid_info.tier_clusters) -------------------------------------------------------------------
constexpr uint32_t kSmall = 8;                               // eight lanes a cluster
constexpr uint32_t kWave = 64;                               // a wave a cluster
// A workgroup's cluster: its labels in an open-addressing table in LDS of kBlockSlots = 2 * kBlockLimit slots (load factor
// at most 1/2), 4 bytes a key and 8 bytes a sum.  48 KiB a workgroup: three workgroups share a CU's 160 KiB of LDS, and at
// 512 threads each that is 24 of the CU's 32 waves.
constexpr uint32_t kBlockLimit = 2048;
constexpr uint32_t kBlockSlots = 2 * kBlockLimit;
constexpr uint32_t kBlockTableBytes = kBlockSlots * (sizeof(uint32_t) + sizeof(uint64_t));
constexpr uint32_t kLdsPerCu = 160 * 1024;
static_assert(kBlockTableBytes == 48 * 1024 && 3 * kBlockTableBytes <= kLdsPerCu, "three workgroups' tables fit a CU's LDS");
static_assert((kBlockSlots & (kBlockSlots - 1)) == 0 && kBlockLimit > kWave && kWave > kSmall, "the slot mask; the tiers follow each other");

enum Tier : uint32_t { kTierOne = 0, kTierSmall = 1, kTierWave = 2, kTierBlock = 3, kTierLarge = 4 };

FQD_CENTROID_HD uint32_t tier_of(uint32_t members)
{
    return members <= 1u ? kTierOne : members <= kSmall ? kTierSmall : members <= kWave ? kTierWave : members <= kBlockLimit ? kTierBlock : kTierLarge;
}

// ---- the values -----------------------------------------------------------------------------------------------------------
constexpr uint32_t kSaturated = 0xFFFFFFFFu;

FQD_CENTROID_HD uint32_t saturate(uint64_t sum) { return sum > kSaturated ? kSaturated : uint32_t(sum); }

// Is the member at place p with abundance a the better centroid than the one at place q with abundance b?
FQD_CENTROID_HD bool better(uint32_t a, uint64_t p, uint32_t b, uint64_t q) { return a > b || (a == b && p < q); }

// What the second pick reads: see (5).
FQD_CENTROID_HD uint32_t masked_score(uint32_t score, bool in_winning_subcluster)
{
    return in_winning_subcluster ? (score > 0xFFFFFFFEu ? 0xFFFFFFFEu : score) + 1u : 0u;
}

// ---- the table in LDS: keyed by the label alone (one cluster a table) -------------------------------------------------------
// A label is a record below n < 2^31: all ones is no label.
constexpr uint32_t kNoLabel = 0xFFFFFFFFu;

// The slots a cluster of `members` uses: the power of two that is at least twice the members (64 .. kBlockSlots), so that a
// cluster of a hundred clears and probes a table of 256, not of 4096.
FQD_CENTROID_HD uint32_t block_slots(uint32_t members)
{
    uint32_t slots = 64;
    while (slots < 2u * members && slots < kBlockSlots) slots <<= 1;
    return slots;
}

// Where the probe for `label` starts in a table of `slots` (a power of two): the high bits of a Fibonacci product, so that
// neighbouring records — the usual labels of one cluster — do not share their low bits' slot runs.
FQD_CENTROID_HD uint32_t block_slot(uint32_t label, uint32_t slots) { return ((label * 0x9E3779B1u) >> 7) & (slots - 1u); }

// ---- the table in scratch: keyed by (head place << 32 | label), so that equal labels of different runs never meet -----------
// A head place is below n <= 2^31 - 1, so its bit 31 is clear and all ones is no key.
constexpr uint64_t kNoKey = ~0ull;

FQD_CENTROID_HD uint64_t pack_key(uint32_t head_place, uint32_t label) { return (uint64_t(head_place) << 32) | label; }

// Twice as many slots as the tier has members (below 2^32, for fewer than 2^31 members).
FQD_CENTROID_HD uint64_t scratch_slots(uint64_t members) { return 2u * members; }

// Where the probe for `key` starts among `slots` (any number in 1 .. 2^32 - 2): the key mixed to 32 bits (the finalizer of
// MurmurHash3, public domain), then the high word of mixed * slots, which is below slots.
FQD_CENTROID_HD uint64_t scratch_slot(uint64_t key, uint64_t slots)
{
    key ^= key >> 33; key *= 0xFF51AFD7ED558CCDull; key ^= key >> 33; key *= 0xC4CEB9FE1A85EC53ull; key ^= key >> 33;
    return ((key >> 32) * slots) >> 32;
}

// The slot behind `slot` (both tables probe linearly and wrap).
FQD_CENTROID_HD uint64_t next_slot(uint64_t slot, uint64_t slots) { return slot + 1 == slots ? 0 : slot + 1; }

} // namespace fqdcentroid
