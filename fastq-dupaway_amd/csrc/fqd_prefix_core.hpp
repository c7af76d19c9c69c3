// fqd_prefix_core.hpp — the rule of FQD_FAST_PREFIX=L: which exact clusters of the `--fast` engine are TRUNCATED copies of
// another (a read that an adapter or quality trimmer cut short is a prefix of its untrimmed copy), how such pairs are found
// without comparing all pairs, and how the clusters hang together.  Shared by the device code (csrc/fqd_prefix.hip) and a CPU
// harness of the tests (tests/native/prefix_check.cpp builds this header with g++ and the sanitizers);
// tests/prefix_reference.py restates the rule and the seed hash in plain Python.
//
// ---- nodes, prefixes, parents ------------------------------------------------------------------------------------------------
// node       one exact cluster of the engine, named by its first record (owner[i] == i): one sequence m1(v), or one pair of
//            them m1(v), m2(v).  span(v) = len1 + len2 (len2 = 0 for a single-end node).
// a ⊑ b      "a is a prefix of b": a and b are different nodes, len1(a) <= len1(b) and the bytes of m1(a) are the first len1(a)
//            bytes of m1(b); for pairs the same holds for mate 2 (the reference's `loose` rule with its same-sided condition:
//            a pair whose mate 1 is the shorter and whose mate 2 is the longer is NOT related).  Every byte is a letter: 'N'
//            equals 'N' only.  Nodes are distinct keys — they differ in a length or in a byte — so a ⊑ b leaves a length
//            that is strictly below: span(a) < span(b), and two nodes of one shape are never related.
// eligible   len1 >= L and, for pairs, len2 >= L (L = the switch's value, the minimum overlap).  Only eligible nodes take
//            part: a ⊑ b is asked of two eligible nodes only.  A node that is not eligible stays a cluster of its own.  It
//            cannot be a CHILD, because its overlap with anything is below L bases — a 5-base remnant is a prefix of a
//            thousandth of all reads, which says nothing about molecules.  It cannot be a PARENT either: a ⊑ b needs
//            len(a) <= len(b) mate by mate, so an eligible a (every mate >= L) under a b with a mate below L does not exist.
// parent(a)  among all b with a ⊑ b the one with the least span, and among those the lowest record number: the least
//            pack(b) = span(b) << 32 | b, a total order on nodes.  A node without such a b is a ROOT.
// merged     one tree of the parent relation, owned by — written as — its first record in input order.
// This is NOT single linkage over ⊑: a 32-base read A is a prefix of two different 150-base reads B and C; A goes to one of
// them (the lower record) and B and C stay two clusters.
//
// ---- what holds --------------------------------------------------------------------------------------------------------------
// (a) FOREST.  span(parent(a)) > span(a), so a chain a, parent(a), parent(parent(a)), .. strictly grows in span, never comes
//     back, and ends after at most (largest span - L) links in a node without a parent: every node has exactly one root.
// (b) TRANSITIVE.  a ⊑ b and b ⊑ c give a ⊑ c: the lengths chain mate by mate, and the first len(a) bytes of b are among the
//     first len(b) bytes of b, which are c's.  a != c since span(a) < span(c); c is eligible.  So by induction along the chain
//     EVERY MEMBER OF A TREE IS ⊑ ITS ROOT (or is the root): a merged cluster is a set of prefixes of ONE maximal sequence.
// (c) TWO ROOTS ARE NEVER IN ONE CLUSTER: a cluster is a tree, and a tree has one root by (a).  In particular two maximal
//     sequences (B and C above) are never merged, whatever they share.
// (d) SCHEDULING.  best[a] = min over the related pairs (a, b) that verification finds of pack(b), by a 64-bit atomicMin
//     into a word that starts as all ones: min is commutative and associative, so best[a] is the formula whatever the order of
//     the pairs and however often one is found.  Verification finds EVERY pair a ⊑ b (see seeds), so best[a] = pack(parent(a)).
//
// ---- seeds -------------------------------------------------------------------------------------------------------------------
// An eligible node has ONE entry (key, node): key = a 64-bit hash of (paired?, L, the first L bytes of mate 1, the first L bytes
// of mate 2).  a ⊑ b with both eligible means that the first len(a) >= L bytes agree mate by mate, so the first L do: RELATED
// NODES SHARE A KEY, and a seed group — the entries of one key — holds every b with a ⊑ b for each of its a.  Unequal inputs
// may collide; that costs compares and never a result, because every candidate pair's lengths are compared as numbers and its
// whole overlap byte for byte.  No hash decides a merge.  (FQD_PREFIX_WEAK_SEEDS cuts the keys to 4 bits to make that happen.)
// A group of more than FQD_PREFIX_MAX_GROUP entries is refused (adapter dimers, amplicons, an L that is too small).
//
// ---- trees: the parallel form ------------------------------------------------------------------------------------------------
// up[v] starts as parent(v) (v itself for a root, an ineligible node, a record that is no node).  One jump, every v at once,
// reads one array and writes another: up'[v] = up[up[v]].  After k jumps up[v] is the node min(2^k, depth(v)) links above v
// (induction: both halves of the doubled path are k-jump pointers, and a root points at itself); a jump changes something
// exactly while some depth(v) > 2^k.  So the jumps that change something number ceil(log2(deepest)) (0 for deepest <= 1), the
// fixed point is root(v), and neither depends on scheduling.  `deepest` itself — the longest parent chain, in links — is
// COUNTED in the first pass: every child walks its chain once (chain_depth), which (a) bounds.
#pragma once
#include <cstdint>

#include "fqd_near_core.hpp"

#define FQD_PREFIX_MAX_GROUP 4096u

namespace fqdprefix {

constexpr uint32_t kMaxGroup = FQD_PREFIX_MAX_GROUP;          // entries of a seed group at most
constexpr uint32_t kMinOverlap = 1, kMaxOverlap = 65535;      // L
constexpr uint32_t kLanes = fqdnear::kLanes;                  // lanes a candidate pair (verify)
constexpr uint32_t kChunk = fqdnear::kChunk;                  // bytes a lane and load
constexpr uint64_t kWeakMask = 15;                            // FQD_PREFIX_WEAK_SEEDS: what is left of a key
constexpr uint64_t kNoParent = ~0ull;                         // best[v] of a node without a parent
constexpr uint64_t kPrefixTag = 0x7072656669780000ull;        // ("prefix": these keys are no FQD_FAST_HAMMING keys)

// ---- eligibility, direction --------------------------------------------------------------------------------------------------

FQD_SEQ_HD bool eligible(bool paired, uint32_t len1, uint32_t len2, uint32_t L) { return len1 >= L && (!paired || len2 >= L); }

// Which of two nodes of one group can be the prefix of the other, by the lengths alone: 1 = a (both mates <=), 2 = b (both
// >=), 0 = neither (opposite sides, or one shape: nodes of one shape are distinct keys and never related).
FQD_SEQ_HD int direction(bool paired, uint32_t a1, uint32_t a2, uint32_t b1, uint32_t b2)
{
    if (!paired) return a1 < b1 ? 1 : a1 > b1 ? 2 : 0;
    if (a1 == b1 && a2 == b2) return 0;
    if (a1 <= b1 && a2 <= b2) return 1;
    if (a1 >= b1 && a2 >= b2) return 2;
    return 0;
}

// ---- the seed key ------------------------------------------------------------------------------------------------------------
// fqdnear's hash (mix, absorb, seed_key: sixteen bytes a load while sixteen are left, then eight, then byte by byte, so no load
// leaves the L bytes): h0 = mix(mix(L | paired << 32) ^ kPrefixTag), mate 1's first L bytes absorbed into h0, and for pairs
// mate 2's first L bytes absorbed into that result.

FQD_SEQ_HD uint64_t seed_start(bool paired, uint32_t L)
{
    return fqdnear::mix(fqdnear::mix(uint64_t(L) | (uint64_t(paired) << 32)) ^ kPrefixTag);
}

// m1, m2: the node's mates, of at least L bytes each (m2 is not looked at for a single-end node).
FQD_SEQ_HD uint64_t node_seed(bool paired, const uint8_t* m1, const uint8_t* m2, uint32_t L, bool weak)
{
    uint64_t key = fqdnear::seed_key(seed_start(paired, L), m1, L);
    if (paired) key = fqdnear::seed_key(key, m2, L);
    return weak ? key & kWeakMask : key;
}

// ---- the overlap compare, kChunk bytes a lane ----------------------------------------------------------------------------------

// Do a and b differ in chunk c of n bytes, [c * kChunk, min(n, (c + 1) * kChunk))?  No behind the end.  A whole chunk is one
// 16-byte load a side, the last, partial one goes byte by byte (fqdnear::chunk_mismatches): no load leaves [0, n).
FQD_SEQ_HD bool chunk_differs(const uint8_t* a, const uint8_t* b, uint32_t n, uint32_t c) { return fqdnear::chunk_mismatches(a, b, n, c) != 0u; }

// What a lane group makes of an overlap of n bytes: rounds of kLanes chunks, and no further round behind the first with a
// difference.  (The harness plays the lanes one after another; the device ors across them.)  rounds: how many were played.
inline bool lanes_equal(const uint8_t* a, const uint8_t* b, uint32_t n, uint32_t* rounds = nullptr)
{
    bool differs = false;
    uint32_t played = 0;
    for (uint32_t c0 = 0; uint64_t(c0) * kChunk < n && !differs; c0 += kLanes, ++played)
        for (uint32_t gl = 0; gl < kLanes; ++gl) differs |= chunk_differs(a, b, n, c0 + gl);
    if (rounds) *rounds = played;
    return !differs;
}

// ---- a ⊑ b as verification decides it, for two eligible nodes of one group ------------------------------------------------------
// Returns direction's answer where the short node is a prefix of the long one, 0 otherwise.
inline int related(bool paired, fqdseq::View a1, fqdseq::View a2, fqdseq::View b1, fqdseq::View b2)
{
    const int dir = direction(paired, a1.len, paired ? a2.len : 0u, b1.len, paired ? b2.len : 0u);
    if (dir == 0) return 0;
    const fqdseq::View s1 = dir == 1 ? a1 : b1, s2 = dir == 1 ? a2 : b2;
    if (!lanes_equal(a1.p, b1.p, s1.len)) return 0;
    if (paired && !lanes_equal(a2.p, b2.p, s2.len)) return 0;
    return dir;
}

// ---- best ----------------------------------------------------------------------------------------------------------------------

FQD_SEQ_HD uint64_t pack(uint32_t span, uint32_t node) { return (uint64_t(span) << 32) | node; }
FQD_SEQ_HD bool has_parent(uint64_t best) { return best != kNoParent; }
FQD_SEQ_HD uint32_t parent_of(uint64_t best, uint32_t self) { return has_parent(best) ? uint32_t(best) : self; }

// The links of v's parent chain.  Bounded by (a): every link grows the span.
FQD_SEQ_HD uint32_t chain_depth(const uint64_t* best, uint32_t v)
{
    uint32_t depth = 0;
    for (uint64_t b = best[v]; has_parent(b); b = best[uint32_t(b)]) ++depth;
    return depth;
}

// ---- trees: the rule as the device runs it, one step after the other -----------------------------------------------------------
// best: n words; up, other: n entries of room each.  The roots end in *roots (up or other); returns the jumps that changed
// something, and the longest chain in *deepest.
inline uint32_t trees(const uint64_t* best, uint32_t n, uint32_t* up, uint32_t* other, const uint32_t** roots, uint32_t* deepest)
{
    *deepest = 0;
    for (uint32_t v = 0; v < n; ++v) {
        up[v] = parent_of(best[v], v);
        const uint32_t d = chain_depth(best, v);
        if (d > *deepest) *deepest = d;
    }
    uint32_t jumps = 0;
    for (;;) {
        bool changed = false;
        for (uint32_t v = 0; v < n; ++v) { other[v] = up[up[v]]; changed |= other[v] != up[v]; }
        if (!changed) break;
        uint32_t* t = up; up = other; other = t;
        ++jumps;
    }
    *roots = up;
    return jumps;
}

} // namespace fqdprefix
