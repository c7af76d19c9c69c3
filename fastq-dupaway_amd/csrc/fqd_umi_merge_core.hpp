// fqd_umi_merge_core.hpp — the rule of FQD_FAST_UMI_MISMATCH=1|2: which exact UMI clusters of `--fast` with FQD_FAST_UMI
// are one molecule although their UMIs differ in a base or two (UMI-tools' `directional` method).  Shared by the device
// code (csrc/fqd_umi_merge.hip) and a CPU harness of the tests (tests/native/umi_merge_check.cpp builds this header with
// g++ and the sanitizers).
//
// ---- definitions -----------------------------------------------------------------------------------------------------
// D         the switch's value, 1 or 2.
// group     the records (pairs) whose sequences are identical without the UMI: mate 1 with its length, mate 2 for pairs,
//           the canonical forms with FQD_FAST_STRAND=both.  UMIs under different sequences never meet.
// node      one distinct B(U) (fqd_umi_core.hpp) inside a group — an exact cluster of the run keyed B(U) ‖ seq.
//           count = its members, first = its first record in input order.  Inside a group the nodes stand in the order of
//           their first records; pos = a node's place in that order, so first ascends with pos.
// dist      the number of places at which two nodes' B(U) differ (all have the run's Lb bases; N is a letter like any other).
// edge      a -> b  <=>  dist(a, b) <= D and count(a) >= 2 count(b) - 1.  Two nodes of count 1 link both ways.
// rank      count descending, then first ascending: a total order, no two nodes share a first record.
// root(v)   the best-ranked node among v and every node with a directed path to v.
// cluster   all records of all nodes with one root; it is written as (owned by) its first record in input order.
//
// ---- the sequential method finds the same clusters ---------------------------------------------------------------------
// UMI-tools visits the nodes in rank order; an unclaimed node starts a component of everything it reaches through nodes
// not claimed before, and a reached node belongs to the first component that reached it.  Claim: v ends in the component
// of root(v).  Let u = root(v), the best-ranked node that reaches v (v reaches itself by the empty path).
// (a) No earlier component claims u: its starter s would reach u and so v, with a better rank than u.  So when the visit
//     comes to u it is unclaimed and starts a component.
// (b) No node w on a path u -> ... -> v was claimed before by a starter s: s reaches w and from there v, with a better
//     rank than u.  So u's search gets through to v, and no starter before u reaches v at all.
// Hence v is claimed by u.  The same argument shows that a SHORTEST path from u to v lies inside u's component.
//
// ---- the parallel form -------------------------------------------------------------------------------------------------------
// label(v) = (~count(v) << 32) | pos(v), a 64-bit word that is smaller for the better rank.  One sweep sets every
// label[v] to the minimum of its old value and the OLD labels of the nodes u with u -> v (all nodes at once: a node reads
// what the sweep before left).  After t sweeps label[v] is the best label among the nodes with a path of at most t edges
// to v; that sequence falls, is bounded, and stands still exactly when label[v] = label(root(v)) for every v: the fixed
// point is unique, whatever order the work is done in.  The sweeps that change something number max over v of the length
// of the shortest path from root(v) to v — at most nodes - 1, which bounds every loop below.
// The cluster's first record is the minimum `first`, that is the minimum pos, over the nodes of a root (the root itself
// has the highest count, not always the lowest first record).
//
// ---- the packed UMI --------------------------------------------------------------------------------------------------------
// A base is four bits (A 0, C 1, G 2, T 3, N 4), sixteen bases a 64-bit word, base j in bits 4 (j % 16) .. of word j / 16;
// the bits behind the last base are 0.  Two words differ in a base exactly where the xor has a set bit in that base's
// nibble: fold the nibble's bits onto its lowest and count.
#pragma once
#include <cstdint>

#include "fqd_umi_core.hpp"

#define FQD_UMI_MERGE_MAX_GROUP 4096u

namespace fqdmerge {

constexpr uint32_t kMaxGroup = FQD_UMI_MERGE_MAX_GROUP;        // nodes of a group at most
constexpr uint32_t kSmall = 8;                                // up to here: eight lanes a group, eight groups a wave
constexpr uint32_t kWave = 64;                                // up to here: a wave a group; beyond: a block
constexpr uint32_t kMaxWords = 4;                             // 64 bases at most (fqdumi::kMaxUmi)
constexpr uint32_t kNoPos = 0xFFFFFFFFu;

FQD_UMI_HD uint32_t code(uint8_t b) { return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : b == 'N' ? 4u : 5u; }

FQD_UMI_HD uint32_t words(uint32_t lb) { return (lb + 15u) / 16u; }

// Word w of B(U): the bases 16 w .. of U's Lb, through the shape's table.  Every load lies in U.
FQD_UMI_HD uint64_t pack_word(const uint8_t* U, const fqdumi::Table& t, uint32_t lb, uint32_t w)
{
    uint64_t x = 0;
    for (uint32_t j = 16u * w; j < lb && j < 16u * w + 16u; ++j) x |= uint64_t(code(U[t.at[j]])) << (4u * (j & 15u));
    return x;
}

FQD_UMI_HD uint32_t word_dist(uint64_t a, uint64_t b)
{
    uint64_t x = a ^ b;
    x |= x >> 2;
    x |= x >> 1;
    return uint32_t(__builtin_popcountll(x & 0x1111111111111111ull));
}

// dist(a, b) <= D, a and b packed in W words each.
FQD_UMI_HD bool near(const uint64_t* a, const uint64_t* b, uint32_t W, uint32_t D)
{
    uint32_t d = 0;
    for (uint32_t w = 0; w < W; ++w) d += word_dist(a[w], b[w]);
    return d <= D;
}

FQD_UMI_HD bool counts_allow(uint32_t count_a, uint32_t count_b) { return uint64_t(count_a) + 1u >= 2u * uint64_t(count_b); }

FQD_UMI_HD uint64_t label_of(uint32_t count, uint32_t pos) { return (uint64_t(~count) << 32) | pos; }
FQD_UMI_HD uint32_t label_pos(uint64_t label) { return uint32_t(label); }

// ---- a lane a node: groups of up to 64 nodes (P = the group's packed UMIs, W words a node; C = its counts) ---------------

// Bit u of the result: u -> v.
FQD_UMI_HD uint64_t lane_in_edges(const uint64_t* P, const uint32_t* C, uint32_t s, uint32_t W, uint32_t D, uint32_t v)
{
    uint64_t m = 0;
    for (uint32_t u = 0; u < s; ++u)
        if (u != v && counts_allow(C[u], C[v]) && near(P + size_t(u) * W, P + size_t(v) * W, W, D)) m |= 1ull << u;
    return m;
}

// One sweep of lane v: old_of(u) = the label lane u held when the sweep began, asked of every u < s_all by every lane (on
// the device a cross-lane read that the whole group takes part in; s_all is the same for all of them).
template <class OldOf>
FQD_UMI_HD uint64_t lane_sweep(uint64_t in_edges, uint64_t own, uint32_t s_all, OldOf old_of)
{
    uint64_t best = own;
    for (uint32_t u = 0; u < s_all; ++u) {
        const uint64_t lu = old_of(u);
        if (((in_edges >> u) & 1u) && lu < best) best = lu;
    }
    return best;
}

// The lowest pos among the lanes that ended with lane v's label: label_of_lane(u) as above.
template <class LabelOf>
FQD_UMI_HD uint32_t lane_first_of_root(uint64_t own, uint32_t s_all, LabelOf label_of_lane)
{
    uint32_t lowest = kNoPos;
    for (uint32_t u = 0; u < s_all; ++u) {
        const uint64_t lu = label_of_lane(u);
        if (lu == own && lowest == kNoPos) lowest = u;
    }
    return lowest;
}

// ---- a block a group: up to kMaxGroup nodes, the labels in one array that every thread reads between two barriers -----------

// Node v's label after one sweep over `labels` (what the sweep before left).  A node u is looked at closely only where its
// label would lower v's and the counts allow the edge; most pairs end at the first of the two compares.
FQD_UMI_HD uint64_t block_sweep(const uint64_t* P, const uint32_t* C, const uint64_t* labels, uint32_t s, uint32_t W, uint32_t D, uint32_t v)
{
    uint64_t best = labels[v];
    const uint32_t cv = C[v];
    for (uint32_t u = 0; u < s; ++u) {
        const uint64_t lu = labels[u];
        if (lu < best && counts_allow(C[u], cv) && near(P + size_t(u) * W, P + size_t(v) * W, W, D)) best = lu;
    }
    return best;
}

// ---- the rule group by group (what the lanes must agree with; the host's way to state it) -----------------------------------

// root_pos[v] = pos(root(v)), first_pos[v] = the lowest pos of root(v)'s cluster; returns the sweeps that changed a label.
inline uint32_t merge_group(const uint64_t* P, const uint32_t* C, uint32_t s, uint32_t W, uint32_t D, uint32_t* root_pos, uint32_t* first_pos,
                            uint64_t* labels, uint64_t* next)
{
    for (uint32_t v = 0; v < s; ++v) labels[v] = label_of(C[v], v);
    uint32_t sweeps = 0;
    for (uint32_t t = 0; t < s; ++t) {
        bool changed = false;
        for (uint32_t v = 0; v < s; ++v) {
            uint64_t best = labels[v];
            for (uint32_t u = 0; u < s; ++u)
                if (u != v && counts_allow(C[u], C[v]) && near(P + size_t(u) * W, P + size_t(v) * W, W, D) && labels[u] < best) best = labels[u];
            next[v] = best;
            changed |= best != labels[v];
        }
        if (!changed) break;
        for (uint32_t v = 0; v < s; ++v) labels[v] = next[v];
        ++sweeps;
    }
    for (uint32_t v = 0; v < s; ++v) { root_pos[v] = label_pos(labels[v]); first_pos[v] = kNoPos; }
    for (uint32_t v = 0; v < s; ++v) if (first_pos[root_pos[v]] == kNoPos) first_pos[root_pos[v]] = v;     // (v ascends: the lowest)
    for (uint32_t v = 0; v < s; ++v) if (root_pos[v] != v) first_pos[v] = first_pos[root_pos[v]];
    return sweeps;
}

} // namespace fqdmerge
