// fqd_near_umi_core.hpp — the rule of FQD_FAST_UMI_HAMMING=D: which exact clusters of a run keyed `B(U) ‖ mate 1, mate 2`
// (FQD_FAST_UMI) are copies of ONE molecule with sequencing errors in the read — one UMI, sequences within D substituted bases
// a mate — and how, with FQD_FAST_UMI_MISMATCH as well, the directional clusters of the UMIs hang into them.  It is
// fqd_near_core.hpp's rule with a tag in front; segments, pigeonhole and sweeps are that header's, unchanged.  Shared by the
// device code (csrc/fqd_near.hip) and a CPU harness of the tests (tests/native/near_umi_check.cpp builds this header with g++
// and the sanitizers); tests/near_umi_reference.py restates the tag and the tagged seed key in plain Python.
//
// ---- nodes, tags, near, links, molecules -----------------------------------------------------------------------------------
// node       one exact cluster of the run keyed B(U) ‖ mate 1, mate 2: fqd_owners of the first pass, owner[i] == i.
// tag        T(U) = the umi_len bytes of the node's first record's UMI field U (fqd_umi_core.hpp) with every joiner place
//            (fqd_umi_info.joiners) set to 0.  The run has ONE shape (umi_len, joiners) — fqd_umi_find refuses every other —
//            so T(U) = T(U') <=> U and U' hold the same byte at every place outside the joiner set <=> U ~ U' <=> B(U) = B(U'),
//            the last step by fqd_umi_core.hpp (a).  AC+GT and AC-GT are one tag; ACGT and ACGA are two.
// near       two nodes are near when their tags are EQUAL and fqdnear::near holds: equal shapes (len1[, len2]), mates 1 that
//            differ in at most D byte positions and, for pairs, mates 2 that differ in at most D positions.  'N' is a letter
//            like any other.  Nodes under different UMIs are never near, whatever their sequences.
// links      with FQD_FAST_UMI_MISMATCH=1|2 every node v is also linked to link[v], the first record of v's directional
//            cluster (fqd_umi_merge's owner_out at v): a node itself, link[v] <= v.  Without that switch there are no links.
// molecule   a connected component of near ∪ links, owned by — written as — its first record in input order.
//
// What follows from that:
//  * UMI distance and sequence distance never stand in ONE edge.  A copy with an error in its UMI AND one in its read joins its
//    family only through an intermediate node that has one of the two: the node (U', s) links to (U, s) and is near (U', s'), or
//    (U, s') is near (U, s) and is what (U', s') links to.  Where no copy with just one of the two errors was read, the copy
//    with both stays a molecule of its own.
//  * The directional rule counts stay those of the exact nodes: the links are made before, and independently of, the near edges.
//  * ALL MEMBERS OF A MOLECULE HAVE THE SAME LENGTHS (FQD_FAST_CONSENSUS's precondition): a near edge needs equal shapes, a link
//    joins two nodes of one sequence group, which is one sequence (pair) and so one shape; shape is constant along every edge,
//    hence on every component, and the members of a node are copies of its sequence.
//
// ---- seeds --------------------------------------------------------------------------------------------------------------------
// A node's key for segment j: h = seed_start(len1, len2, j); h = absorb(h, w) for the ceil(umi_len / 8) little-endian 64-bit
// words w of T(U), the last one zero-filled (umi_len is the run's, so the filling says nothing new); then the segment's bytes as
// in fqdnear::seed_key, and mix.  Equal (shape, tag, j, bytes) give equal keys, and two near nodes have equal tags and — by the
// pigeonhole of fqd_near_core.hpp — a segment on which they agree: near nodes share a key.
// The tag MUST be in the key: without it one sequence under 5000 UMIs would be one seed group of 5000 entries and be refused at
// FQD_NEAR_MAX_GROUP, where no two of its nodes can ever merge.  It decides nothing: the verification compares the tags byte for
// byte (tags_differ, word by word), because no hash decides a merge; FQD_NEAR_WEAK_SEEDS makes nodes of unlike tags meet.
//
// ---- eight lanes a pair ---------------------------------------------------------------------------------------------------------
// U is at most kMaxUmi = 64 = 8 * kLanes bytes: lane gl of a pair's group compares tag word gl of the two nodes (tag_word; 0
// behind the tag's end on both sides), the group sums what the lanes found, and a sum above 0 rejects the pair before a base
// is read.  No load leaves U: a whole word is one 8-byte load, U's tail goes byte by byte.
#pragma once
#include <cstdint>

#include "fqd_near_core.hpp"
#include "fqd_umi_core.hpp"

#if defined(__clang__)
#define FQD_NEAR_UMI_UNROLL _Pragma("unroll")               // (the tag's words stay in registers: no indexed array)
#else
#define FQD_NEAR_UMI_UNROLL
#endif

namespace fqdnearumi {

using fqdnear::kLanes;
using fqdumi::kMaxUmi;

constexpr uint32_t kTagWords = kMaxUmi / 8u;                   // words of a tag at most
static_assert(kMaxUmi == 8u * kLanes && kTagWords == kLanes, "lane gl of a pair's group compares tag word gl");

FQD_SEQ_HD uint32_t tag_words(uint32_t umi_len) { return (umi_len + 7u) / 8u; }

// 0xFF in byte k of the result where bit k of the low eight bits of `bits` is set.  (bits * 0x0101..01 puts a copy of the
// eight bits into every byte, the mask keeps bit k of byte k; + 0x7F carries a byte that is not 0 into its top bit, and no
// further, a byte being at most 0x80.)
FQD_SEQ_HD uint64_t bytes_of_bits(uint64_t bits)
{
    const uint64_t one = ((bits & 0xFFull) * 0x0101010101010101ull) & 0x8040201008040201ull;
    const uint64_t top = ((one + 0x7F7F7F7F7F7F7F7Full) | one) & 0x8080808080808080ull;
    return (top >> 7) * 0xFFull;
}

// Word w of T(U): the bytes U[8w .. min(8w + 8, umi_len)), little-endian, the joiner places and everything behind the tag's
// end 0.  No load leaves U[0 .. umi_len).
FQD_SEQ_HD uint64_t tag_word(const uint8_t* U, uint32_t umi_len, uint64_t joiners, uint32_t w)
{
    const uint32_t at = 8u * w;
    if (at >= umi_len) return 0ull;
    uint64_t x = 0;
    if (at + 8u <= umi_len) __builtin_memcpy(&x, U + at, 8);
    else for (uint32_t k = 0; at + k < umi_len; ++k) x |= uint64_t(U[at + k]) << (8u * k);
    return x & ~bytes_of_bits(joiners >> at);
}

// T(U) as words; those from tag_words(umi_len) on are 0.
struct Tag { uint64_t w[kTagWords]; };

FQD_SEQ_HD Tag load_tag(const uint8_t* U, uint32_t umi_len, uint64_t joiners)
{
    Tag t;
    FQD_NEAR_UMI_UNROLL
    for (uint32_t w = 0; w < kTagWords; ++w) t.w[w] = tag_word(U, umi_len, joiners, w);
    return t;
}

// Node's key for segment j of mate 1 under its tag (words = tag_words(umi_len)).
FQD_SEQ_HD uint64_t tagged_seed(const Tag& t, uint32_t words, const uint8_t* m1, uint32_t len1, uint32_t len2, uint32_t D, uint32_t j, bool weak)
{
    uint64_t h = fqdnear::seed_start(len1, len2, j);
    FQD_NEAR_UMI_UNROLL
    for (uint32_t w = 0; w < kTagWords; ++w)
        if (w < words) h = fqdnear::absorb(h, t.w[w]);
    const uint32_t from = fqdnear::bound(len1, D, j), to = fqdnear::bound(len1, D, j + 1u);
    const uint64_t key = fqdnear::seed_key(h, m1 + from, to - from);
    return weak ? key & fqdnear::kWeakMask : key;
}

// What a lane group makes of two tags: lane gl's word of each, and whether any lane's words differ.  (The harness plays the
// lanes one after another; the device sums across them.)
inline bool tags_differ(const uint8_t* Ua, const uint8_t* Ub, uint32_t umi_len, uint64_t joiners)
{
    uint32_t d = 0;
    for (uint32_t gl = 0; gl < kLanes; ++gl) d += tag_word(Ua, umi_len, joiners, gl) != tag_word(Ub, umi_len, joiners, gl);
    return d != 0;
}

inline bool near(const uint8_t* Ua, const uint8_t* Ub, uint32_t umi_len, uint64_t joiners, bool paired, fqdseq::View a1, fqdseq::View a2, fqdseq::View b1,
                 fqdseq::View b2, uint32_t D)
{
    return !tags_differ(Ua, Ub, umi_len, joiners) && fqdnear::near(paired, a1, a2, b1, b2, D);
}

// ---- links --------------------------------------------------------------------------------------------------------------------------
// A link is good where it names a node at or below its own: link <= v and owner[link] == link.
FQD_SEQ_HD bool link_is_good(const uint32_t* owner, uint32_t v, uint32_t link) { return link <= v && owner[link] == link; }

// The edge list of a molecule run: (link[v], v) for every node v with link[v] != v, in front of the m near edges; edges has
// room for 2 * (nodes + m) words.  Returns the edges.  components() of fqd_near_core.hpp takes the list as it is.
inline uint64_t with_links(const uint32_t* owner, const uint32_t* link, uint32_t n, const uint32_t* near_edges, uint64_t m, uint32_t* edges)
{
    uint64_t k = 0;
    if (link)
        for (uint32_t v = 0; v < n; ++v)
            if (owner[v] == v && link[v] != v) { edges[2 * k] = link[v]; edges[2 * k + 1] = v; ++k; }
    for (uint64_t q = 0; q < m; ++q, ++k) { edges[2 * k] = near_edges[2 * q]; edges[2 * k + 1] = near_edges[2 * q + 1]; }
    return k;
}

} // namespace fqdnearumi
