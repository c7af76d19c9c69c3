// fqd_near_core.hpp — the rule of FQD_FAST_HAMMING=D: which exact clusters of the `--fast` engine are copies of one another
// with sequencing errors in them (at most D substituted bases a mate), how such pairs are found without comparing all pairs,
// and how the clusters hang together.  Shared by the device code (csrc/fqd_near.hip) and a CPU harness of the tests
// (tests/native/near_check.cpp builds this header with g++ and the sanitizers); tests/near_reference.py restates the segment
// bounds and the seed hash in plain Python.
//
// ---- nodes, near, merged clusters ------------------------------------------------------------------------------------------
// node       one exact cluster of the engine, named by its first record (owner[i] == i): one sequence, or one pair of them.
// shape      (len1) of a single-end node, (len1, len2) of a pair.
// near       two nodes of EQUAL shape whose mates 1 differ in at most D byte positions and, for pairs, whose mates 2 differ in
//            at most D positions as well: D holds for each mate on its own (hamming_match of fqd_seq_core.hpp, mate by mate).
//            Every byte is a letter: 'N' agrees with 'N' and differs from 'A'.  Nodes of different shape are never near.
// merged     a connected component of `near` (single linkage: A-B-C is one cluster even where A and C differ in 2D places),
//            owned by — written as — its first record in input order.  D is 1, 2 or 3.
//
// ---- seeds ---------------------------------------------------------------------------------------------------------------
// Mate 1 of length len is cut at b_j = floor(j * len / (D + 1)), j = 0 .. D + 1, into the D + 1 segments [b_j, b_j+1).
// b_0 = 0, b_(D+1) = len and b_j <= b_j+1, so the segments are disjoint and cover [0, len); for len < D + 1 some are empty.
// PIGEONHOLE.  Two near nodes have one len (equal shape), so one set of bounds, and their mates 1 differ in at most D
// positions.  Every differing position lies in exactly one segment; D + 1 segments and at most D positions leave a segment
// without one: on that segment the two nodes agree byte for byte.  An empty segment holds no position at all, so it is
// "agreed on" by every two nodes of the shape: the argument does not care, it only needs one segment that is free of
// differences, and for len < D + 1 an empty one always is.
// A node's seed key for segment j is seed_key below: a 64-bit hash of (len1, len2, j, the segment's bytes); len2 is 0 for a
// single-end node.  Equal (shape, j, bytes) give equal keys, so two near nodes share a key; a seed group is the set of
// entries (key, node) with one key.  Unequal inputs may collide: that puts nodes into one group that agree on nothing, which
// costs compares and never a result, because EVERY candidate pair is compared byte for byte over both mates and the shapes
// are compared as numbers.  No hash decides a merge.  (FQD_NEAR_WEAK_SEEDS cuts the keys to 4 bits to make that happen.)
// A group of more than FQD_NEAR_MAX_GROUP entries is refused (adapter dimers, amplicons).  A group is counted in entries:
// a node stands in one group twice only where two of its own keys collide.
//
// ---- components: the parallel form ---------------------------------------------------------------------------------------
// An edge is a pair of near nodes that verification found; neighbour = the other end of an edge.  label(v) starts as v, the
// node's record number.  One sweep is two steps, every node at once, each step reading only what the step before left:
//   min    L'[v] = min(L[v], min over the neighbours u of v of L[u])
//   jump   L[v]  = L'[L'[v]]                                         (pointer jumping)
// and the sweeps end with the first min step that changes nothing (that step is not counted).
// (a) L[v] <= v, and L[v] is a node of v's component, always: true at the start; a min step takes v's own label or a lower
//     one of a neighbour, which names a node of the neighbour's component, that is of v's; a jump takes the label of a node
//     w = L'[v] of v's component, and L'[w] <= w = L'[v].  So no step raises a label.
// (b) After t sweeps L[v] <= min{u : u within t edges of v}: the min step gives the min over the neighbours' bounds, that is
//     the bound for t + 1, and the jump only lowers.  With (a), L[v] >= the lowest node m of v's component; so after at most
//     ecc <= s - 1 sweeps (s = the component's nodes) every label IS m, and the next min step changes nothing.  Every loop is
//     bounded by the number of nodes.
// (c) Where a min step changes nothing, every node's label is <= its neighbours' and, edges being symmetric, equal to them:
//     constant c on a component.  By (a) c <= m and c names a node of it: c = m.  The fixed point is unique.
// (d) Every step reads one array and writes another.  The min step over an edge LIST is, for every edge (a, b), an integer
//     atomicMin of the lower of L[a], L[b] into L' of the other end, L' having started as a copy of L: min is commutative and
//     associative, so L' is the formula above whatever order the edges are taken in and however often one edge stands in the
//     list.  The labels after every sweep, and with them the NUMBER of sweeps, depend neither on scheduling nor on the order
//     or multiplicity of the edges.
#pragma once
#include <cstdint>

#include "fqd_seq_core.hpp"

#define FQD_NEAR_MAX_GROUP 4096u

namespace fqdnear {

constexpr uint32_t kMaxGroup = FQD_NEAR_MAX_GROUP;            // entries of a seed group at most
constexpr uint32_t kMaxDistance = 3;
constexpr uint32_t kLanes = 8;                                // lanes a candidate pair (verify)
constexpr uint32_t kChunk = 16;                               // bytes a lane and load
constexpr uint64_t kWeakMask = 15;                            // FQD_NEAR_WEAK_SEEDS: what is left of a key
constexpr uint64_t kMul = 0x9E3779B97F4A7C15ull;

// ---- segments ------------------------------------------------------------------------------------------------------------

FQD_SEQ_HD uint32_t bound(uint32_t len, uint32_t D, uint32_t j) { return uint32_t(uint64_t(j) * len / (D + 1u)); }

// ---- the seed hash ---------------------------------------------------------------------------------------------------------
// h0 = mix(mix(len1 | len2 << 32) ^ (j + 1) * kMul); every 8 bytes of the segment, little-endian, the last word filled up with
// zero bytes (the segment's length follows from len1 and j, so the filling says nothing new), go in as h = absorb(h, w); the
// key is mix(h).

FQD_SEQ_HD uint64_t mix(uint64_t h)
{
    h ^= h >> 32; h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32; h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    return h;
}

FQD_SEQ_HD uint64_t absorb(uint64_t h, uint64_t w)
{
    h = (h ^ w) * kMul;
    return h ^ (h >> 29);
}

FQD_SEQ_HD uint64_t seed_start(uint32_t len1, uint32_t len2, uint32_t j)
{
    return mix(mix(uint64_t(len1) | (uint64_t(len2) << 32)) ^ (uint64_t(j + 1u) * kMul));
}

// The key of the n bytes at p.  Sixteen bytes a load while sixteen are left, then eight, then byte by byte: no load leaves
// [p, p + n), whatever p's alignment.
FQD_SEQ_HD uint64_t seed_key(uint64_t start, const uint8_t* p, uint32_t n)
{
    uint64_t h = start;
    uint32_t k = 0;
    for (; k + 16u <= n; k += 16u) {
        uint64_t w[2];
        __builtin_memcpy(w, p + k, 16);
        h = absorb(absorb(h, w[0]), w[1]);
    }
    if (k + 8u <= n) {
        uint64_t w;
        __builtin_memcpy(&w, p + k, 8);
        h = absorb(h, w);
        k += 8u;
    }
    if (k < n) {
        uint64_t w = 0;
        for (uint32_t b = 0; k + b < n; ++b) w |= uint64_t(p[k + b]) << (8u * b);
        h = absorb(h, w);
    }
    return mix(h);
}

// Node's key for segment j of mate 1 (its bytes at m1).
FQD_SEQ_HD uint64_t node_seed(const uint8_t* m1, uint32_t len1, uint32_t len2, uint32_t D, uint32_t j, bool weak)
{
    const uint32_t from = bound(len1, D, j), to = bound(len1, D, j + 1u);
    const uint64_t key = seed_key(seed_start(len1, len2, j), m1 + from, to - from);
    return weak ? key & kWeakMask : key;
}

// ---- the mismatch counter, kChunk bytes a lane ---------------------------------------------------------------------------------

// Bit 0 of every byte of the result's mask = that byte of x and y differs (fqdseq::mismatches' popcount).
FQD_SEQ_HD uint32_t differing_bytes(uint64_t x, uint64_t y)
{
    uint64_t z = x ^ y;
    z |= z >> 4; z |= z >> 2; z |= z >> 1;
    return uint32_t(__builtin_popcountll(z & 0x0101010101010101ull));
}

// The differing bytes of a and b in chunk c of n bytes: [c * kChunk, min(n, (c + 1) * kChunk)).  0 behind the end.  A whole
// chunk is one 16-byte load a side; the last, partial one goes byte by byte: no load leaves [0, n).
FQD_SEQ_HD uint32_t chunk_mismatches(const uint8_t* a, const uint8_t* b, uint32_t n, uint32_t c)
{
    const uint64_t at = uint64_t(c) * kChunk;
    if (at >= n) return 0u;
    if (at + kChunk <= n) {
        uint64_t x[2], y[2];
        __builtin_memcpy(x, a + at, 16); __builtin_memcpy(y, b + at, 16);
        return differing_bytes(x[0], y[0]) + differing_bytes(x[1], y[1]);
    }
    uint32_t d = 0;
    for (uint32_t k = uint32_t(at); k < n; ++k) d += a[k] != b[k];
    return d;
}

// What a lane group makes of a mate: rounds of kLanes chunks, the lanes' counts summed behind every round, and no further
// round once the sum is above cap.  The result is above cap exactly where the mates differ in more than cap bytes; below, it
// is the number itself.  (The harness plays the lanes one after another; the device sums across them.)
inline uint32_t lanes_mismatches(const uint8_t* a, const uint8_t* b, uint32_t n, uint32_t cap)
{
    uint32_t d = 0;
    for (uint32_t c0 = 0; uint64_t(c0) * kChunk < n && d <= cap; c0 += kLanes)
        for (uint32_t gl = 0; gl < kLanes; ++gl) d += chunk_mismatches(a, b, n, c0 + gl);
    return d;
}

// ---- near ------------------------------------------------------------------------------------------------------------------------

inline bool near(bool paired, fqdseq::View a1, fqdseq::View a2, fqdseq::View b1, fqdseq::View b2, uint32_t D)
{
    if (a1.len != b1.len || (paired && a2.len != b2.len)) return false;
    if (lanes_mismatches(a1.p, b1.p, a1.len, D) > D) return false;
    return !paired || lanes_mismatches(a2.p, b2.p, a2.len, D) <= D;
}

// ---- components: the rule as the device runs it, one step after the other ----------------------------------------------------------
// edges: m pairs (a, b) of labels' places; labels, next: n entries of room.  labels[v] = the lowest place of v's component
// (v itself where no edge names it); returns the sweeps.

FQD_SEQ_HD bool edge_min(const uint32_t* labels, uint32_t a, uint32_t b, uint32_t* to, uint32_t* low)
{
    const uint32_t la = labels[a], lb = labels[b];
    if (la == lb) return false;
    *to = la < lb ? b : a;
    *low = la < lb ? la : lb;
    return true;
}

inline uint32_t components(const uint32_t* edges, uint64_t m, uint32_t n, uint32_t* labels, uint32_t* next)
{
    for (uint32_t v = 0; v < n; ++v) labels[v] = v;
    uint32_t sweeps = 0;
    for (uint32_t t = 0; t < n; ++t) {
        bool changed = false;
        for (uint32_t v = 0; v < n; ++v) next[v] = labels[v];
        for (uint64_t k = 0; k < m; ++k) {
            uint32_t to, low;
            if (!edge_min(labels, edges[2 * k], edges[2 * k + 1], &to, &low)) continue;
            if (low < next[to]) next[to] = low;
            changed = true;                                   // (the higher end's label is above `low`: the step lowers it)
        }
        if (!changed) break;
        for (uint32_t v = 0; v < n; ++v) labels[v] = next[next[v]];
        ++sweeps;
    }
    return sweeps;
}

} // namespace fqdnear
