// fqd_optical_core.hpp — the rule of FQD_FAST_OPTICAL=D: where on the flow cell a record was read, which records of one
// cluster of identical reads lie so close together that they are one molecule read twice (an optical duplicate), and how a
// cluster falls apart into such groups.  Shared by the device code (csrc/fqd_optical.hip) and a CPU harness of the tests
// (tests/native/optical_check.cpp builds this header with g++ and the sanitizers).
//
// ---- the place of a record ---------------------------------------------------------------------------------------------
// W          fqd_umi_core.hpp's first word of file 1's ID line: the bytes behind position 0 ('@' / '>') up to, not including,
//            the first of ' ', '\t', '\r', '\n' (the line's end where none occurs); wend = its end's position.
// fields     W split at ':' (Casava 1.8+ / bcl-convert: instrument:run:flowcell:lane:tile:x:y[:UMI]); c1 < c2 < ... are the
//            positions of W's colons.  Fields behind the 7th are not looked at.
// surface    the bytes [1, c4): fields 1 .. 4 with the three colons between them; its length is c4 - 1.
// tile, x    fields 5 and 6, [c4 + 1, c5) and [c5 + 1, c6): 1 .. 9 decimal digits each, leading zeros allowed.
// y          the leading 1 .. 9 decimal digits of field 7, which starts at c6 + 1 and ends at c7 (wend where W has six
//            colons only); what follows them is the field's end or one of ':' '_' '#' '/'.
// A record is refused for the FIRST of these that holds (the numbers are fqd_places_info.bad_reason):
//   1 kFewFields   W holds fewer than six colons
//   2 kEmptyField  one of the fields 1 .. 7 is empty
//   3 kNotDigit    tile or x holds a byte that is no digit, or y does not begin with one      } judged field by field,
//   4 kTooLong     tile or x has more than nine digits, or y begins with more than nine       } tile, then x, then y:
//   5 kBadEnd      y's digits are followed by a byte other than ':' '_' '#' '/'               } the first field's reason
// and a run is refused at the LOWEST refused record.  All values are below 10^9 < 2^30: differences of two of them are
// taken as |a - b| = a > b ? a - b : b - a in 32 bits, without wrap-around.
//
// ---- neighbours, optical groups ------------------------------------------------------------------------------------------
// Two records of one cluster are neighbours when their surfaces are bytewise identical (same length, same bytes: no hash
// decides), their tiles are equal, and |xa - xb| <= D and |ya - yb| <= D (Picard's box, integers only).  The relation is
// symmetric; an optical group is a connected component of it, owned by (written as) its first member in input order.
// The surface word of a record is its surface's length with kSameSurface set where the surface is record 0's: two records
// that both have the bit have one surface, one that has it and one that has not differ, and only two without it are
// compared byte by byte (lengths first).  Nearly every real run has one surface, so that compare hardly ever runs.
//
// ---- the parallel form -----------------------------------------------------------------------------------------------------
// The members of a cluster stand in input order (fqd_group_owners); pos = a member's place in it, label(v) starts as pos(v).
// One sweep is two steps, every member at once, each step reading only what the step before left:
//   min    L'[v] = min(L[v], min over the neighbours u of v of L[u])
//   jump   L[v]  = L'[L'[v]]                                         (pointer jumping)
// and the sweeps end with the first min step that changes nothing (that step is not counted).
// (a) L[v] <= v, and L[v] is the pos of a member of v's group, always: true at the start; a min step takes v's own label or
//     a lower one of a neighbour, which names a member of the neighbour's group, that is of v's; a jump takes the label of
//     a member w = L'[v] of v's group, and L'[w] <= w = L'[v].  So no step raises a label.
// (b) After t sweeps L[v] <= min{pos(u) : u within t edges of v}: the min step gives min over the neighbours' bounds, that is
//     the bound for t + 1, and the jump only lowers.  With (a), L[v] >= the lowest pos m of v's group; so after at most
//     ecc <= s - 1 sweeps (s = the cluster's members) every label IS m, and the next min step changes nothing.  Every loop
//     below is bounded by s sweeps.
// (c) Where a min step changes nothing, every member's label is <= its neighbours' and, the relation being symmetric, equal
//     to them: constant c on a group.  By (a) c <= m and c names a member: c = m.  The fixed point is unique.
// (d) Every step reads one array and writes another (registers behind a barrier, or a second array), so what a step computes
//     depends on the labels before it alone, never on the order in which lanes, waves or blocks run: the labels after every
//     sweep, and with them the NUMBER of sweeps, are the same for eight lanes, a wave, a block or many blocks.
#pragma once
#include <cstdint>

#include "fqd_umi_core.hpp"

#define FQD_OPTICAL_MAX_CLUSTER 65536u

namespace fqdoptical {

constexpr uint32_t kMaxCluster = FQD_OPTICAL_MAX_CLUSTER;     // members of a cluster at most
constexpr uint32_t kSmall = 8;                                // up to here: eight lanes a cluster, eight clusters a wave
constexpr uint32_t kWave = 64;                                // up to here: a wave a cluster
constexpr uint32_t kBlockLimit = 2048;                        // up to here: a workgroup a cluster, places and labels in LDS; beyond: the large tier
constexpr uint32_t kMaxDigits = 9;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kSameSurface = 0x80000000u;                // in a surface word: the surface is record 0's
constexpr uint32_t kGroup = 16;                               // lanes a record (parse)

enum Reason : uint32_t { kOk = 0, kFewFields = 1, kEmptyField = 2, kNotDigit = 3, kTooLong = 4, kBadEnd = 5 };

struct Place { uint32_t tile, x, y, surface, reason; };       // surface: the length (the parse never sets kSameSurface)

FQD_UMI_HD bool is_digit(uint8_t b) { return b >= '0' && b <= '9'; }
FQD_UMI_HD bool ends_y(uint8_t b) { return b == ':' || b == '_' || b == '#' || b == '/'; }

// A field [from, to) that is all number (tile, x): its value and kOk, or why not.  from < to.
FQD_UMI_HD uint32_t whole_number(const uint8_t* line, uint32_t from, uint32_t to, uint32_t* value)
{
    uint32_t v = 0;
    for (uint32_t p = from; p < to; ++p) {
        if (!is_digit(line[p])) return kNotDigit;
        if (p - from < kMaxDigits) v = v * 10u + uint32_t(line[p] - '0');
    }
    *value = v;
    return to - from > kMaxDigits ? uint32_t(kTooLong) : uint32_t(kOk);
}

// The digits a field [from, to) begins with (y): their value and kOk, or why not.  from < to.
FQD_UMI_HD uint32_t leading_number(const uint8_t* line, uint32_t from, uint32_t to, uint32_t* value)
{
    uint32_t v = 0, nd = 0;
    while (nd <= kMaxDigits && from + nd < to && is_digit(line[from + nd])) {
        if (nd < kMaxDigits) v = v * 10u + uint32_t(line[from + nd] - '0');
        ++nd;
    }
    if (nd == 0) return kNotDigit;
    if (nd > kMaxDigits) return kTooLong;
    *value = v;
    return from + nd < to && !ends_y(line[from + nd]) ? uint32_t(kBadEnd) : uint32_t(kOk);
}

// The verdict from what was found: W's colons (counted up to seven), c[0 .. 3] = c4 .. c7 (kNone where W has fewer), W's end,
// whether one of the first seven colons ends an empty field, and the three fields' own reasons and values.
FQD_UMI_HD Place judge(uint32_t colons, const uint32_t* c, uint32_t wend, bool empty, const uint32_t* field_reason, const uint32_t* value)
{
    Place p{0u, 0u, 0u, 0u, kOk};
    if (colons < 6u) { p.reason = kFewFields; return p; }
    const uint32_t yend = colons >= 7u ? c[3] : wend;
    if (empty || c[2] + 1u >= yend) { p.reason = kEmptyField; return p; }
    p.surface = c[0] - 1u;
    for (uint32_t f = 0; f < 3u; ++f) if (field_reason[f]) { p.reason = field_reason[f]; return p; }
    p.tile = value[0]; p.x = value[1]; p.y = value[2];
    return p;
}

// Field f (0 tile, 1 x, 2 y) of a line whose colons c4 .. c7 and word end are known and whose fields are not empty.
FQD_UMI_HD uint32_t field_number(const uint8_t* line, const uint32_t* c, uint32_t colons, uint32_t wend, uint32_t f, uint32_t* value)
{
    if (f < 2u) return whole_number(line, c[f] + 1u, c[f + 1u], value);
    return leading_number(line, c[2] + 1u, colons >= 7u ? c[3] : wend, value);
}

// ---- the rule record by record -------------------------------------------------------------------------------------------

FQD_UMI_HD Place parse(const uint8_t* line, uint32_t len)
{
    uint32_t wend = len, colons = 0, c[4] = {kNone, kNone, kNone, kNone}, last = 0;
    bool empty = false;
    for (uint32_t i = 1; i < len; ++i)
        if (fqdumi::is_word_end(line[i])) { wend = i; break; }
    for (uint32_t i = 1; i < wend && colons < 7u; ++i) {
        if (line[i] != ':') continue;
        ++colons;
        if (i == last + 1u) empty = true;                     // (last = 0 at first: a colon at position 1 ends an empty field 1)
        if (colons >= 4u) c[colons - 4u] = i;
        last = i;
    }
    uint32_t reason[3] = {kOk, kOk, kOk}, value[3] = {0u, 0u, 0u};
    if (colons >= 6u && !empty && c[2] + 1u < (colons >= 7u ? c[3] : wend))
        for (uint32_t f = 0; f < 3u; ++f) reason[f] = field_number(line, c, colons, wend, f, &value[f]);
    return judge(colons, c, wend, empty, reason, value);
}

// Is this record's surface (its line, its colon c4) record 0's?  line0[1 .. c4] = line[1 .. c4], the colon included: then
// line 0's fourth colon stands at c4 as well (the bytes in front hold three), and the surfaces are the same bytes.
FQD_UMI_HD bool surface_byte_same(const uint8_t* line0, uint32_t len0, const uint8_t* line, uint32_t k) { return k < len0 && line0[k] == line[k]; }

FQD_UMI_HD bool surface_is_record0s(const uint8_t* line0, uint32_t len0, const uint8_t* line, uint32_t c4)
{
    for (uint32_t k = 1; k <= c4; ++k) if (!surface_byte_same(line0, len0, line, k)) return false;
    return true;
}

// ---- sixteen lanes a record (csrc/fqd_optical.hip; the harness plays the lanes one after another) --------------------------
// rounds  fqd_umi_core.hpp's lane_look with ':' for the separator: lane gl holds the colons of its sixteen bytes as a mask.
//         `before` = W's colons in front of the lane's chunk (the rounds before, and the lanes below it in this round: an
//         exclusive sum across the group).  The lane owns those of the first seven colons that lie in its chunk below the
//         word's end: it notes the positions of the 4th .. 7th and looks, with one byte load each, whether the byte in front
//         is a colon too (an empty field).  The group takes the minimum of the positions and the sum of the counts.
// fields  lanes 0, 1 and 2 read tile, x and y (field_number); all sixteen compare the surface with record 0's, a byte a lane.

struct Colons { uint32_t count; uint32_t at[4]; bool empty; };  // this lane's colons below `end`; at: c4 .. c7 where the lane owns them

// The lane's colons below `end`, the word's end as far as the group has seen it (kNone: not yet), as a mask.
FQD_UMI_HD uint32_t colons_below(const fqdumi::Look& k, uint32_t end)
{
    if (end == fqdumi::kNone) return k.seps;
    return end <= k.base ? 0u : end - k.base >= 16u ? k.seps : k.seps & ((1u << (end - k.base)) - 1u);
}

FQD_UMI_HD Colons lane_colons(const uint8_t* line, const fqdumi::Look& k, uint32_t end, uint32_t before)
{
    Colons got{0u, {kNone, kNone, kNone, kNone}, false};
    uint32_t m = colons_below(k, end);
    got.count = uint32_t(__builtin_popcount(m));
    uint32_t rank = before;
    for (; m && rank < 7u; m &= m - 1u) {
        const uint32_t p = k.base + uint32_t(__builtin_ctz(m));
        ++rank;
        if (rank >= 4u) got.at[rank - 4u] = p;
        if (p == 1u || line[p - 1u] == ':') got.empty = true;  // (p >= 1: position 0 is never a separator)
    }
    return got;
}

// ---- neighbours ------------------------------------------------------------------------------------------------------------

FQD_UMI_HD uint32_t gap(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

// Tile and box; the surfaces are looked at by surfaces_same.
FQD_UMI_HD bool close(uint32_t ta, uint32_t xa, uint32_t ya, uint32_t tb, uint32_t xb, uint32_t yb, uint32_t D)
{
    return ta == tb && gap(xa, xb) <= D && gap(ya, yb) <= D;
}

// From the surface words alone: 1 the same, 0 different, 2 the bytes must be compared (same length, neither is record 0's).
FQD_UMI_HD uint32_t surfaces_quick(uint32_t sa, uint32_t sb)
{
    if ((sa & sb) & kSameSurface) return 1u;
    if (((sa ^ sb) & kSameSurface) || sa != sb) return 0u;
    return 2u;
}

FQD_UMI_HD bool bytes_same(const uint8_t* a, const uint8_t* b, uint32_t len)
{
    for (uint32_t k = 0; k < len; ++k) if (a[k] != b[k]) return false;
    return true;
}

// Members u and v of a cluster whose places stand in four arrays (LDS, or the per-record arrays through rec_of).
// bytes_of(member) = where its surface's bytes start.
template <class BytesOf>
FQD_UMI_HD bool near_at(const uint32_t* T, const uint32_t* X, const uint32_t* Y, const uint32_t* S, uint32_t u, uint32_t v, uint32_t D, BytesOf bytes_of)
{
    if (!close(T[u], X[u], Y[u], T[v], X[v], Y[v], D)) return false;
    const uint32_t q = surfaces_quick(S[u], S[v]);
    return q == 2u ? bytes_same(bytes_of(u), bytes_of(v), S[u]) : q == 1u;
}

// ---- a lane a member: clusters of up to 64 -----------------------------------------------------------------------------------

// Bit u of the result: u is a neighbour of this lane's member.  place_of(u, &t, &x, &y, &s) = member u's place and
// bytes_of(u) its surface's bytes, asked of every u < s_all by every lane (on the device cross-lane reads that the whole
// group takes part in); live = the lane holds a member.
template <class PlaceOf, class BytesOf>
FQD_UMI_HD uint64_t lane_neighbours(bool live, uint32_t v, uint32_t s, uint32_t s_all, uint32_t t, uint32_t x, uint32_t y, uint32_t sw, const uint8_t* bytes,
                                    uint32_t D, PlaceOf place_of, BytesOf bytes_of)
{
    uint64_t m = 0;
    for (uint32_t u = 0; u < s_all; ++u) {
        uint32_t tu, xu, yu, su;
        place_of(u, &tu, &xu, &yu, &su);
        const uint8_t* bu = bytes_of(u);
        if (!live || u >= s || u == v || !close(tu, xu, yu, t, x, y, D)) continue;
        const uint32_t q = surfaces_quick(su, sw);
        if (q == 2u ? bytes_same(bu, bytes, sw) : q == 1u) m |= 1ull << u;
    }
    return m;
}

// The min step of lane v: old_of(u) = the label lane u held when the step began.
template <class OldOf>
FQD_UMI_HD uint32_t lane_min(uint64_t neighbours, uint32_t own, uint32_t s_all, OldOf old_of)
{
    uint32_t best = own;
    for (uint32_t u = 0; u < s_all; ++u) {
        const uint32_t lu = old_of(u);
        if (((neighbours >> u) & 1u) && lu < best) best = lu;
    }
    return best;
}

// ---- a block a cluster, and the large tier: the labels in one array that is read between two barriers (two launches) ---------

// Member v's label after a min step over `labels`.  A member u is looked at closely only where its label would lower v's.
template <class BytesOf>
FQD_UMI_HD uint32_t array_min(const uint32_t* T, const uint32_t* X, const uint32_t* Y, const uint32_t* S, const uint32_t* labels, uint32_t s, uint32_t D,
                              uint32_t v, BytesOf bytes_of)
{
    uint32_t best = labels[v];
    for (uint32_t u = 0; u < s; ++u)
        if (labels[u] < best && near_at(T, X, Y, S, u, v, D, bytes_of)) best = labels[u];
    return best;
}

// ---- the rule cluster by cluster (what the lanes must agree with; the host's way to state it) --------------------------------

// labels[v] = the lowest pos of v's group; returns the sweeps.  next: s entries of room.
template <class BytesOf>
inline uint32_t split_cluster(const uint32_t* T, const uint32_t* X, const uint32_t* Y, const uint32_t* S, uint32_t s, uint32_t D, uint32_t* labels,
                              uint32_t* next, BytesOf bytes_of)
{
    for (uint32_t v = 0; v < s; ++v) labels[v] = v;
    uint32_t sweeps = 0;
    for (uint32_t t = 0; t < s; ++t) {
        bool changed = false;
        for (uint32_t v = 0; v < s; ++v) { next[v] = array_min(T, X, Y, S, labels, s, D, v, bytes_of); changed |= next[v] != labels[v]; }
        if (!changed) break;
        for (uint32_t v = 0; v < s; ++v) labels[v] = next[next[v]];
        ++sweeps;
    }
    return sweeps;
}

} // namespace fqdoptical
