// fqd_seq_pick_core.hpp — the rules of FQD_SEQ_KEEP=best: which member of a cluster of duplicates is WRITTEN by the
// sequence-based modes.  Shared by the device code (csrc/fqd_seq_pick.hip) and a CPU harness of the tests
// (tests/native/seq_pick_check.cpp builds this header with g++ and the sanitizers).
//
// ---- the score --------------------------------------------------------------------------------------------------------
// A record's score = the sum of (b - 33) over the bytes b >= 33 of its LAST LINE without the '\n' (the quality line of a
// FASTQ record, Phred+33); bytes below 33 count 0 (the '\r' of a CRLF file is one).  The last line of a record of `len`
// bytes: drop the final byte when it is '\n'; what follows the last '\n' of the rest (the whole rest when there is none).
// A sum saturates at 2^32-1; a pair's score is the saturating sum of its mates' scores.  word_score() adds the eight bytes
// of a 64-bit word with masked arithmetic; the device reads a line as such words, eight lanes to a record.
//
// ---- the representative ------------------------------------------------------------------------------------------------
// Clusters are the segments of the sorted order that start at the head flags of fqd_seq_heads (place 0 starts one
// whatever its flag says).  The representative of a cluster = its member with the highest score, the EARLIEST place in
// the sort order among equal scores.  pack(score, place) = score << 32 | (2^32-1 - place) orders exactly that way under
// max: a higher score wins by the high half, among equal scores the smaller place has the larger low half.  Places are
// below 2^32-1, so a packed value of a member is never 0.
//
// ---- the segmented scan -------------------------------------------------------------------------------------------------
// An element of the scan is Pick{best, start}: over a span of places, `start` = the place of the LAST segment start
// inside the span (kNoStart: none) and `best` = the maximum of pack() over the span's places from that start on (over the
// whole span when there is none).  A single place k is {pack(score, k), k if it starts a segment else kNoStart}.
//
//     combine(a, b) = b.start != kNoStart ? b : {max(a.best, b.best), a.start}          (a = the span to the left of b)
//
// That is the element of the joined span: when b holds a segment start, the last start of a+b is b's and what follows it
// lies in b alone; otherwise all of b continues a's last segment (or a's start-less run), so the maxima join and the last
// start is a's.  Associative — combine(combine(a, b), c) == combine(a, combine(b, c)):
//   c has a start:            both sides are c.
//   c has none, b has one:    left = {max(b.best, c.best), b.start}; right = combine(a, {max(b.best, c.best), b.start}),
//                             whose right operand has a start, so it is that operand: the same.
//   neither has one:          left = {max(max(a.best, b.best), c.best), a.start}, right = {max(a.best, max(b.best, c.best)),
//                             a.start}: max is associative.
// The identity is {0, kNoStart}.  So the inclusive scan may be cut into lanes, waves, workgroups and tiles at any place
// and joined in order.  At the LAST place of a segment the inclusive scan holds the segment's start and its best member:
// that place (one per segment) reports them, and the order entries of the two places are swapped afterwards.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FQD_PICK_HD __host__ __device__ __forceinline__
#else
#define FQD_PICK_HD inline
#endif

namespace fqdseq {

constexpr uint32_t kScoreBase = 33;                       // Phred+33
constexpr uint32_t kNoStart = 0xFFFFFFFFu;

FQD_PICK_HD uint32_t byte_score(uint8_t b) { return b >= kScoreBase ? uint32_t(b) - kScoreBase : 0u; }

FQD_PICK_HD uint32_t saturate_score(uint64_t sum) { return sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(sum); }

FQD_PICK_HD uint32_t add_scores(uint32_t a, uint32_t b) { return saturate_score(uint64_t(a) + b); }

// The sum of byte_score over the eight bytes of x (at most 8 x 222).  The even and the odd bytes go through 16-bit
// fields: (v | 0x100) - 33 keeps bit 8 exactly when v >= 33 and then holds v - 33 below it; no field borrows from its
// neighbour.  The four fields of a half are added by one multiply (a sum stays below 2^16).
FQD_PICK_HD uint32_t word_score(uint64_t x)
{
    constexpr uint64_t kLow = 0x00FF00FF00FF00FFull, kOne = 0x0001000100010001ull;
    const uint64_t te = ((x & kLow) | (kOne << 8)) - kOne * kScoreBase;
    const uint64_t to = (((x >> 8) & kLow) | (kOne << 8)) - kOne * kScoreBase;
    const uint64_t ve = te & (((te >> 8) & kOne) * 0xFFu), vo = to & (((to >> 8) & kOne) * 0xFFu);
    return uint32_t(((ve + vo) * kOne) >> 48);
}

// 0x80 in every byte of x that is '\n', 0 elsewhere (exact: no carry leaves a byte).
FQD_PICK_HD uint64_t newline_bytes(uint64_t x)
{
    constexpr uint64_t k7F = 0x7F7F7F7F7F7F7F7Full;
    const uint64_t y = x ^ 0x0A0A0A0A0A0A0A0Aull;
    return ~(((y & k7F) + k7F) | y | k7F);
}

// x holds eight bytes of text, the first in its low byte.  The score of the bytes BEHIND the last '\n' among them (of
// all eight when there is none); *found says whether there was one.
FQD_PICK_HD uint32_t word_score_after_newline(uint64_t x, bool* found)
{
    const uint64_t z = newline_bytes(x);
    *found = z != 0;
    if (!z) return word_score(x);
    const uint32_t j = (63u - uint32_t(__builtin_clzll(z))) >> 3;       // the byte of the last '\n'
    return j == 7u ? 0u : word_score(x >> (8u * (j + 1u)));             // zeros come in from above: they count 0
}

// The rule itself, byte by byte (what the harness and the tests hold the words against).
inline uint32_t last_line_score(const uint8_t* rec, uint64_t len)
{
    if (len && rec[len - 1] == '\n') --len;
    uint64_t from = len;
    while (from > 0 && rec[from - 1] != '\n') --from;
    uint64_t sum = 0;
    for (uint64_t k = from; k < len; ++k) sum += byte_score(rec[k]);
    return saturate_score(sum);
}

FQD_PICK_HD uint64_t pack_pick(uint32_t score, uint32_t place) { return (uint64_t(score) << 32) | uint64_t(0xFFFFFFFFu - place); }
FQD_PICK_HD uint32_t picked_place(uint64_t packed) { return 0xFFFFFFFFu - uint32_t(packed); }

struct Pick {
    uint64_t best;
    uint32_t start;
};

FQD_PICK_HD Pick pick_identity() { return Pick{0ull, kNoStart}; }

FQD_PICK_HD Pick pick_of(uint32_t score, uint32_t place, bool starts) { return Pick{pack_pick(score, place), starts ? place : kNoStart}; }

FQD_PICK_HD Pick combine(Pick a, Pick b)
{
    if (b.start != kNoStart) return b;
    return Pick{a.best > b.best ? a.best : b.best, a.start};
}

} // namespace fqdseq
