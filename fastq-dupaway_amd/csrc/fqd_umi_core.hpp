// fqd_umi_core.hpp — the rule of FQD_FAST_UMI=colon|underscore: which bytes of a record's ID line are its unique molecular
// identifier, and how they enter the key, so that two reads of one sequence and different UMIs stay two molecules.  Shared
// by the device code (csrc/fqd_umi.hip) and a CPU harness of the tests (tests/native/umi_check.cpp builds this header with
// g++ and the sanitizers).
//
// ---- definitions -----------------------------------------------------------------------------------------------------
// ID line   the bytes [start, start + id_len) of a record of file 1: '@' or '>' first, '\n' last.  File 2's ID lines are
//           not looked at (bcl-convert, fastp and umi_tools write the same UMI into both files).
// W         the first word: the bytes behind the leading '@' / '>' up to, not including, the first of ' ', '\t', '\r',
//           '\n' (the line's end where none of them occurs).  Nothing behind W counts: a separator in the comment is none.
// U         the UMI field: the bytes of W behind the LAST separator byte in W (':' for colon, '_' for underscore).
//           umi_off = U's offset inside the ID line (the separator's position + 1; 0 where W holds no separator).
// joiners   '+', '-' and '_' inside U join the halves of a dual UMI; every other byte of U must be one of A C G T N.
// shape(U)  (its length, the set of its positions that hold a joiner): (umi_len, joiners) with bit p of joiners = U[p] is
//           a joiner.  U is at most 64 bytes, so the set is one 64-bit word.
// B(U)      U with the joiners taken out, Lb = umi_len - popcount(joiners) bytes.
// key       B(U) ‖ seq of mate 1 (with FQD_FAST_STRAND=both: of the canonical mate 1); mate 2 as it is.
//
// A record is refused for the FIRST of these that holds (the numbers are fqd_umi_info.bad_reason):
//   1 W holds no separator            4 U holds a byte outside ACGTN+-_
//   2 U is empty                      5 U has no base (joiners only)
//   3 U is longer than 64 bytes       6 U's shape differs from record 0's
// and a run is refused at the LOWEST refused record.  Record 0 is judged by 1 .. 5 only; its shape is the run's.
//
// ---- one fixed shape makes the key exact -----------------------------------------------------------------------------------
// Let U and U' have the same shape (L, J) and write U ~ U' when they hold the same base at every place outside J (over
// one joiner character, as in any one file's convention, that is U = U'; AC+GT and AC-GT are one label).
// (a) B(U) = B(U') <=> U ~ U'.  The places outside J in ascending order are one list p_0 < p_1 < ... < p_(Lb-1) for both,
//     and B(U)[j] = U[p_j], B(U')[j] = U'[p_j]: the two sides say the same thing place by place.
// (b) Every B has the one length Lb = L - |J|, so B ‖ seq splits at a fixed place: B ‖ seq = B' ‖ seq' <=> B = B' and
//     seq = seq'.  With (a): two records have one key exactly when their UMIs agree base for base and their sequences
//     are identical.
// Without the fixed shape neither holds: AC+GTA and ACG+TA both give ACGTA, and ACGT ‖ A... equals ACG ‖ TA....  A file
// that holds both is refused (reason 6), never merged.  UMIs of varying length are out of scope.
//
// ---- sixteen lanes a record (csrc/fqd_umi.hip; tests/native/umi_check.cpp plays the lanes one after another) ------------------
// find   in a round lane gl (0 .. 15) looks at chunk c0 + gl of the line: sixteen bytes (one byte a lane for lines under
//        sixteen bytes) as two 16-bit masks, word ends and separators.  The group takes the minimum of look_end over its
//        lanes — the word's end, if the round holds it — and then the maximum of look_sep, the last separator below that
//        end; rounds go on while no lane has seen the end.  Every load lies inside the line.
// class  U is at most 64 bytes: lane gl classifies U[gl], U[gl + 16], U[gl + 32], U[gl + 48].
// gather the Lb bases go one byte a lane through a table of their places in U (bases_table); the shape is fixed, so the
//        table is the same for every record of a run.
#pragma once
#include <cstdint>

#include "fqd_strand_core.hpp"                               // zero_bytes

#if defined(__HIPCC__)
#define FQD_UMI_HD __host__ __device__ __forceinline__
#else
#define FQD_UMI_HD inline
#endif

namespace fqdumi {

constexpr uint32_t kMaxUmi = 64;                              // bytes of U at most
constexpr uint32_t kNone = 0xFFFFFFFFu;

enum Reason : uint32_t { kOk = 0, kNoSeparator = 1, kEmpty = 2, kTooLong = 3, kBadByte = 4, kNoBase = 5, kShapeDiffers = 6 };

FQD_UMI_HD bool is_word_end(uint8_t b) { return b == ' ' || b == '\t' || b == '\r' || b == '\n'; }
FQD_UMI_HD bool is_joiner(uint8_t b) { return b == '+' || b == '-' || b == '_'; }
FQD_UMI_HD bool is_base(uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T' || b == 'N'; }

// ---- find ------------------------------------------------------------------------------------------------------------

// Chunks of a line of len bytes (rounds = chunks over sixteen, rounded up): lines under sixteen bytes take ONE chunk with
// one byte a lane; longer ones len/16 chunks and, when len is no multiple of sixteen, the last sixteen bytes once more.
FQD_UMI_HD uint32_t line_chunks(uint32_t len) { return len == 0 ? 0u : len < 16u ? 1u : (len >> 4) + ((len & 15u) ? 1u : 0u); }

// Four bytes at a time (little-endian dwords, as in fqd_strand_core.hpp).  nibble: bit j = byte j of z has its top bit set,
// for a z with nothing but top bits (the products 2^(8j+7) * 2^(21-7j) land on bits 21 .. 24, all others elsewhere: no
// carry reaches them).  bytes_up_to_blank: 0x80 in every byte of x that is <= ' ' (0x20), 0 elsewhere.
FQD_UMI_HD uint32_t nibble(uint32_t z) { return (((z >> 7) * 0x00204081u) >> 21) & 0xFu; }
FQD_UMI_HD uint32_t bytes_up_to_blank(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x5F5F5F5Fu) | x) & 0x80808080u; }

// What a lane has seen: bit k of the masks = position base + k of the line.
struct Look { uint32_t base, ends, seps; };

// Lane gl's look at round c0.  Position 0 (the '@' / '>') is never a word end nor a separator.
FQD_UMI_HD Look lane_look(const uint8_t* line, uint32_t len, uint8_t sep, uint32_t c0, uint32_t gl)
{
    Look k{0u, 0u, 0u};
    if (len < 16u) {
        if (c0 != 0 || gl >= len || gl == 0) return k;
        const uint8_t b = line[gl];
        k.base = gl; k.ends = is_word_end(b) ? 1u : 0u; k.seps = b == sep ? 1u : 0u;
        return k;
    }
    const uint32_t c = c0 + gl, full = len >> 4;
    if (c >= line_chunks(len)) return k;
    k.base = 16u * c;
    const uint32_t q = c < full ? k.base : len - 16u;          // (the last chunk: loaded from len-16 on, its new bytes kept)
    uint32_t w[4];
    __builtin_memcpy(w, line + q, 16);
    uint32_t ends = 0, seps = 0, low = 0;
    for (uint32_t d = 0; d < 4u; ++d) {
        seps |= nibble(fqdstrand::zero_bytes(w[d] ^ (0x01010101u * sep))) << (4u * d);
        low |= bytes_up_to_blank(w[d]);
    }
    if (low)                                                   // (a word end is a byte up to ' ': most chunks hold none)
        for (uint32_t d = 0; d < 4u; ++d)
            ends |= nibble(fqdstrand::zero_bytes(w[d] ^ 0x20202020u) | fqdstrand::zero_bytes(w[d] ^ 0x09090909u) |
                           fqdstrand::zero_bytes(w[d] ^ 0x0A0A0A0Au) | fqdstrand::zero_bytes(w[d] ^ 0x0D0D0D0Du)) << (4u * d);
    k.ends = ends >> (k.base - q); k.seps = seps >> (k.base - q);
    if (c == 0) { k.ends &= ~1u; k.seps &= ~1u; }
    return k;
}

// The position of the first word end the lane has seen, kNone for none.
FQD_UMI_HD uint32_t look_end(const Look& k) { return k.ends ? k.base + uint32_t(__builtin_ctz(k.ends)) : kNone; }

// 1 + the position of the last separator below `end` the lane has seen, 0 for none.
FQD_UMI_HD uint32_t look_sep(const Look& k, uint32_t end)
{
    if (end <= k.base) return 0u;
    const uint32_t below = end - k.base >= 16u ? k.seps : k.seps & ((1u << (end - k.base)) - 1u);
    return below ? k.base + 32u - uint32_t(__builtin_clz(below)) : 0u;
}

// ---- class -------------------------------------------------------------------------------------------------------------

// Lane gl's four bytes of U (ulen <= 64): bit k of *joiner4 = U[gl + 16k] is a joiner; *bad = one of them is neither a
// joiner nor a base.  Every load lies in U[0 .. ulen).
FQD_UMI_HD void lane_class(const uint8_t* U, uint32_t ulen, uint32_t gl, uint32_t* joiner4, bool* bad)
{
    uint32_t j = 0;
    bool x = false;
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t p = gl + 16u * k;
        if (p >= ulen) break;
        const uint8_t b = U[p];
        if (is_joiner(b)) j |= 1u << k;
        else if (!is_base(b)) x = true;
    }
    *joiner4 = j; *bad = x;
}

// The verdict over one record from what its sixteen lanes found (have0: record 0's shape is known and this is not it).
FQD_UMI_HD uint32_t verdict(bool has_sep, uint32_t ulen, uint64_t joiners, bool any_bad, bool have0, uint32_t ulen0, uint64_t joiners0)
{
    if (!has_sep) return kNoSeparator;
    if (ulen == 0) return kEmpty;
    if (ulen > kMaxUmi) return kTooLong;
    if (any_bad) return kBadByte;
    if (uint32_t(__builtin_popcountll(joiners)) == ulen) return kNoBase;
    if (have0 && (ulen != ulen0 || joiners != joiners0)) return kShapeDiffers;
    return kOk;
}

// ---- gather --------------------------------------------------------------------------------------------------------------

struct Table { uint8_t at[kMaxUmi]; };                          // at[j] = the place in U of base j, j < Lb

// The places outside the joiner set in ascending order; returns Lb.
FQD_UMI_HD uint32_t bases_table(uint32_t ulen, uint64_t joiners, Table* t)
{
    uint32_t lb = 0;
    for (uint32_t p = 0; p < kMaxUmi; ++p) t->at[p] = 0;
    for (uint32_t p = 0; p < ulen && p < kMaxUmi; ++p)
        if (!((joiners >> p) & 1u)) t->at[lb++] = uint8_t(p);
    return lb;
}

// Lane gl's share of dst[0 .. lb) = B(U): bases gl, gl + 16, ...  Every load lies in U, every store in dst[0 .. lb).
FQD_UMI_HD void gather_lane(const uint8_t* U, const Table& t, uint32_t lb, uint8_t* dst, uint32_t gl)
{
    for (uint32_t j = gl; j < lb; j += 16u) dst[j] = U[t.at[j]];
}

// ---- the rule record by record (what the lanes must agree with; also the host's way to state it) -------------------------

struct Field { uint32_t off, len; bool has_sep; };            // U = line[off .. off + len)

FQD_UMI_HD Field find_field(const uint8_t* line, uint32_t len, uint8_t sep)
{
    uint32_t end = len, last = 0;
    for (uint32_t i = 1; i < len; ++i)
        if (is_word_end(line[i])) { end = i; break; }
    for (uint32_t i = 1; i < end; ++i)
        if (line[i] == sep) last = i;
    if (!last) return Field{0u, 0u, false};
    return Field{last + 1u, end - last - 1u, true};
}

// The reason a record is refused (kOk: it is not) and, for a U of at most 64 bytes, its joiner set.
FQD_UMI_HD uint32_t judge(const uint8_t* line, uint32_t len, uint8_t sep, bool have0, uint32_t ulen0, uint64_t joiners0, Field* f, uint64_t* joiners)
{
    *f = find_field(line, len, sep);
    uint64_t j = 0;
    bool bad = false;
    for (uint32_t p = 0; p < f->len && p < kMaxUmi; ++p) {
        const uint8_t b = line[f->off + p];
        if (is_joiner(b)) j |= 1ull << p;
        else if (!is_base(b)) bad = true;
    }
    *joiners = j;
    return verdict(f->has_sep, f->len, j, bad, have0, ulen0, joiners0);
}

} // namespace fqdumi
