// fqd_strand_core.hpp — the rule of FQD_FAST_STRAND=both: the orientation in which a read (pair) is keyed, so that the two
// strands of one fragment get one key.  Shared by the device code (csrc/fqd_strand.hip) and a CPU harness of the tests
// (tests/native/strand_check.cpp builds this header with g++ and the sanitizers).
//
// ---- definitions -----------------------------------------------------------------------------------------------------
// comp(b): 'A' <-> 'T', 'C' <-> 'G', every other byte ('N' included) maps to itself.  comp(comp(b)) = b.
// rc(s)[i] = comp(s[L-1-i]) for a sequence s of L bytes.  rc(rc(s)) = s (the mirror and comp are both involutions).
//
// Single-end.  canon(s) = the bytewise smaller of s and rc(s) (equal lengths: a plain unsigned byte compare);
//   flipped(s) = rc(s) < s, strictly: a read that is its own reverse complement is not flipped.
//   Function of the set:  canon(rc(s)) = min(rc(s), s) = canon(s).
//   Duplicates:  canon(t) == canon(s)  <=>  t == s or t == rc(s).  (<=) by the line above.  (=>) canon(t) is t or rc(t),
//   canon(s) is s or rc(s); whichever two are equal, applying rc to both sides where needed gives t in {s, rc(s)}.
//   Half the read decides.  Let D = { i : s[i] != comp(s[L-1-i]) }, the places where s and rc(s) differ.  Since comp is
//   an involution, s[i] != comp(s[L-1-i]) <=> comp(s[i]) != s[L-1-i] <=> (L-1-i) in D: D is symmetric under
//   i -> L-1-i.  So its smallest member i0 has i0 <= L-1-i0, that is i0 <= (L-1)/2, and the compare never has to look
//   beyond position (L-1)/2: half(L) = (L+1)/2 positions.
//
// Pairs.  No complementing: mate 2 is sequenced from the other end of the fragment on the opposite strand, so it already
//   IS the other strand's 5' end, read 5' to 3'.  The copy that comes off the other strand therefore has the same two
//   byte strings with the mates exchanged: its R1 is this copy's R2 and the reverse.  canon(a, b) = (a, b) if a <= b,
//   else (b, a); flipped = b < a.  The order is bytewise over the shorter length, the shorter read first on a tie
//   (the order of Python's bytes).  The exchange is an involution, so as above canon is a function of the set
//   {(a,b), (b,a)} and two pairs are strand-duplicates exactly when their canonical forms are identical, lengths included.
//
// Bytes outside {A,C,G,T,N} are not judged here: they pass through at their mirrored place (comp leaves them alone) and
// the engine refuses them when the canonical reads are keyed, as it does today.
//
// ---- sixteen bytes at a time --------------------------------------------------------------------------------------------
// The kernel moves reads as 16-byte chunks (four little-endian dwords: byte j of the chunk is byte j%4 of w[j/4]).
// rc16(m) is the reverse complement of a chunk: byte j = comp(byte 15-j of m).  With M = the 16 bytes s[L-16-q .. L-q)
// that is rc(s)[q .. q+16).  first_diff16 finds the first byte at which two chunks differ and says which is smaller.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FQD_STRAND_HD __host__ __device__ __forceinline__
#else
#define FQD_STRAND_HD inline
#endif

namespace fqdstrand {

FQD_STRAND_HD uint8_t comp(uint8_t b)
{
    return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b;
}

// 0x80 in every byte of x that is zero, 0 elsewhere (no carry leaves a byte: the add is over 7-bit fields).
FQD_STRAND_HD uint32_t zero_bytes(uint32_t x)
{
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | x | 0x7F7F7F7Fu);
}

// comp of four bytes at once: 'A' ^ 'T' = 0x15, 'C' ^ 'G' = 0x04.
FQD_STRAND_HD uint32_t comp4(uint32_t v)
{
    const uint32_t at = (zero_bytes(v ^ 0x41414141u) | zero_bytes(v ^ 0x54545454u)) >> 7;     // 0x01 per byte that is A or T
    const uint32_t cg = (zero_bytes(v ^ 0x43434343u) | zero_bytes(v ^ 0x47474747u)) >> 7;
    return v ^ (at * 0x15u) ^ (cg * 0x04u);
}

FQD_STRAND_HD uint32_t bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

// Positions 0 .. half(L)-1 decide a single-end read (the lemma above).
FQD_STRAND_HD uint32_t half(uint32_t L) { return (L + 1u) >> 1; }

struct Chunk { uint32_t w[4]; };

FQD_STRAND_HD Chunk rc16(const Chunk& m)
{
    Chunk r;
    r.w[0] = comp4(bswap32(m.w[3])); r.w[1] = comp4(bswap32(m.w[2]));
    r.w[2] = comp4(bswap32(m.w[1])); r.w[3] = comp4(bswap32(m.w[0]));
    return r;
}

// The first byte (0 .. 15) at which x and y differ, 16 when they are equal; *y_less = (y's byte < x's byte) there.
FQD_STRAND_HD uint32_t first_diff16(const Chunk& x, const Chunk& y, bool* y_less)
{
    uint32_t at = 16u;
    bool less = false;
    for (int k = 3; k >= 0; --k) {
        const uint32_t d = x.w[k] ^ y.w[k];
        if (d) {
            const uint32_t sh = uint32_t(__builtin_ctz(d)) & ~7u;
            at = 4u * uint32_t(k) + (sh >> 3);
            less = ((y.w[k] >> sh) & 0xFFu) < ((x.w[k] >> sh) & 0xFFu);
        }
    }
    *y_less = less;
    return at;
}

// ---- a record under sixteen lanes (csrc/fqd_strand.hip; tests/native/strand_check.cpp plays the lanes one after another) --
// A record is decided in rounds; in a round lane gl (0 .. 15) looks at chunk c0 + gl.  The lowest lane of the first round
// in which any lane sees a difference decides; no difference in any round: not flipped (single-end), the shorter mate
// first (pairs).  Every load lies inside the read(s).

FQD_STRAND_HD Chunk load16(const uint8_t* p) { Chunk c; __builtin_memcpy(&c, p, 16); return c; }
FQD_STRAND_HD void store16(uint8_t* p, const Chunk& c) { __builtin_memcpy(p, &c, 16); }

// Chunks to look at (rounds = chunks over sixteen, rounded up).  Single-end: reads under 32 bytes take ONE round with one
// byte a lane (half(L) <= 16); longer ones the chunks that cover positions below half(L), for which q + 16 <= L holds.
FQD_STRAND_HD uint32_t se_chunks(uint32_t L) { return L == 0 ? 0u : L < 32u ? 1u : (half(L) + 15u) >> 4; }
// Pairs, m = the shorter length: under 16 bytes one round with one byte a lane; else m/16 chunks and, when m is no
// multiple of 16, the last sixteen bytes once more from m-16 on (they only add bytes already seen equal by a lower lane).
FQD_STRAND_HD uint32_t pe_chunks(uint32_t m) { return m == 0 ? 0u : m < 16u ? 1u : (m >> 4) + ((m & 15u) ? 1u : 0u); }

// Lane gl's look at round c0 of a single-end read: does it see a difference, and is rc(s) the smaller one there?
FQD_STRAND_HD bool se_lane_sees(const uint8_t* s, uint32_t L, uint32_t c0, uint32_t gl, bool* rc_less)
{
    *rc_less = false;
    if (L < 32u) {
        if (c0 != 0 || gl >= half(L)) return false;
        const uint8_t x = s[gl], y = comp(s[L - 1u - gl]);
        *rc_less = y < x;
        return x != y;
    }
    const uint32_t c = c0 + gl;
    if (c >= se_chunks(L)) return false;
    const uint32_t q = 16u * c;
    return first_diff16(load16(s + q), rc16(load16(s + (L - 16u - q))), rc_less) < 16u;
}

// The same for a pair: is b the smaller one where lane gl sees a and b differ?
FQD_STRAND_HD bool pe_lane_sees(const uint8_t* a, const uint8_t* b, uint32_t m, uint32_t c0, uint32_t gl, bool* b_less)
{
    *b_less = false;
    if (m < 16u) {
        if (c0 != 0 || gl >= m) return false;
        *b_less = b[gl] < a[gl];
        return a[gl] != b[gl];
    }
    const uint32_t c = c0 + gl, full = m >> 4;
    if (c >= pe_chunks(m)) return false;
    const uint32_t q = c < full ? 16u * c : m - 16u;
    return first_diff16(load16(a + q), load16(b + q), b_less) < 16u;
}

// Lane gl's share of dst[0 .. L) = src[0 .. L), or rc(src) when `turn`.  Chunk c of the output is bytes [16c, 16c+16); the
// last sixteen bytes of a length that is no multiple of sixteen are stored once more from L-16 on (same bytes, same
// place) by the lane whose turn the next chunk would have been; under 16 bytes one byte a lane.  Every load lies in
// src[0 .. L), every store in dst[0 .. L).
FQD_STRAND_HD void copy_lane(const uint8_t* src, uint8_t* dst, uint32_t L, bool turn, uint32_t gl)
{
    if (L < 16u) {
        if (gl < L) dst[gl] = turn ? comp(src[L - 1u - gl]) : src[gl];
        return;
    }
    const uint32_t full = L >> 4, chunks = full + ((L & 15u) ? 1u : 0u);
    for (uint32_t c = gl; c < chunks; c += 16u) {
        const uint32_t q = c < full ? 16u * c : L - 16u;
        store16(dst + q, turn ? rc16(load16(src + (L - 16u - q))) : load16(src + q));
    }
}

// ---- the rule read by read (what the kernel's chunks must agree with; also the host's way to state it) ----------------

// flipped(s): looks at positions below half(L) only.
FQD_STRAND_HD bool se_flipped(const uint8_t* s, uint32_t L)
{
    for (uint32_t i = 0; i < half(L); ++i) {
        const uint8_t r = comp(s[L - 1u - i]);
        if (r != s[i]) return r < s[i];
    }
    return false;
}

// out[0 .. L) = canon(s); returns flipped(s).  out must not overlap s.
FQD_STRAND_HD bool se_canon(const uint8_t* s, uint32_t L, uint8_t* out)
{
    const bool flip = se_flipped(s, L);
    for (uint32_t i = 0; i < L; ++i) out[i] = flip ? comp(s[L - 1u - i]) : s[i];
    return flip;
}

// flipped(a, b) = b < a: bytewise over the shorter length, the shorter read first on a tie.
FQD_STRAND_HD bool pe_flipped(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb)
{
    const uint32_t m = la < lb ? la : lb;
    for (uint32_t i = 0; i < m; ++i)
        if (a[i] != b[i]) return b[i] < a[i];
    return lb < la;
}

} // namespace fqdstrand
