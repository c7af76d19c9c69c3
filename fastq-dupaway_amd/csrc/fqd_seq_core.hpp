// fqd_seq_core.hpp — the comparator rules of the sequence-based modes (`--compare-seq tight|loose|tail-hamming`), shared by
// the device heads (csrc/fqd_seq.hip) and host checks (a CPU harness of the tests builds this header with g++).
//
// A read is its sequence bytes WITHOUT the '\n' (len = seq_len - 1 of the reference's views).  The reference compares
// the sequence line including its '\n' (comparator.cpp:45-91); with no byte below '\n' in a sequence (the device sort
// refuses such bytes) the rules below say the same thing:
//   tight        same length and same bytes                                (comparator.cpp:45-58)
//   loose        the shorter is a prefix of the longer: strncmp over min(len) (comparator.cpp:60-74); for pairs both
//                mates, and both overlaps same-sided (comparator.cpp:73)
//   tail-hamming same length, at most `distance` differing bytes         (comparator.cpp:76-91, seq_utils.cpp:65-72)
// The reference walks the records in sorted order with one current reference (seq_dup_remover.hpp:54-109,131-218): a
// record that does not match it is written and becomes the reference; a match is a duplicate, and in loose mode a
// match at least as long (both mates) becomes the reference without being written (hpp:93-98,194-202).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FQD_SEQ_HD __host__ __device__ __forceinline__
#else
#define FQD_SEQ_HD inline
#endif

namespace fqdseq {

enum Mode : int { kTight = 0, kLoose = 1, kHamming = 2 };   // = FQD_SEQ_TIGHT / _LOOSE / _HAMMING of fqdupaway.h

struct View { const uint8_t* p; uint32_t len; };         // one mate: sequence bytes, no '\n'

FQD_SEQ_HD bool same_bytes(const uint8_t* a, const uint8_t* b, uint32_t n)
{
    uint32_t k = 0;
    for (; k + 8u <= n; k += 8u) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + k, 8); __builtin_memcpy(&y, b + k, 8);
        if (x != y) return false;
    }
    for (; k < n; ++k) if (a[k] != b[k]) return false;
    return true;
}

// Number of differing bytes of a and b over n, counted up to `cap + 1` (enough to tell "more than cap").
FQD_SEQ_HD uint32_t mismatches(const uint8_t* a, const uint8_t* b, uint32_t n, uint32_t cap)
{
    uint32_t d = 0, k = 0;
    for (; k + 8u <= n && d <= cap; k += 8u) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + k, 8); __builtin_memcpy(&y, b + k, 8);
        uint64_t z = x ^ y;
        z |= z >> 4; z |= z >> 2; z |= z >> 1;              // bit 0 of every byte = that byte differs
        d += uint32_t(__builtin_popcountll(z & 0x0101010101010101ull));
    }
    for (; k < n && d <= cap; ++k) d += a[k] != b[k];
    return d;
}

FQD_SEQ_HD bool tight_match(View r, View x) { return r.len == x.len && same_bytes(r.p, x.p, r.len); }
FQD_SEQ_HD bool loose_match(View r, View x) { return same_bytes(r.p, x.p, r.len < x.len ? r.len : x.len); }
FQD_SEQ_HD bool hamming_match(View r, View x, uint32_t d) { return r.len == x.len && mismatches(r.p, x.p, r.len, d) <= d; }

// Does record x (mates x1, x2) match the reference r?  paired = false: the second mates are ignored.
FQD_SEQ_HD bool matches(int mode, uint32_t d, bool paired, View r1, View r2, View x1, View x2)
{
    if (mode == kTight) return tight_match(r1, x1) && (!paired || tight_match(r2, x2));
    if (mode == kLoose) {
        if (!loose_match(r1, x1)) return false;
        if (!paired) return true;
        if (!loose_match(r2, x2)) return false;
        return (r1.len <= x1.len && r2.len <= x2.len) || (r1.len > x1.len && r2.len > x2.len);
    }
    return hamming_match(r1, x1, d) && (!paired || hamming_match(r2, x2, d));
}

// Loose mode: a matching record becomes the reference when it is at least as long (both mates).
FQD_SEQ_HD bool loose_takes_over(bool paired, View r1, View r2, View x1, View x2)
{
    return r1.len <= x1.len && (!paired || r2.len <= x2.len);
}

// ---- the parallel head rules (sorted order; record k-1 precedes record k) -------------------------------------------
//
// tight: k is a head iff it does not match k-1.  The reference is the head of k-1's cluster, and every member of a
//   tight cluster is equal to its head.
//
// loose: k is a head iff it does not match k-1 — the current reference when k is compared is ALWAYS record k-1.
//   Proof, by induction over k.  After record k-1 has been compared with the reference r: either it did not match
//   (it is written and becomes the reference), or it matched and was at least as long as r in every mate (it becomes
//   the reference), or it matched and is SHORTER than r in some mate.  The last case cannot happen in sorted order.
//   SE: x = k-1 matches r and is shorter, so x is a proper prefix of r; then x + '\n' < r + '\n' because '\n' is
//   below every byte of r at that place (no sequence byte is below '\n': the sort refuses them), so x sorts before
//   r — but r precedes x.  PE: a match is same-sided, so "not at least as long in every mate" means shorter in BOTH
//   mates; mate 1 of x is then a proper prefix of mate 1 of r and the pair x sorts before the pair r by its first
//   mate, again against the order.  (Two empty mates are equal and as long: the "at least as long" case.)
//
// tail-hamming: the reference is the cluster's head h, and k-1 is either h or within `d` of it, with h's lengths.
//   So k is CERTAINLY a head if a mate's length differs from k-1's (h has k-1's lengths), or if a mate differs from
//   k-1's in more than 2d places (triangle inequality: ham(h,k) >= ham(k-1,k) - ham(h,k-1) > 2d - d).  These
//   certain heads cut the order into segments that are independent; inside a segment the scan from its first
//   record (a head) is run as the reference runs it.
FQD_SEQ_HD bool hamming_certain_head(uint32_t d, bool paired, View p1, View p2, View x1, View x2)
{
    const uint32_t two_d = d > 0x7FFFFFFFu ? 0xFFFFFFFFu : 2u * d;
    if (p1.len != x1.len || mismatches(p1.p, x1.p, x1.len, two_d) > two_d) return true;
    if (!paired) return false;
    return p2.len != x2.len || mismatches(p2.p, x2.p, x2.len, two_d) > two_d;
}

// The reference's scan over records 0..n-1 in sorted order, as written (seq_dup_remover.hpp:54-109,131-218):
// head[k] = 1 iff record k is written.  `at(k, x1, x2)` yields the mates of record k.  Returns the number of heads.
template <class At>
uint64_t sequential_heads(int mode, uint32_t d, bool paired, uint64_t n, At at, uint8_t* head)
{
    if (n == 0) return 0;
    View r1, r2, x1, x2;
    at(0, r1, r2);
    head[0] = 1;
    uint64_t heads = 1;
    for (uint64_t k = 1; k < n; ++k) {
        at(k, x1, x2);
        if (!matches(mode, d, paired, r1, r2, x1, x2)) { head[k] = 1; ++heads; r1 = x1; r2 = x2; }
        else {
            head[k] = 0;
            if (mode == kLoose && loose_takes_over(paired, r1, r2, x1, x2)) { r1 = x1; r2 = x2; }
        }
    }
    return heads;
}

} // namespace fqdseq
