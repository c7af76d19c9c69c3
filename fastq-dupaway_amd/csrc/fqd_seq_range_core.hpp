// fqd_seq_range_core.hpp — the rules of the RANGED run of the sequence-based modes (`--compare-seq` on inputs larger than
// HBM): the prefix key, the exact plan of the ranges and what the comparator carries over a cut.  Shared by the device
// code (csrc/fqd_seq.hip), the host run (host/run_sequence.cpp) and a CPU harness of the tests
// (tests/native/seq_range_check.cpp builds this header with g++).
//
// ---- the prefix key ---------------------------------------------------------------------------------------------------
// key = the first 8 bytes of (sequence + '\n' + '\n' + ...) as a big-endian uint64.  The sort order is that of the
// terminated strings sequence + '\n' (fqd_seq_core.hpp, FastqView::cmp) and no accepted sequence byte is below '\n' (and
// none IS '\n'), so for two records a <= b in that order key(a) <= key(b): the terminated strings differ first at some
// place p, a's byte there being the smaller; for p < 8 that is where the keys differ too (behind a's '\n' the key holds
// '\n', below or equal to every byte), for p >= 8 the keys are equal.  Equal sequences have equal keys.  Pairs are
// ordered by mate 1 first, so mate 1's key is monotone in the pairs' order as well.  Hence: the records of a set of key
// values [lo, hi] are CONTIGUOUS in the sorted order, and sorting every range on its own (stable, input order kept
// inside the range) and writing the ranges in key order gives the sorted order of the whole input, ties included.
//
// ---- the plan ------------------------------------------------------------------------------------------------------------
// Over the pairs sorted by key, with prefix(i) = bytes of the pairs before sorted place i: a range starts where the last
// one ended (a place where the key changes) and ends at the LAST key change e with prefix(e) - prefix(start) <= target;
// when even the first key value does not fit it ends behind that key value (one oversized key value is a range of its
// own).  next_cut() below is that rule; it is all the device and the harness run.
//
// ---- what is carried over a cut (the phantom) --------------------------------------------------------------------------
// The reference's scan (seq_dup_remover.hpp:54-218) walks the whole sorted order with ONE current reference record.
// Range r+1 is scanned on its own, so it has to start with the reference the scan holds when it leaves range r:
//
//   tight         nothing.  A record matches the reference only when it is EQUAL to it; equal records have equal keys
//                 and a key value is never cut.  The first record of range r+1 has a key above every key of range r, so
//                 it differs from the reference whatever that is, is written and becomes the reference: exactly what a
//                 scan that starts there does.  Pairs: equal pairs have equal first mates, the same argument.
//
//   loose         the LAST record of range r in sorted order, whether it was written or not.  fqd_seq_core.hpp proves
//                 that the reference, when record k is compared, is always record k-1 of the sorted order (SE and PE).
//                 The sorted order of the input is the ranges' sorted orders one after the other (above), so record k-1
//                 of the first record of range r+1 is the last sorted record of range r.  One record (pair) is enough:
//                 the proof needs no older state.  Such a cluster does straddle cuts: ACGT is a prefix of ACGTAAAAA
//                 and their keys differ.
//
//   tail-hamming  the LAST HEAD of range r in sorted order (the carried record itself when range r wrote nothing).  The
//                 reference is the current cluster's head and changes only when a record does not match it; members
//                 leave no trace.  Two reads within d may differ inside the first 8 bytes, so a cluster straddles cuts
//                 too.  For pairs the head is the pair; mate 1 alone decides the range, mate 2 only the match.
//
// The carried record (pair) is put in front of range r+1's store with its whole text, as record 0: the PHANTOM.  Its key
// is below the range's lowest key (it belongs to an earlier range), so it is strictly below every record of the range in
// the sort order and fqd_sort_seqs puts it first; the order of the others is untouched.  fqd_seq_heads then does what it
// always does: position 0 is a head and the reference of what follows — for tight / loose as record k-1 of position 1,
// for tail-hamming as the head of the first segment (position 0 is a certain head, and the certain-head test of position
// 1 against it is sound because position 0 IS the head).  Afterwards the phantom's head flag is cleared: it was written,
// listed and counted where it belongs, in its own range.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FQD_RANGE_HD __host__ __device__ __forceinline__
#else
#define FQD_RANGE_HD inline
#endif

namespace fqdseq {

constexpr uint32_t kKeyBytes = 8;

FQD_RANGE_HD uint64_t prefix_key(const uint8_t* seq, uint32_t len)
{
    uint64_t k = 0;
    for (uint32_t j = 0; j < kKeyBytes; ++j) k = (k << 8) | (j < len ? seq[j] : uint8_t('\n'));
    return k;
}

// Is some byte of the 8 in x below '\n'?  (exact: x - 0x0A.. borrows into bit 7 of a byte whose own bit 7 is clear only
// when that byte, or a lower one that borrowed, was below 0x0A; the lowest such byte is always found)
FQD_RANGE_HD bool word_has_byte_below_newline(uint64_t x)
{
    return ((x - 0x0A0A0A0A0A0A0A0Aull) & ~x & 0x8080808080808080ull) != 0;
}

// The first sorted place in [lo, hi) whose key is >= k (not_below) / > k (above).  key(i): the key at sorted place i.
template <class KeyAt>
FQD_RANGE_HD uint64_t first_not_below(uint64_t lo, uint64_t hi, uint64_t k, KeyAt key)
{
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (key(mid) < k) lo = mid + 1; else hi = mid; }
    return lo;
}
template <class KeyAt>
FQD_RANGE_HD uint64_t first_above(uint64_t lo, uint64_t hi, uint64_t k, KeyAt key)
{
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (key(mid) <= k) lo = mid + 1; else hi = mid; }
    return lo;
}

// The range that starts at sorted place `start` (< n, a place where the key changes) ends before the place returned.
// key(i) for i < n; prefix(i) for i <= n = bytes of the pairs before place i (64 bits, non-decreasing, prefix(n) = all).
template <class KeyAt, class PrefixAt>
FQD_RANGE_HD uint64_t next_cut(uint64_t start, uint64_t n, uint64_t target, KeyAt key, PrefixAt prefix)
{
    const uint64_t base = prefix(start);
    uint64_t lo = start, hi = n;                            // p = the last place with prefix(p) - base <= target
    while (lo < hi) { const uint64_t mid = lo + (hi - lo + 1) / 2; if (prefix(mid) - base <= target) lo = mid; else hi = mid - 1; }
    if (lo == n) return n;                                  // everything that is left fits
    const uint64_t e = first_not_below(start, lo + 1, key(lo), key);    // the pair at place p does not fit: back to where its key starts
    if (e > start) return e;
    return first_above(start, n, key(start), key);          // the first key value alone is beyond the target: it stands alone
}

// The range of a key: how many ranges end below it.  hi(r) = the largest key of range r (ascending).
template <class HiAt>
FQD_RANGE_HD uint32_t range_of_key(uint64_t k, uint32_t n_ranges, HiAt hi)
{
    uint32_t lo = 0, up = n_ranges;
    while (lo < up) { const uint32_t mid = lo + (up - lo) / 2; if (hi(mid) < k) lo = mid + 1; else up = mid; }
    return lo;
}

// The words of the refusal of a sequence byte below '\n' (the census of fqd_sort_seqs and pass A of the ranged run).
#define FQD_SEQ_LOW_BYTE_FORMAT "a sequence line holds the byte %u (NUL or a control byte below '\\n'), which the " \
                                "sequence-based modes of this build do not support"

} // namespace fqdseq
