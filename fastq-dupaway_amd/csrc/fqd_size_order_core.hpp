// fqd_size_order_core.hpp — the rules of FQD_FAST_SORT=size / FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE: which clusters of the
// `--fast` mode are written at all, and in which order.  Shared by the device code (csrc/fqd_size_order.hip) and a CPU
// harness of the tests (tests/native/size_order_check.cpp builds this header with g++ and the sanitizers).
//
// ---- definitions ------------------------------------------------------------------------------------------------------
// (perm, head)  fqd_size_core.hpp's: an order of the n records and a flag at the first place of every cluster, the clusters
//               in the order of their first member in the input, perm[s] at a head's place s the record that is written.
// size, keep    fqd_cluster_sizes' member count at every written record (0 elsewhere) and the flags of the written records.
// filter        a written record r stays written iff min_size <= size[r] and (max_size = 0 or size[r] <= max_size).
// kept place    a place s with head[s] set and keep[perm[s]] set (a perm[s] outside 0 .. n-1 is no kept place).  W = their
//               number; W <= the number of head places <= n.
// order         the kept places s_0 < s_1 < .. < s_(W-1), sorted STABLY by size[perm[s]] descending; order[k] = perm[s] of
//               the k-th.  So among clusters of one size the one whose first member stands earlier in the input comes first:
//               the order of `<output>.clusters`.
//
// ---- compaction: an exclusive count in three launches (the scan shape of fqd_record_scan.hpp) ---------------------------
// c(s) = 1 at a kept place, 0 elsewhere.  tiles: T(t) = the sum of c over tile t (kOffTile places a block); carry: one block
// scans T exclusively and leaves W; places: at(s) = carry(t) + the sum of c over the tile's places in front of s.  A kept
// place writes entry at(s): the entries 0 .. W-1 are written once each, in place order.  No block waits for another.
//
// ---- two tiers: the work over all W entries does not grow with the largest cluster ------------------------------------------
// An LSD radix sort over the bits of the largest size would send all W entries through one pass per eight bits of it: one
// poly-G cluster of 10^5 reads would cost 80 M singletons two more passes.  Instead:
//   tier 1  ONE stable 8-bit pass over all W entries by digit(size) = 256 - size for size <= 255, 0 above.  Bucket 0 then
//           holds the L entries above 255 members in place order, bucket d = 1 .. 255 the entries of size 256 - d in place
//           order.  The buckets stand in ascending digit: bucket 0, then sizes 255, 254, .., 1.
//   tier 2  the first L entries alone, stably by key = largest - size over the bits of largest - 256 (the largest key:
//           the smallest size in bucket 0 is 256), eight bits a pass, least significant first.
// Proof.  (a) Every entry of bucket 0 has a larger size than every entry behind it, and tier 2 permutes bucket 0 within
// itself only, so the entries 0 .. L-1 and L .. W-1 stand in the right order to each other.  (b) Behind bucket 0, digit
// ascending is size descending, and a stable pass leaves equal digits — equal sizes, digit being one-to-one on 1 .. 255 —
// in the order they came in, the place order.  (c) An LSD radix sort of stable passes is a stable sort by the whole key;
// key ascending is size descending; bucket 0 came in place order (tier 1 is stable), so equal sizes stay in place order.
// A cluster above 255 members holds at least 256 records, so L <= n / 256: tier 2's passes, however many, move at most
// 1/256 of the records each.  fqd_internal_radix_sort (fqd_join.hip) is the stable pass of both tiers.
//
// ---- nothing is written outside order[0 .. n) ---------------------------------------------------------------------------------
// Only kept places produce entries, a kept place is a head place, and there are at most n places: W <= n whatever perm
// holds.  A perm[s] >= n is never used as an index (it is no kept place), so keep and size are read inside 0 .. n-1 only.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FQD_ORDER_HD __host__ __device__ __forceinline__
#else
#define FQD_ORDER_HD inline
#endif

namespace fqdorder {

constexpr uint32_t kSmallMax = 255;                          // the largest size tier 1 tells apart
constexpr uint32_t kMaxSize = 0x7FFFFFFFu;                   // n < 2^31: no cluster has more members

// Does the filter take a cluster of `size` members out?  max_size = 0: no upper bound.
FQD_ORDER_HD bool dropped(uint32_t size, uint32_t min_size, uint32_t max_size)
{
    return size < min_size || (max_size != 0u && size > max_size);
}

// Tier 1's digit: 1 .. 255 for the sizes 255 .. 1, 0 for everything above.  (Size 0 is no cluster's; it is refused before
// the sort and takes the last bucket here, so that the digit has eight bits whatever comes in.)
FQD_ORDER_HD uint32_t tier1_digit(uint32_t size)
{
    if (size > kSmallMax) return 0u;
    return size ? 256u - size : 255u;
}

// What the compaction stores for a kept place: the digit in the low byte, the size in the high word (tier 2 takes its
// key from it once `largest` is known).
FQD_ORDER_HD uint64_t tier1_key(uint32_t size) { return (uint64_t(size) << 32) | tier1_digit(size); }
FQD_ORDER_HD uint32_t key_size(uint64_t key) { return uint32_t(key >> 32); }

// Tier 2's key of an entry of bucket 0 (256 <= size <= largest): ascending key is descending size.
FQD_ORDER_HD uint64_t tier2_key(uint32_t largest, uint32_t size) { return uint64_t(largest - size); }

// The bits of the largest tier-2 key, largest - 256; 0 where bucket 0 is empty or holds one size only.
FQD_ORDER_HD uint32_t tier2_bits(uint32_t largest)
{
    if (largest <= kSmallMax + 1u) return 0u;
    uint32_t span = largest - (kSmallMax + 1u), bits = 0;
    while (span) { ++bits; span >>= 1; }
    return bits;
}

FQD_ORDER_HD uint32_t tier2_passes(uint32_t largest) { return (tier2_bits(largest) + 7u) / 8u; }

} // namespace fqdorder
