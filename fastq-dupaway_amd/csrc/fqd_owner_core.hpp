// fqd_owner_core.hpp — the rules of FQD_FAST_KEEP / FQD_FAST_CLUSTERS: from the `--fast` engine's "an EARLIER record holds
// my key" to "the FIRST record with my key", and the key the records are grouped by.  Shared by the device code
// (csrc/fqd_owner.hip) and a CPU harness of the tests (tests/native/owner_check.cpp builds this header with g++ and the
// sanitizers).
//
// ---- the chain ----------------------------------------------------------------------------------------------------------
// After a run of fqd_submit_linked over records 0 .. n-1 (engine indices, input order):
//   keep[i] = 1  exactly for the first record of every distinct key (the engine's first-occurrence-wins rule);
//   keep[i] = 0  otherwise, and then link[i] = j with j < i and key(j) == key(i).  WHICH such j depends on how the lanes
//                of the insert kernels met; nothing below uses more than "earlier, same key".
// next(i) = i when keep[i], else link[i].  owner(i) = the fixed point of next reached from i.
//   Ends:     next(i) < i whenever keep[i] == 0, so the walk strictly decreases and takes at most i steps.
//   Same key: every step goes to a record of the same key, so the fixed point f has key(f) == key(i) and keep[f] == 1.
//   Unique:   exactly one record of a key has keep == 1, the first one.  So owner(i) = the first record with key(i),
//             whatever the links were: the result is deterministic although the links are not.
// A link that does not decrease (memory that fqd_submit_linked did not write) ends the walk with kBrokenChain instead of
// running on or leaving the arrays: every index the walk reads is below the one it came from.
//
// ---- the grouping key ----------------------------------------------------------------------------------------------------
// Records are grouped by owner with a STABLE sort of (group_key(owner[i]), i) over the low group_bits(n) bits of the key:
// owners are below n, so those bits order them fully; stability keeps the members of an owner in input order; and since
// an owner is its cluster's first member, ascending owners ARE the order of the clusters' first members in the input.
// The owner itself stands first in its run (it is the smallest index of its cluster).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FQD_OWNER_HD __host__ __device__ __forceinline__
#else
#define FQD_OWNER_HD inline
#endif

namespace fqdowner {

constexpr uint32_t kBrokenChain = 0xFFFFFFFFu;

// owner(i); *steps (may be null) = the links followed.
FQD_OWNER_HD uint32_t chain_owner(const uint8_t* keep, const uint32_t* link, uint32_t i, uint32_t* steps)
{
    uint32_t s = 0;
    while (!keep[i]) {
        const uint32_t next = link[i];
        if (next >= i) { i = kBrokenChain; break; }
        i = next;
        ++s;
    }
    if (steps) *steps = s;
    return i;
}

FQD_OWNER_HD uint64_t group_key(uint32_t owner) { return uint64_t(owner); }

// The key bits that tell the owners of n records apart: the bits of n - 1, at least one.
FQD_OWNER_HD uint32_t group_bits(uint64_t n)
{
    uint32_t b = 1;
    while (b < 64u && ((n - 1) >> b) != 0) ++b;
    return n <= 1 ? 1u : b;
}

// Does sorted place k start a run?  (prev = the key at place k - 1)
FQD_OWNER_HD bool group_starts(uint64_t k, uint64_t prev, uint64_t key) { return k == 0 || prev != key; }

} // namespace fqdowner
