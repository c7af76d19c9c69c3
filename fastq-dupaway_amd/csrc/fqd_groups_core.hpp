// fqd_groups_core.hpp — the ends of a group of equal keys in a SORTED key array, for the seed joins of the `--fast` mode
// (csrc/fqd_near.hip, csrc/fqd_prefix.hip): a lane that stands on entry e finds where e's group ends and where it begins
// without a scan over the group.  Plain functions, host and device; the CPU harness of the prefix rule
// (tests/native/prefix_check.cpp) plays them against a linear scan.
#pragma once
#include <cstdint>

#include "fqd_seq_core.hpp"

namespace fqdgroups {

// The first place behind e whose key is not keys[e] (N where there is none): a gallop, then a binary search.
FQD_SEQ_HD uint64_t group_end(const uint64_t* __restrict__ keys, uint64_t N, uint64_t e)
{
    const uint64_t key = keys[e];
    uint64_t lo = e, step = 1;                               // keys[lo] == key
    while (lo + step < N && keys[lo + step] == key) { lo += step; step <<= 1; }
    uint64_t hi = lo + step < N ? lo + step : N;             // keys[hi] != key, or hi == N
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] == key) lo = mid; else hi = mid;
    }
    return hi;
}

// The first place of e's group.
FQD_SEQ_HD uint64_t group_start(const uint64_t* __restrict__ keys, uint64_t e)
{
    const uint64_t key = keys[e];
    uint64_t hi = e, step = 1;                               // keys[hi] == key
    while (hi >= step && keys[hi - step] == key) { hi -= step; step <<= 1; }
    uint64_t lo = hi >= step ? hi - step : 0;                // keys[lo] != key, or lo == 0
    if (keys[lo] == key) return lo;                          // (lo == 0)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] == key) hi = mid; else lo = mid;
    }
    return hi;
}

} // namespace fqdgroups
