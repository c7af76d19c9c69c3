// fqd_groups.hpp — the pass over a SORTED (key, node) entry list that the seed joins of the `--fast` mode share
// (csrc/fqd_near.hip, csrc/fqd_prefix.hip): the groups of equal keys are counted, the largest is kept, a group beyond the
// unit's limit is offered to the refusal, and the entries that have a later entry in their group go on the work list.
// Device-only; the group ends themselves are fqd_groups_core.hpp's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fqd_groups_core.hpp"
#include "fqd_wave.hpp"

namespace fqdgroups {

// A lane an entry, no stride (the wave's sums): e = the lane's entry, every lane of the wave reaches the call.  work: room for
// N places — the entries that have a later entry in their group, a wave adding to the list with one atomic.  The first entry
// of a group finds the group's end and with it the size.  An entry with an equal key half the limit away on either side —
// every entry of a group beyond the limit has one — finds both ends, and where the group is beyond the limit offers
// (its node << 32 | size) to one 64-bit atomicMin: the lowest first record of such a group, and that group's size.
// C: the unit's counters, with the 64-bit words groups, largest, work and over (over starts as all ones).
template <uint32_t kMaxGroup, class C>
__device__ __forceinline__ void mark_groups(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t N, uint64_t e, uint64_t* __restrict__ work,
                                            C* counters)
{
    const bool live = e < N;
    uint64_t key = 0;
    if (live) key = keys[e];
    const bool first = live && (e == 0 || keys[e - 1] != key);
    unsigned long long size = 0;
    if (first) size = group_end(keys, N, e) - e;
    constexpr uint64_t half = kMaxGroup / 2;
    if (live && ((e >= half && keys[e - half] == key) || (e + half < N && keys[e + half] == key))) {
        const unsigned long long all = group_end(keys, N, e) - group_start(keys, e);
        if (all > kMaxGroup) atomicMin(&counters->over, (static_cast<unsigned long long>(vals[e]) << 32) | (all > 0xFFFFFFFFull ? 0xFFFFFFFFull : all));
    }
    const unsigned long long groups = static_cast<unsigned long long>(__popcll(__ballot(first)));
    const unsigned long long largest = fqdwave::wave_max(size);
    const bool followed = live && e + 1 < N && keys[e + 1] == key;
    const unsigned long long at = fqdwave::ballot_append(followed, &counters->work);
    if (followed && at < N) work[at] = e;
    if ((threadIdx.x & 63) == 0) {
        if (groups) atomicAdd(&counters->groups, groups);
        if (largest) atomicMax(&counters->largest, largest);
    }
}

} // namespace fqdgroups
