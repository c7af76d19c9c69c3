// fqd_clusters.hpp — the walk over the clusters of (perm, head) that starts a `--fast` unit's work, once: the places where
// an item starts counted a tile and compacted (heads), every cluster's size taken as the distance to the next head and the
// cluster put on the list of its size class (classes).  The words of it — a list's entry and room, the refusal word — are
// fqd_clusters_core.hpp's.  The kernels stay the units' own (head_count_kernel, check_heads_kernel, node_count_kernel,
// classify_kernel): each holds what only its unit checks and counts, around the functions in here.
//
// An entry point then reads: reserve (TileScratch::reserve, fqd_internal.hpp), count (count_heads around the unit's
// counting kernel), refuse, carve (take_lists among the unit's own pieces), write heads (write_heads), classify.
//
// Not in here: fqd_consensus.hip's append to its lists.  Its classify_kernel stages a block's clusters in LDS and takes a
// list's places with one global atomic a block; list_append's one atomic a wave on a list's counter is what that kernel
// waited for (3.43 ms).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fqd_clusters_core.hpp"
#include "fqd_internal.hpp"
#include "fqd_record_scan.hpp"

namespace fqdclusters {
namespace {

using fqdscan::kBlock;
using fqdscan::kOffTile;

// ---- device ------------------------------------------------------------------------------------------------------------------

// A block of kWaves waves counts the places of its tile of kOffTile that start an item, 8 neighbouring places a thread, into
// tile_sum[blockIdx.x].  starts(k) is asked for every place k < n of the tile, in order, and says whether k starts one; what
// else the unit holds against place k it counts in locals of its own that the callable captures, and reduces behind the call.
// Every thread of the block reaches the call.
template <int kWaves, class Starts>
__device__ __forceinline__ void tile_count(uint64_t n, unsigned long long* __restrict__ tile_sum, Starts starts)
{
    __shared__ unsigned long long ws[kWaves];
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    unsigned long long s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint64_t k = base + uint32_t(e);
        if (k < n) s += starts(k) ? 1u : 0u;
    }
    s = fqdwave::block_total<kWaves>(s, ws);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = s;
}

// Cluster c of m: its first place and its members.
__device__ __forceinline__ uint32_t cluster_at(const uint32_t* __restrict__ head_place, uint64_t m, uint64_t n, uint64_t c, uint32_t* k0)
{
    *k0 = head_place[c];
    return uint32_t((c + 1 < m ? uint64_t(head_place[c + 1]) : n) - *k0);
}

template <uint32_t N>
struct Lists { unsigned long long* of[N]; };                 // entries: fqd_clusters_core.hpp's

// A lane's cluster (first place k0, s members) of class cls goes on lists.of[cls]; cls >= N: on none.  A wave adds to a list
// with one atomic on listed[cls].  All 64 lanes reach the call (ballot_append).
template <uint32_t N>
__device__ __forceinline__ void list_append(const Lists<N>& lists, uint32_t* listed, uint32_t cls, uint32_t k0, uint32_t s)
{
#pragma unroll
    for (uint32_t t = 0; t < N; ++t) {
        const uint32_t at = fqdwave::ballot_append(cls == t, &listed[t]);
        if (cls == t) lists.of[t][at] = entry(k0, s);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------

inline uint32_t tiles_of(uint64_t n) { return uint32_t((n + kOffTile - 1) / kOffTile); }

// List t holds the clusters of more than bounds[t] members among n places.
template <uint32_t N>
void take_lists(Carver& c, uint64_t n, const uint32_t (&bounds)[N], Lists<N>& lists)
{
    for (uint32_t t = 0; t < N; ++t) lists.of[t] = c.take<unsigned long long>(list_room(n, bounds[t]));
}

// The heads phase up to the count: count(grid, block) launches the unit's counting kernel over t.tile_sum and t.counters, the
// tile sums are scanned in place, and the number of items m and the counters come back.  *fits: 0 < m <= n; what else refuses
// the call is in got, and the message is the caller's.  Returns what an entry point returns.
template <class C, class Count>
int count_heads(fqd_engine* e, hipStream_t stream, const TileScratch<C>& t, uint64_t n, Count count, unsigned long long* m, C* got, bool* fits)
{
    count(dim3(t.tiles), dim3(kBlock));
    hipLaunchKernelGGL(fqdscan::scan_tiles_kernel<unsigned long long>, dim3(1), dim3(1024), 0, stream, t.tile_sum, t.tiles, t.total);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, hipMemcpyAsync(m, t.total, sizeof *m, hipMemcpyDeviceToHost, stream));
    FQD_TRY(e, read_back(*got, t.counters, stream));
    *fits = *m != 0 && *m <= n;
    return FQD_OK;
}

// Behind count_heads: head_place[j] = the place of the j-th set flag of head[0 .. n), j < m.
template <class C>
void write_heads(hipStream_t stream, const TileScratch<C>& t, const uint8_t* head, uint64_t n, uint64_t m, uint32_t* head_place)
{
    hipLaunchKernelGGL(fqdscan::head_write_kernel, dim3(t.tiles), dim3(kBlock), 0, stream, head, n, m, static_cast<const unsigned long long*>(t.tile_sum), head_place);
}

} // namespace
} // namespace fqdclusters
