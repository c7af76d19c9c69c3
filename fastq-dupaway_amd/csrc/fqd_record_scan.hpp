// fqd_record_scan.hpp — the three-launch scan of the HIP units: kOffTile elements a block for the tiles' sums, ONE block
// over the tile sums (scan_tiles_kernel, the only one-block scan of the library), kOffTile elements a block again for every
// element's start — the scan of fqd_output_plan.  Here with it: where every record's packed bytes start, over the
// descriptors of one or two mates (record_bytes_kernel + scan_tiles_kernel + record_offsets_kernel, fqd_strand.hip and
// fqd_umi.hip; a record's bytes are len0 (+ len1 for S = 2), and a mate that adds one fixed length to every record is a
// uniform Mate), and the places of the set flags of a byte array (head_write_kernel, behind a unit's own count of them).
// The reductions and placements inside a block are fqd_wave.hpp's block_total and block_exclusive.
// Internal to the library's HIP units; every kernel has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fqd_wave.hpp"

namespace fqdscan {
namespace {

constexpr int kBlock = 256;
constexpr int kOffTile = kBlock * 8;                         // records a block of the scan's two passes

struct Mate { const uint8_t* bases; const uint64_t* offsets; const uint32_t* lengths; uint32_t ulen, ustride; };

__device__ __forceinline__ uint64_t mate_off(const Mate& m, uint64_t i) { return m.offsets ? m.offsets[i] : i * uint64_t(m.ustride); }
__device__ __forceinline__ uint32_t mate_len(const Mate& m, uint64_t i) { return m.lengths ? m.lengths[i] : m.ulen; }

// A record's bytes.
template <int S>
__device__ __forceinline__ uint64_t record_len(const Mate& m0, const Mate& m1, uint64_t k)
{
    return uint64_t(mate_len(m0, k)) + (S == 2 ? mate_len(m1, k) : 0u);
}

template <int S>
__global__ __launch_bounds__(kBlock)
void record_bytes_kernel(Mate m0, Mate m1, uint64_t n, unsigned long long* __restrict__ tile_sum)
{
    __shared__ unsigned long long ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    unsigned long long s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const uint64_t k = base + uint32_t(e); if (k < n) s += record_len<S>(m0, m1, k); }
    s = fqdwave::block_total<4>(s, ws);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = s;
}

// The exclusive scan of data[0 .. n) in place by ONE block of 1024; every thread gets the sum back.  It brings its own LDS
// (16 words of T, a copy per kernel that calls it): scan_tiles_kernel and fqd_join.hip's radix_rowscan_kernel.
template <typename T>
__device__ __forceinline__ T scan_in_place(T* __restrict__ data, uint32_t n)
{
    __shared__ T ws[16];
    T carry = 0;                                             // (the same in every thread)
    for (uint32_t t0 = 0; t0 < n; t0 += 1024u) {
        const uint32_t i = t0 + threadIdx.x;
        T total;
        const T before = fqdwave::block_exclusive<16, T>(i < n ? data[i] : T(0), ws, total);
        if (i < n) data[i] = carry + before;
        carry += total;
    }
    return carry;
}

// (the scan of fqd_output_plan: the tile sums, 32 or 64 bits wide, become the tiles' starts; *total = the sum)
template <typename T>
__global__ __launch_bounds__(1024)
void scan_tiles_kernel(T* __restrict__ data, uint32_t n, unsigned long long* __restrict__ total)
{
    const T sum = scan_in_place(data, n);
    if (threadIdx.x == 0) *total = sum;
}

template <int S>
__global__ __launch_bounds__(kBlock)
void record_offsets_kernel(Mate m0, Mate m1, uint64_t n, const unsigned long long* __restrict__ tile_start,
                           unsigned long long* __restrict__ rec_off)
{
    __shared__ unsigned long long ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    uint64_t L[8];
    unsigned long long s = 0, total;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const uint64_t k = base + uint32_t(e); L[e] = k < n ? record_len<S>(m0, m1, k) : 0u; s += L[e]; }
    unsigned long long at = tile_start[blockIdx.x] + fqdwave::block_exclusive<4>(s, ws, total);
#pragma unroll
    for (int e = 0; e < 8; ++e) { const uint64_t k = base + uint32_t(e); if (k < n) { rec_off[k] = at; at += L[e]; } }
}

// Compaction of byte flags by the same scan (a count of the flags a tile into tile_start, scan_tiles_kernel, then this):
// head_place[j] = the place of the j-th set flag of head[0 .. n), for j < m.  Launched by fqd_clusters.hpp's write_heads;
// the other units that include this header do not launch it, hence [[maybe_unused]].
[[maybe_unused]] __global__ __launch_bounds__(kBlock)
void head_write_kernel(const uint8_t* __restrict__ head, uint64_t n, uint64_t m, const unsigned long long* __restrict__ tile_start,
                       uint32_t* __restrict__ head_place)
{
    __shared__ uint32_t ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    bool is_head[8];
    uint32_t s = 0, total;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const uint64_t k = base + uint32_t(e); is_head[e] = k < n && head[k] != 0; s += is_head[e]; }
    unsigned long long at = tile_start[blockIdx.x] + fqdwave::block_exclusive<4>(s, ws, total);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (is_head[e] && at < m) head_place[at] = uint32_t(base + uint32_t(e));
        at += is_head[e];
    }
}

} // namespace
} // namespace fqdscan
