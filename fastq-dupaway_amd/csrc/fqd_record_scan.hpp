// fqd_record_scan.hpp — where every record's packed bytes start: the three-step scan over the descriptors of one or two
// mates that fqd_strand.hip and fqd_umi.hip share (record_bytes_kernel + u64_scan_kernel + record_offsets_kernel: kOffTile
// records a block, one block over the block sums, kOffTile records a block again — the scan of fqd_output_plan).  A
// record's bytes are len0 (+ len1 for S = 2); a mate that adds one fixed length to every record is a uniform Mate.
// Internal to the library's HIP units; every kernel has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fqdscan {
namespace {

constexpr int kBlock = 256;
constexpr int kOffTile = kBlock * 8;                         // records a block of the scan's two passes

struct Mate { const uint8_t* bases; const uint64_t* offsets; const uint32_t* lengths; uint32_t ulen, ustride; };

__device__ __forceinline__ uint64_t mate_off(const Mate& m, uint64_t i) { return m.offsets ? m.offsets[i] : i * uint64_t(m.ustride); }
__device__ __forceinline__ uint32_t mate_len(const Mate& m, uint64_t i) { return m.lengths ? m.lengths[i] : m.ulen; }

template <int S>
__global__ __launch_bounds__(kBlock)
void record_bytes_kernel(Mate m0, Mate m1, uint64_t n, unsigned long long* __restrict__ tile_sum)
{
    __shared__ unsigned long long ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    unsigned long long s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint64_t k = base + uint32_t(e);
        if (k < n) s += uint64_t(mate_len(m0, k)) + (S == 2 ? mate_len(m1, k) : 0u);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// (the scan of fqd_output_plan: exclusive, in place, by one block; *total = the sum)
__global__ __launch_bounds__(1024)
void u64_scan_kernel(unsigned long long* __restrict__ data, uint32_t n, unsigned long long* __restrict__ total)
{
    __shared__ unsigned long long wt[16];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t t0 = 0; t0 < n; t0 += 1024u) {
        const uint32_t i = t0 + threadIdx.x;
        const unsigned long long v = i < n ? data[i] : 0ull;
        unsigned long long inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const unsigned long long up = __shfl_up(inc, d, 64); if (int(lane) >= d) inc += up; }
        if (lane == 63u) wt[wave] = inc;
        __syncthreads();
        unsigned long long before = carry;
        for (uint32_t w = 0; w < wave; ++w) before += wt[w];
        if (i < n) data[i] = before + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023u) carry = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

template <int S>
__global__ __launch_bounds__(kBlock)
void record_offsets_kernel(Mate m0, Mate m1, uint64_t n, const unsigned long long* __restrict__ tile_start,
                           unsigned long long* __restrict__ rec_off)
{
    __shared__ unsigned long long ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    uint64_t L[8];
    unsigned long long s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint64_t k = base + uint32_t(e);
        L[e] = k < n ? uint64_t(mate_len(m0, k)) + (S == 2 ? mate_len(m1, k) : 0u) : 0u;
        s += L[e];
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long up = __shfl_up(inc, d, 64); if (int(lane) >= d) inc += up; }
    if (lane == 63u) ws[wave] = inc;
    __syncthreads();
    unsigned long long at = tile_start[blockIdx.x] + inc - s;
    for (uint32_t w = 0; w < wave; ++w) at += ws[w];
#pragma unroll
    for (int e = 0; e < 8; ++e) { const uint64_t k = base + uint32_t(e); if (k < n) { rec_off[k] = at; at += L[e]; } }
}

} // namespace
} // namespace fqdscan
