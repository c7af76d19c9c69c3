// fqd_wave.hpp — the wave and workgroup idioms of the HIP units, once: reductions across a wave or a group of its lanes, the
// sum scan across a wave and a workgroup, and a wave's append to a list.  Sums, minima, maxima and ors only; a scan over
// another operation (fqd_seq_pick.hip, fqd_size.hip) stays where it is used.  Device-only, every function inlined.
//
// What holds for all of them: a wave is 64 lanes; workgroups are one-dimensional and a multiple of 64 threads, so a
// thread's lane is threadIdx.x & 63 and its wave threadIdx.x >> 6.  EVERY LANE OF THE WAVE (block_*: every thread of the
// workgroup) REACHES THE CALL — a lane with nothing to add passes 0 (or the operation's identity), it does not skip the call:
// the shuffles and ballots read all 64 lanes, and the block_* functions hold barriers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fqdwave {

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint32_t wave_id() { return threadIdx.x >> 6; }

// ---- across a wave: down-shuffles, LANE 0'S RESULT IS THE WAVE'S (the other lanes hold partial ones) -----------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const T o = __shfl_down(v, d, 64); v = o > v ? o : v; }
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const T o = __shfl_down(v, d, 64); v = o < v ? o : v; }
    return v;
}

// ---- across a group of G neighbouring lanes (G a power of two, groups aligned): xor butterflies, EVERY LANE OF THE GROUP
// holds the group's result ---------------------------------------------------------------------------------------------------
template <int G, typename T>
__device__ __forceinline__ T group_sum(T v)
{
#pragma unroll
    for (int d = G / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, G);
    return v;
}

template <int G, typename T>
__device__ __forceinline__ T group_or(T v)
{
#pragma unroll
    for (int d = G / 2; d > 0; d >>= 1) v |= __shfl_xor(v, d, G);
    return v;
}

template <int G, typename T>
__device__ __forceinline__ T group_min(T v)
{
#pragma unroll
    for (int d = G / 2; d > 0; d >>= 1) { const T o = __shfl_xor(v, d, G); v = o < v ? o : v; }
    return v;
}

template <int G, typename T>
__device__ __forceinline__ T group_max(T v)
{
#pragma unroll
    for (int d = G / 2; d > 0; d >>= 1) { const T o = __shfl_xor(v, d, G); v = o > v ? o : v; }
    return v;
}

// ---- sum scans -------------------------------------------------------------------------------------------------------------
// The sum of v over this lane and the lanes below it in its group of G lanes (G = 64: the wave).
template <typename T, int G = 64>
__device__ __forceinline__ T wave_inclusive(T v)
{
    const int l = int(lane_id() % uint32_t(G));
#pragma unroll
    for (int d = 1; d < G; d <<= 1) { const T up = __shfl_up(v, d, G); if (l >= d) v += up; }
    return v;
}

// The workgroup's sum of v (kWaves waves; ws: kWaves words of LDS).  What thread 0 gets back is the sum.  ws is read after
// the barrier in here and by nothing later: another barrier has to stand between this call and the next store to ws.
template <int kWaves, typename T>
__device__ __forceinline__ T block_total(T v, T* ws)
{
    v = wave_sum(v);
    if (lane_id() == 0u) ws[wave_id()] = v;
    __syncthreads();
    T total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += ws[w];
    return total;
}

// The sum of v over the threads below this one in the workgroup (kWaves waves; ws: kWaves words of LDS), and in `total`,
// for every thread, the workgroup's sum.  A barrier ends the call: ws may be stored to again right after it.
template <int kWaves, typename T>
__device__ __forceinline__ T block_exclusive(T v, T* ws, T& total)
{
    const uint32_t wave = wave_id();
    const T inc = wave_inclusive(v);
    if (lane_id() == 63u) ws[wave] = inc;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) { const T c = ws[w]; before += uint32_t(w) < wave ? c : T(0); total += c; }
    __syncthreads();
    return before + inc - v;
}

// ---- a wave appends to a list ----------------------------------------------------------------------------------------------
// The lanes for which `mine` holds take consecutive places, `each` entries apart, behind ONE atomicAdd to *counter (32 or 64
// bits, global memory or LDS) by the first of them; each of them gets its own place back, the others 0 (all of them where the wave has no taker).  All 64 lanes reach
// the call: a kernel that uses it gives every lane an index without a grid stride, and passes mine = false beyond the end.
template <typename T>
__device__ __forceinline__ T ballot_append(bool mine, T* counter, T each = 1)
{
    const unsigned long long takers = __ballot(mine);
    if (!takers) return 0;                                   // (the same for every lane)
    const uint32_t lane = lane_id();
    const int leader = __ffsll(takers) - 1;
    T first = 0;
    if (int(lane) == leader) first = atomicAdd(counter, T(__popcll(takers)) * each);
    first = __shfl(first, leader, 64) + T(__popcll(takers & ((1ull << lane) - 1ull))) * each;
    return mine ? first : T(0);
}

} // namespace fqdwave
