// fqd_size_order.hip — FQD_FAST_SORT=size / FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE of the `--fast` mode (same library as
// fqd_engine.hip): the clusters outside the size bounds taken out of the keep flags, the written records in order of
// decreasing cluster size, and the gather that brings per-record arrays into that order.  Rules and proofs:
// fqd_size_order_core.hpp.
//
//   filter   size_filter_kernel: one streaming pass, four records a lane (a 16-byte load of sizes and a 4-byte load of flags
//            where both pointers allow it), the three counters summed wave by wave, then over the block's four waves in LDS:
//            three global atomics a block, none per record.  Only a lane that clears a flag stores.
//   order    the kept head places compacted into (key, record) pairs in place order — order_tiles_kernel (kOffTile places a
//            block, one count a tile), fqd_record_scan.hpp's scan_tiles_kernel (one block over the tile counts, exclusive; its
//            total is W), order_places_kernel (kOffTile places a block again; it also counts the clusters above 255 members
//            and finds the largest) — then tier 1, one pass of fqd_internal_radix_sort over all W pairs by the size's digit,
//            order_rekey_kernel over the L pairs of bucket 0, and tier 2, the passes of largest - 256 over those L alone.
//            fqd_size_order_ex reports W, L, the largest size and tier 2's passes as the call counted and launched them.
//            The host waits twice in between: for W, which sizes the sort's scratch, and for L and the largest size, which
//            decide tier 2's length and passes.
//   take     take_u32_kernel: out[k] = values[idx[k]], a 4-byte gather a lane.
#include <hip/hip_runtime.h>

#include "fqd_internal.hpp"
#include "fqd_record_scan.hpp"
#include "fqd_size_order_core.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kOffTile = fqdscan::kOffTile;                  // places a block of the compaction's two passes

struct FilterCounts { unsigned long long clusters, records, bad; };
struct OrderStats { unsigned long long above, bad; uint32_t largest, reserved; };

using fqdwave::wave_max;
using fqdwave::wave_sum;

// ---- filter ----------------------------------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kBlock)
void size_filter_kernel(const uint32_t* __restrict__ size, uint64_t n, uint32_t min_size, uint32_t max_size, uint8_t* __restrict__ keep,
                        FilterCounts* __restrict__ out)
{
    __shared__ unsigned long long ws[3][4];
    unsigned long long clusters = 0, records = 0, bad = 0;
    const uint64_t quads = (n + 3u) / 4u;
    for (uint64_t q = blockIdx.x * uint64_t(kBlock) + threadIdx.x; q < quads; q += uint64_t(gridDim.x) * kBlock) {
        const uint64_t r0 = q * 4u;
        const bool whole = VEC && r0 + 4u <= n;
        uint32_t sz[4] = {0u, 0u, 0u, 0u};
        uint8_t k[4] = {0, 0, 0, 0};
        if (whole) {
            const uint4 v = *reinterpret_cast<const uint4*>(size + r0);
            const uchar4 f = *reinterpret_cast<const uchar4*>(keep + r0);
            sz[0] = v.x; sz[1] = v.y; sz[2] = v.z; sz[3] = v.w;
            k[0] = f.x; k[1] = f.y; k[2] = f.z; k[3] = f.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (r0 + uint32_t(j) < n) { sz[j] = size[r0 + uint32_t(j)]; k[j] = keep[r0 + uint32_t(j)]; }
        }
        uint32_t cleared = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!k[j]) continue;
            bad += sz[j] == 0u;
            if (fqdorder::dropped(sz[j], min_size, max_size)) { cleared |= 1u << j; ++clusters; records += sz[j]; }
        }
        if (cleared) {
#pragma unroll
            for (int j = 0; j < 4; ++j) if ((cleared >> j) & 1u) keep[r0 + uint32_t(j)] = 0;   // (a cleared flag's record lies below n: its flag was loaded)
        }
    }
    // (three sums behind ONE barrier, a thread an atomic: block_total would be a barrier a sum)
    clusters = wave_sum(clusters); records = wave_sum(records); bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = clusters; ws[1][threadIdx.x >> 6] = records; ws[2][threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned long long v = ws[threadIdx.x][0] + ws[threadIdx.x][1] + ws[threadIdx.x][2] + ws[threadIdx.x][3];
        unsigned long long* to = threadIdx.x == 0 ? &out->clusters : threadIdx.x == 1 ? &out->records : &out->bad;
        if (v) atomicAdd(to, v);
    }
}

// ---- order: compaction -------------------------------------------------------------------------------------------------------

// Is place k a kept place?  r = its record where it is.
__device__ __forceinline__ bool kept_place(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ head, const uint8_t* __restrict__ keep,
                                           uint64_t n, uint64_t k, uint32_t& r)
{
    if (k >= n || !head[k]) return false;
    r = perm[k];
    return r < n && keep[r] != 0;                            // (an order that is no permutation of 0 .. n-1 never reads outside keep[])
}

__global__ __launch_bounds__(kBlock)
void order_tiles_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ head, const uint8_t* __restrict__ keep, uint64_t n,
                        unsigned long long* __restrict__ tile_count)
{
    __shared__ unsigned long long ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    unsigned long long c = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { uint32_t r = 0; c += kept_place(perm, head, keep, n, base + uint32_t(e), r) ? 1u : 0u; }
    c = fqdwave::block_total<4>(c, ws);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = c;
}

__global__ __launch_bounds__(kBlock)
void order_places_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ head, const uint8_t* __restrict__ keep,
                         const uint32_t* __restrict__ size, uint64_t n, const unsigned long long* __restrict__ tile_start,
                         unsigned long long n_pairs, uint64_t* __restrict__ key, uint32_t* __restrict__ val, OrderStats* __restrict__ stats)
{
    __shared__ uint32_t ws[4];
    __shared__ uint32_t s_above, s_bad, s_largest;
    if (threadIdx.x == 0) { s_above = 0; s_bad = 0; s_largest = 0; }
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    uint32_t rec[8];
    uint32_t mask = 0, c = 0, total;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        rec[e] = 0;
        if (kept_place(perm, head, keep, n, base + uint32_t(e), rec[e])) { mask |= 1u << e; ++c; }
    }
    unsigned long long at = tile_start[blockIdx.x] + fqdwave::block_exclusive<4>(c, ws, total);   // (its barriers stand behind thread 0's stores above)
    uint32_t above = 0, bad = 0, largest = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (!((mask >> e) & 1u)) continue;
        const uint32_t sz = size[rec[e]];
        if (at < n_pairs) { key[at] = fqdorder::tier1_key(sz); val[at] = rec[e]; }      // (at < W by the scan; the bound is the allocation's)
        ++at;
        above += sz > fqdorder::kSmallMax;
        bad += sz == 0u;
        largest = sz > largest ? sz : largest;
    }
    above = wave_sum(above); bad = wave_sum(bad); largest = wave_max(largest);
    if ((threadIdx.x & 63) == 0) {
        if (above) atomicAdd(&s_above, above);
        if (bad) atomicAdd(&s_bad, bad);
        if (largest) atomicMax(&s_largest, largest);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_above) atomicAdd(&stats->above, static_cast<unsigned long long>(s_above));
        if (s_bad) atomicAdd(&stats->bad, static_cast<unsigned long long>(s_bad));
        if (s_largest) atomicMax(&stats->largest, s_largest);
    }
}

// Bucket 0 after tier 1: the size in the key's high word becomes tier 2's key.
__global__ __launch_bounds__(kBlock)
void order_rekey_kernel(uint64_t* __restrict__ key, uint64_t n, uint32_t largest)
{
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
        const uint32_t sz = fqdorder::key_size(key[i]);
        key[i] = fqdorder::tier2_key(largest, sz < largest ? sz : largest);
    }
}

// ---- take ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void take_u32_kernel(const uint32_t* __restrict__ values, const uint32_t* __restrict__ idx, uint64_t n, uint32_t* __restrict__ out)
{
    for (uint64_t k = blockIdx.x * uint64_t(kBlock) + threadIdx.x; k < n; k += uint64_t(gridDim.x) * kBlock) out[k] = values[idx[k]];
}

// Is p memory the device can be handed?  Asked of the runtime's bookkeeping: nothing is allocated or touched.
struct CountBuffers { OrderStats* stats; unsigned long long* total; unsigned long long* tile; };

size_t carve_counts(uint32_t tiles, char* base, CountBuffers& b)
{
    Carver c{base};
    b.stats = c.take<OrderStats>(1);
    b.total = c.take<unsigned long long>(1);
    b.tile = c.take<unsigned long long>(tiles);
    return c.used + 256;
}

struct SortBuffers { uint64_t* keys[2]; uint32_t* vals[2]; uint32_t *counts, *tot; };

size_t carve_sort(uint64_t w, char* base, SortBuffers& b)
{
    Carver c{base};
    b.keys[0] = c.take<uint64_t>(w); b.keys[1] = c.take<uint64_t>(w);
    b.vals[0] = c.take<uint32_t>(w); b.vals[1] = c.take<uint32_t>(w);
    b.counts = c.take<uint32_t>(fqd_internal_radix_counts(w)); b.tot = c.take<uint32_t>(256);
    return c.used + 256;
}

} // namespace

extern "C" {

int fqd_size_filter(fqd_engine* e, const uint32_t* size, uint64_t n, uint32_t min_size, uint32_t max_size, uint8_t* keep,
                    uint64_t* clusters_dropped, uint64_t* records_dropped)
{
    if (!e) return FQD_ERR_ARG;
    if (clusters_dropped) *clusters_dropped = 0;
    if (records_dropped) *records_dropped = 0;
    if (n >= 0x80000000ull || (n && (!size || !keep)) || min_size == 0u || min_size > fqdorder::kMaxSize ||
        (max_size != 0u && (max_size < min_size || max_size > fqdorder::kMaxSize)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_filter: bad arguments (the sizes and keep flags of at most 2^31-1 records, 1 <= min_size <= 2^31-1, max_size 0 for none or min_size <= max_size <= 2^31-1)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(size, keep)) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_filter: size and keep are device memory");
    hipStream_t s = fqd_internal_stream(e);
    void* small = nullptr;
    const int rc = fqd_internal_scratch(e, 1, 4096, &small);
    if (rc) return rc;
    FilterCounts* counts = static_cast<FilterCounts*>(small);
    FQD_TRY(e, hipMemsetAsync(counts, 0, sizeof(FilterCounts), s));
    const uint32_t grid = grid_for((n + 3u) / 4u, kBlock, 4096);
    if (reinterpret_cast<uintptr_t>(size) % 16u == 0 && reinterpret_cast<uintptr_t>(keep) % 4u == 0)
        hipLaunchKernelGGL(size_filter_kernel<true>, dim3(grid), dim3(kBlock), 0, s, size, n, min_size, max_size, keep, counts);
    else
        hipLaunchKernelGGL(size_filter_kernel<false>, dim3(grid), dim3(kBlock), 0, s, size, n, min_size, max_size, keep, counts);
    FQD_TRY(e, hipGetLastError());
    FilterCounts got{};
    FQD_TRY(e, hipMemcpyAsync(&got, counts, sizeof got, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (got.bad) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_filter: a kept record has cluster size 0 (are keep and size those of one grouping, after fqd_heads_to_keep?)");
    if (clusters_dropped) *clusters_dropped = got.clusters;
    if (records_dropped) *records_dropped = got.records;
    return FQD_OK;
}

int fqd_size_order(fqd_engine* e, const uint32_t* perm, const uint8_t* head, const uint32_t* size, const uint8_t* keep, uint64_t n,
                   uint32_t* order, uint64_t* n_written)
{
    return fqd_size_order_ex(e, perm, head, size, keep, n, order, n_written, nullptr);
}

int fqd_size_order_ex(fqd_engine* e, const uint32_t* perm, const uint8_t* head, const uint32_t* size, const uint8_t* keep, uint64_t n,
                      uint32_t* order, uint64_t* n_written, fqd_size_order_info* info)
{
    if (!e) return FQD_ERR_ARG;
    if (n_written) *n_written = 0;
    if (info) *info = fqd_size_order_info{};
    if (n >= 0x80000000ull || !n_written || (n && (!perm || !head || !size || !keep || !order)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_order: bad arguments (the order, its head flags, the sizes and keep flags of at most 2^31-1 records, room for the written order and for its length)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(perm, head, size, keep, order))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_order: perm, head, size, keep and order are device memory");
    hipStream_t s = fqd_internal_stream(e);
    uint8_t head0 = 0;
    FQD_TRY(e, hipMemcpyAsync(&head0, head, 1, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (!head0) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_order: head[0] is not set: place 0 starts the first cluster (nothing was written)");
    const uint32_t tiles = uint32_t((n + kOffTile - 1) / kOffTile);
    CountBuffers cb{};
    void* base = nullptr;
    int rc = fqd_internal_scratch(e, 1, carve_counts(tiles, nullptr, cb), &base);
    if (rc) return rc;
    (void)carve_counts(tiles, static_cast<char*>(base), cb);
    FQD_TRY(e, hipMemsetAsync(cb.stats, 0, sizeof(OrderStats), s));
    hipLaunchKernelGGL(order_tiles_kernel, dim3(tiles), dim3(kBlock), 0, s, perm, head, keep, n, cb.tile);
    hipLaunchKernelGGL(fqdscan::scan_tiles_kernel<unsigned long long>, dim3(1), dim3(1024), 0, s, cb.tile, tiles, cb.total);
    FQD_TRY(e, hipGetLastError());
    unsigned long long w = 0;
    FQD_TRY(e, hipMemcpyAsync(&w, cb.total, sizeof w, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (w == 0) return FQD_OK;                              // nothing is written: order stays as it is
    SortBuffers sb{};
    if ((rc = fqd_internal_scratch(e, 0, carve_sort(w, nullptr, sb), &base))) return rc;
    (void)carve_sort(w, static_cast<char*>(base), sb);
    hipLaunchKernelGGL(order_places_kernel, dim3(tiles), dim3(kBlock), 0, s, perm, head, keep, size, n,
                       static_cast<const unsigned long long*>(cb.tile), w, sb.keys[0], sb.vals[0], cb.stats);
    FQD_TRY(e, hipGetLastError());
    OrderStats st{};
    FQD_TRY(e, hipMemcpyAsync(&st, cb.stats, sizeof st, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (st.bad) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_order: a kept record has cluster size 0 (are keep and size those of one grouping, after fqd_heads_to_keep?); nothing was written");
    // tier 1: one pass over all W pairs; tier 2: the L pairs of bucket 0 alone
    int cur = 0;
    if ((rc = fqd_internal_radix_sort(e, s, sb.keys, sb.vals, sb.counts, sb.tot, w, 8u, &cur))) return rc;
    const uint64_t L = st.above;
    const uint32_t bits = fqdorder::tier2_bits(st.largest);
    int top = cur;
    uint32_t passes = 0;
    if (L > 1 && bits) {
        hipLaunchKernelGGL(order_rekey_kernel, dim3(grid_for(L, kBlock, 4096)), dim3(kBlock), 0, s, sb.keys[cur], L, st.largest);
        if ((rc = fqd_internal_radix_sort(e, s, sb.keys, sb.vals, sb.counts, sb.tot, L, bits, &top))) return rc;
        passes = fqdorder::tier2_passes(st.largest);         // (what the call above has just launched over the L pairs)
    }
    if (L) FQD_TRY(e, hipMemcpyAsync(order, sb.vals[top], L * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    if (w > L) FQD_TRY(e, hipMemcpyAsync(order + L, sb.vals[cur] + L, (w - L) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, hipStreamSynchronize(s));                     // the scratch may be reused by the next call
    *n_written = w;
    if (info) { info->written = w; info->large = L; info->largest = st.largest; info->tier2_passes = passes; }
    return FQD_OK;
}

int fqd_take_u32(fqd_engine* e, const uint32_t* values, const uint32_t* idx, uint64_t n, uint32_t* out)
{
    if (!e) return FQD_ERR_ARG;
    if (n && (!values || !idx || !out)) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_take_u32: bad arguments");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(values, idx, out)) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_take_u32: values, idx and out are device memory");
    hipLaunchKernelGGL(take_u32_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, fqd_internal_stream(e), values, idx, n, out);
    FQD_TRY(e, hipGetLastError());
    return FQD_OK;
}

} // extern "C"
