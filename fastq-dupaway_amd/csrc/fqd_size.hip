// fqd_size.hip — FQD_FAST_SIZEOUT / FQD_FAST_LEVELS of the `--fast` mode (same library as fqd_engine.hip): every cluster's
// member count from the grouping of fqd_owner.hip, the `;size=N` label's place and the grown size of every written record,
// and the copy that puts the label in as the survivors leave.  Rules and proofs: fqd_size_core.hpp.
//
//   sizes    fqd_cluster_sizes: a max-scan of "the last head at or in front of this place" over (perm, head) in the three
//            launches of fqd_output_plan's scan — size_tiles_kernel (kOffTile places a block, one value a tile),
//            size_carry_kernel (one block over the tile values, exclusive), size_places_kernel (kOffTile places a block
//            again).  The last place of a run stores the run's length at the record of its head place, every place that
//            is no head stores 0 at its own record: n stores to n entries, none of them atomic.  The level counts go wave
//            by wave into LDS (lanes that end a run agree level by level through ballots) and from there with one global
//            atomic per block and level; the largest size the same way.
//   labels   size_labels_kernel: a wave takes a tile of 64 neighbouring records and works through it four at a time, SIXTEEN
//            LANES A RECORD, sixteen bytes a lane — umi_find_kernel's search for the first word's end (fqdumi::lane_look),
//            without the separator.  Kept records of size 0 are counted, not reported one by one.
//   copy     copy_labelled_kernel: fqd_copy_spans' eight lanes a span, each of the two parts around the label by that
//            kernel's rule; the second part's stores are unaligned by the label's length.
#include <hip/hip_runtime.h>

#include "fqd_internal.hpp"
#include "fqd_size_core.hpp"
#include "fqd_umi_core.hpp"
#include "fqd_wave.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kOffTile = kBlock * 8;                         // places a block of the scan's two passes (fqd_record_scan.hpp's)
constexpr uint32_t kGroup = 16;                              // lanes a record (labels)
constexpr uint32_t kWaveTile = 64;                           // records a wave (labels)
constexpr uint32_t kTile = kWaveTile * (kBlock / 64);        // records a block (labels)
constexpr uint32_t kNone = fqdsize::kNone;
constexpr uint32_t kSpanLanes = fqdsize::kSpanLanes;

static_assert(sizeof(fqd_size_levels) == 2 * 16 * 8 + 8, "fqd_size_levels is two tables of sixteen 64-bit counts and two 32-bit words");

// ---- sizes -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void size_tiles_kernel(const uint8_t* __restrict__ head, uint64_t n, uint32_t* __restrict__ tile_last)
{
    __shared__ uint32_t ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    uint32_t last = kNone;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const uint64_t k = base + uint32_t(e); if (k < n && head[k]) last = uint32_t(k); }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) last = fqdsize::combine(last, __shfl_down(last, d, 64));
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = last;
    __syncthreads();
    if (threadIdx.x == 0) tile_last[blockIdx.x] = fqdsize::combine(fqdsize::combine(ws[0], ws[1]), fqdsize::combine(ws[2], ws[3]));
}

// (scan_tiles_kernel's shape with combine for the sum: exclusive, in place, by one block.  fqd_wave.hpp's scans are sums only:
// this one and fqd_seq_pick.hip's are the two over another operation, too few for a helper over operation and identity.)
__global__ __launch_bounds__(1024)
void size_carry_kernel(uint32_t* __restrict__ data, uint32_t n)
{
    __shared__ uint32_t wt[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = kNone;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t t0 = 0; t0 < n; t0 += 1024u) {
        const uint32_t i = t0 + threadIdx.x;
        const uint32_t v = i < n ? data[i] : kNone;
        uint32_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(inc, d, 64); if (int(lane) >= d) inc = fqdsize::combine(up, inc); }
        const uint32_t left = __shfl_up(inc, 1, 64);             // (there is no taking v out of a maximum again)
        if (lane == 63u) wt[wave] = inc;
        __syncthreads();
        uint32_t before = carry;
        for (uint32_t w = 0; w < wave; ++w) before = fqdsize::combine(before, wt[w]);
        if (i < n) data[i] = lane ? fqdsize::combine(before, left) : before;
        __syncthreads();
        if (threadIdx.x == 1023u) carry = fqdsize::combine(before, inc);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock)
void size_places_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ head, uint64_t n,
                        const uint32_t* __restrict__ tile_carry, uint32_t* __restrict__ size, fqd_size_levels* levels)
{
    __shared__ uint32_t ws[4];
    __shared__ uint32_t s_clusters[fqdsize::kLevels];
    __shared__ unsigned long long s_records[fqdsize::kLevels];
    __shared__ uint32_t s_largest;
    if (threadIdx.x < fqdsize::kLevels) { s_clusters[threadIdx.x] = 0; s_records[threadIdx.x] = 0; }
    if (threadIdx.x == 0) s_largest = 0;
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    uint8_t h[9];                                            // h[8]: does the place behind this lane's eight start a run?
    uint32_t last = kNone;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        const uint64_t k = base + uint32_t(e);
        h[e] = k < n ? head[k] : (k == n ? 1 : 0);           // (the place behind the last ends its run as a head would)
        if (e < 8 && k < n && h[e]) last = uint32_t(k);
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = last;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(inc, d, 64); if (int(lane) >= d) inc = fqdsize::combine(up, inc); }
    const uint32_t left = __shfl_up(inc, 1, 64);
    if (lane == 63u) ws[wave] = inc;
    __syncthreads();
    uint32_t start = tile_carry[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) start = fqdsize::combine(start, ws[w]);
    if (lane) start = fqdsize::combine(start, left);
    uint32_t largest = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint64_t k = base + uint32_t(e);
        uint32_t run = 0;                                    // the length of the run that ends here, 0: none does
        if (k < n) {
            if (h[e]) start = uint32_t(k);
            else { const uint32_t r = perm[k]; if (r < n) size[r] = 0; }   // (an order that is no permutation of 0 .. n-1 never leaves size[])
            if (h[e + 1] && start != kNone) {
                run = uint32_t(k) + 1u - start;
                const uint32_t r = perm[start];
                if (r < n) size[r] = run;
            }
        }
        if (levels) {                                        // (the same for every lane: the ballots below are the whole wave's)
            largest = run > largest ? run : largest;
            const uint32_t lv = run ? fqdsize::level(run) : fqdsize::kLevels;
            unsigned long long todo = __ballot(lv < fqdsize::kLevels);
            while (todo) {
                const uint32_t L = __shfl(lv, __ffsll(todo) - 1, 64);
                const bool mine = lv == L;
                const unsigned long long m = __ballot(mine);
                // the rows 1 .. 9 hold one size each; the others take the sum
                const unsigned long long records = L < 9u ? uint64_t(__popcll(m)) * (L + 1u) : fqdwave::wave_sum<unsigned long long>(mine ? run : 0u);
                if (lane == 0) { atomicAdd(&s_clusters[L], uint32_t(__popcll(m))); atomicAdd(&s_records[L], records); }
                todo &= ~m;
            }
        }
    }
    if (!levels) return;
    largest = fqdwave::wave_max(largest);
    if (lane == 0 && largest) atomicMax(&s_largest, largest);
    __syncthreads();
    if (threadIdx.x < fqdsize::kLevels && s_clusters[threadIdx.x]) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&levels->clusters[threadIdx.x]), static_cast<unsigned long long>(s_clusters[threadIdx.x]));
        atomicAdd(reinterpret_cast<unsigned long long*>(&levels->records[threadIdx.x]), s_records[threadIdx.x]);
    }
    if (threadIdx.x == fqdsize::kLevels && s_largest) atomicMax(&levels->largest, s_largest);
}

// ---- labels ----------------------------------------------------------------------------------------------------------------

// One wave per tile of kWaveTile records; see the head of the file.
__global__ __launch_bounds__(kBlock)
void size_labels_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ id_start, const uint32_t* __restrict__ id_len,
                        const uint32_t* __restrict__ rec_size, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ size,
                        uint64_t n, uint32_t* __restrict__ label_at, uint32_t* __restrict__ out_size, unsigned long long* __restrict__ n_bad)
{
    const uint32_t lane = threadIdx.x & 63u, g = lane / kGroup, gl = lane % kGroup;
    const uint64_t tile0 = (uint64_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6)) * kWaveTile;
    if (tile0 >= n) return;                                  // (the whole wave)
    const uint64_t mine = tile0 + lane;
    unsigned long long line_at = 0;
    uint32_t line_len = 0;
    if (mine < n) { line_at = id_start[mine]; line_len = id_len[mine]; }
    uint32_t my_end = 0;
    for (uint32_t j = 0; j < kWaveTile / 4u && tile0 + 4u * j < n; ++j) {
        const int r = int(4u * j + g);                       // the group's record of this step (beyond n: an empty line)
        const uint8_t* __restrict__ line = text + __shfl(line_at, r, 64);
        const uint32_t L = __shfl(line_len, r, 64);
        const uint32_t chunks = fqdumi::line_chunks(L);
        uint32_t end = fqdumi::kNone;
        for (uint32_t c0 = 0; __any(end == fqdumi::kNone && c0 < chunks); c0 += kGroup) {
            const bool live = end == fqdumi::kNone && c0 < chunks;
            fqdumi::Look k{0u, 0u, 0u};
            if (live) k = fqdumi::lane_look(line, L, uint8_t(' '), c0, gl);     // (the separator masks are not looked at)
            const uint32_t e = fqdwave::group_min<kGroup>(fqdumi::look_end(k));
            if (live) end = e;
        }
        if (end == fqdumi::kNone) end = L;                   // no word end in the line: the word ends with it
        const uint32_t got = __shfl(end, int((lane & 3u) * kGroup), 64);
        if ((lane >> 2) == j) my_end = got;                  // record `lane` of the tile is group lane%4's at step lane/4
    }
    uint32_t bad = 0;
    if (mine < n) {
        const bool kept = keep[mine] != 0;
        const uint32_t N = kept ? size[mine] : 0u;
        label_at[mine] = my_end;
        out_size[mine] = rec_size[mine] + (kept ? fqdsize::label_len(N) : 0u);
        bad = kept && N == 0u;
    }
    bad = fqdwave::wave_sum(bad);
    if (lane == 0 && bad) atomicAdd(n_bad, static_cast<unsigned long long>(bad));
}

// ---- copy ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void copy_labelled_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off, const uint32_t* __restrict__ len,
                          const uint32_t* __restrict__ label_at, const uint32_t* __restrict__ size, uint64_t n,
                          uint8_t* __restrict__ dst, const uint64_t* __restrict__ dst_off)
{
    const uint32_t l = threadIdx.x % kSpanLanes;
    for (uint64_t i = (blockIdx.x * uint64_t(kBlock) + threadIdx.x) / kSpanLanes; i < n; i += uint64_t(gridDim.x) * (kBlock / kSpanLanes)) {
        const uint32_t L = len[i];
        if (L == 0) continue;
        fqdsize::copy_labelled_lane(src + src_off[i], dst + dst_off[i], L, label_at[i], size[i], l);
    }
}

// Is p memory the device can be handed?  Asked of the runtime's bookkeeping: nothing is allocated or touched.
struct SizeBuffers { uint32_t* tile; fqd_size_levels* levels; };

size_t carve_sizes(uint32_t tiles, char* base, SizeBuffers& b)
{
    Carver c{base};
    b.levels = c.take<fqd_size_levels>(1);
    b.tile = c.take<uint32_t>(tiles);
    return c.used + 256;
}

} // namespace

extern "C" {

int fqd_cluster_sizes(fqd_engine* e, const uint32_t* perm, const uint8_t* head, uint64_t n, uint32_t* size, fqd_size_levels* levels)
{
    if (!e) return FQD_ERR_ARG;
    if (levels) *levels = fqd_size_levels{};
    if (n >= 0x80000000ull || (n && (!perm || !head || !size)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_cluster_sizes: bad arguments (the order, its head flags and room for the sizes of at most 2^31-1 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(perm, head, size))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_cluster_sizes: perm, head and size are device memory");
    hipStream_t s = fqd_internal_stream(e);
    uint8_t head0 = 0;
    FQD_TRY(e, hipMemcpyAsync(&head0, head, 1, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (!head0) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_cluster_sizes: head[0] is not set: place 0 starts the first cluster (nothing was written)");
    const uint32_t tiles = uint32_t((n + kOffTile - 1) / kOffTile);
    SizeBuffers b{};
    void* base = nullptr;
    const int rc = fqd_internal_scratch(e, 1, carve_sizes(tiles, nullptr, b), &base);
    if (rc) return rc;
    (void)carve_sizes(tiles, static_cast<char*>(base), b);
    if (levels) FQD_TRY(e, hipMemsetAsync(b.levels, 0, sizeof(fqd_size_levels), s));
    hipLaunchKernelGGL(size_tiles_kernel, dim3(tiles), dim3(kBlock), 0, s, head, n, b.tile);
    hipLaunchKernelGGL(size_carry_kernel, dim3(1), dim3(1024), 0, s, b.tile, tiles);
    hipLaunchKernelGGL(size_places_kernel, dim3(tiles), dim3(kBlock), 0, s, perm, head, n, static_cast<const uint32_t*>(b.tile), size,
                       levels ? b.levels : nullptr);
    FQD_TRY(e, hipGetLastError());
    if (levels) FQD_TRY(e, hipMemcpyAsync(levels, b.levels, sizeof(fqd_size_levels), hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    return FQD_OK;
}

int fqd_size_labels(fqd_engine* e, const uint8_t* text, const uint64_t* start, const uint32_t* id_len, const uint32_t* rec_size,
                    const uint8_t* keep, const uint32_t* size, uint64_t n, uint32_t* label_at, uint32_t* out_size)
{
    if (!e) return FQD_ERR_ARG;
    if (n >= 0x100000000ull || (n && (!text || !start || !id_len || !rec_size || !keep || !size || !label_at || !out_size)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_labels: bad arguments (the text, the records' starts, ID line lengths, sizes, keep flags and cluster sizes, and room for label_at and out_size of at most 2^32-1 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(text, start, id_len, rec_size, keep, size, label_at, out_size))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_labels: the text and every array are device memory");
    hipStream_t s = fqd_internal_stream(e);
    void* small = nullptr;
    const int rc = fqd_internal_scratch(e, 1, 4096, &small);
    if (rc) return rc;
    unsigned long long* n_bad = static_cast<unsigned long long*>(small);
    FQD_TRY(e, hipMemsetAsync(n_bad, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(size_labels_kernel, dim3(uint32_t((n + kTile - 1) / kTile)), dim3(kBlock), 0, s, text, start, id_len, rec_size, keep, size, n,
                       label_at, out_size, n_bad);
    FQD_TRY(e, hipGetLastError());
    unsigned long long bad = 0;
    FQD_TRY(e, hipMemcpyAsync(&bad, n_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (bad) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_labels: a kept record has cluster size 0 (are keep and size those of one grouping, after fqd_heads_to_keep?)");
    return FQD_OK;
}

int fqd_copy_labelled(fqd_engine* e, const uint8_t* src, const uint64_t* src_off, const uint32_t* len, const uint32_t* label_at,
                      const uint32_t* size, uint64_t n, uint8_t* dst, const uint64_t* dst_off)
{
    if (!e) return FQD_ERR_ARG;
    if (n && (!src || !src_off || !len || !label_at || !size || !dst || !dst_off)) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_copy_labelled: bad arguments");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    hipLaunchKernelGGL(copy_labelled_kernel, dim3(grid_for(n * kSpanLanes, kBlock, 8192)), dim3(kBlock), 0, fqd_internal_stream(e),
                       src, src_off, len, label_at, size, n, dst, dst_off);
    FQD_TRY(e, hipGetLastError());
    return FQD_OK;
}

} // extern "C"
