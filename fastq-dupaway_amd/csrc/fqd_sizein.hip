// fqd_sizein.hip — FQD_FAST_SIZEIN of the `--fast` mode (same library as fqd_engine.hip): the `;size=N` annotations that the
// input's ID lines already carry as the records' weights, every cluster's weighted size, and the copy that puts the new
// label where the old annotation stood.  Rules and proofs: fqd_sizein_core.hpp.  Nothing in here is called unless the switch
// is set: fqd_size.hip's entries stay as they are.
//
//   parse    size_annotations_kernel: size_labels_kernel's shape — a wave takes a tile of 64 neighbouring records and works
//            through it four at a time, SIXTEEN LANES A RECORD, sixteen bytes a lane.  A lane's look (fqdumi::lane_look with
//            ';') gives the word ends and the ';' of its chunk; it tests its own ';' for the pattern with byte loads, so a
//            pattern across a chunk's or a round's edge is read where it lies.  The digits behind the first candidate go one
//            byte a lane through ballots.  The lowest refused record and its reason come back through one 64-bit atomicMin a
//            wave of (record << 3 | reason); a wave without an annotation does no other atomic either.
//   weights  fqd_cluster_weights: fqd_cluster_sizes' three launches over Seg elements (the last head, the 64-bit sum of the
//            weights since it): weight_tiles_kernel, weight_carry_kernel, weight_places_kernel.  weight[perm[k]] is a 4-byte
//            gather.  A run above 2^31-1 leaves the lowest record of its head place through an atomicMin; its sum is then
//            fetched by the places kernel once more in a mode that writes nothing else.
//   relabel  size_relabel_kernel: elementwise.
//   copy     copy_relabelled_kernel: copy_labelled_kernel with the cut.
#include <hip/hip_runtime.h>

#include "fqd_clusters_core.hpp"
#include "fqd_internal.hpp"
#include "fqd_size_core.hpp"
#include "fqd_sizein_core.hpp"
#include "fqd_umi_core.hpp"
#include "fqd_wave.hpp"

namespace {

using fqdsizein::Seg;

constexpr int kBlock = 256;
constexpr int kOffTile = kBlock * 8;                         // places a block of the scan's two passes
constexpr uint32_t kGroup = 16;                              // lanes a record (parse)
constexpr uint32_t kWaveTile = 64;                           // records a wave (parse)
constexpr uint32_t kTile = kWaveTile * (kBlock / 64);        // records a block (parse)
constexpr uint32_t kNone = fqdsizein::kNone;
constexpr uint32_t kSpanLanes = fqdsize::kSpanLanes;
using fqdclusters::kNoBad;

static_assert(sizeof(Seg) == 16, "a tile value is sixteen bytes");

// ---- parse -----------------------------------------------------------------------------------------------------------------

struct Found { unsigned long long bad, annotated, extra; };  // the lowest (record << 3 | reason); records with an annotation; the sum of weight - 1

using fqdwave::wave_sum;

// One wave per tile of kWaveTile records; see the head of the file.
__global__ __launch_bounds__(kBlock)
void size_annotations_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ id_start, const uint32_t* __restrict__ id_len,
                             uint64_t n, const uint32_t* __restrict__ expect, uint32_t* __restrict__ weight, uint32_t* __restrict__ label_at,
                             uint32_t* __restrict__ cut, Found* found)
{
    const uint32_t lane = threadIdx.x & 63u, g = lane / kGroup, gl = lane % kGroup;
    const uint64_t tile0 = (uint64_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6)) * kWaveTile;
    if (tile0 >= n) return;                                  // (the whole wave)
    const uint64_t mine = tile0 + lane;
    unsigned long long line_at = 0;
    uint32_t line_len = 0;
    if (mine < n) { line_at = id_start[mine]; line_len = id_len[mine]; }
    fqdsizein::Parsed my{1u, 0u, 0u, fqdsizein::kOk};
    for (uint32_t j = 0; j < kWaveTile / 4u && tile0 + 4u * j < n; ++j) {
        const int r = int(4u * j + g);                       // the group's record of this step (beyond n: an empty line)
        const uint8_t* __restrict__ line = text + __shfl(line_at, r, 64);
        const uint32_t L = __shfl(line_len, r, 64);

        // ---- rounds: the word's end, the first candidate and how many there are ----
        const uint32_t chunks = fqdumi::line_chunks(L);
        uint32_t end = fqdumi::kNone, first = kNone, count = 0;
        for (uint32_t c0 = 0; __any(end == fqdumi::kNone && c0 < chunks); c0 += kGroup) {
            const bool live = end == fqdumi::kNone && c0 < chunks;
            fqdumi::Look k{0u, 0u, 0u};
            if (live) k = fqdumi::lane_look(line, L, uint8_t(';'), c0, gl);
            const uint32_t e = fqdwave::group_min<kGroup>(fqdumi::look_end(k));
            fqdsizein::Cand c{kNone, 0u};
            if (live && k.seps) c = fqdsizein::lane_candidates(line, L, k, e);
            const uint32_t f = fqdwave::group_min<kGroup>(c.first), many = fqdwave::group_sum<kGroup>(c.count);
            if (live) { end = e; if (first == kNone) first = f; count += many; }
        }
        if (end == fqdumi::kNone) end = L;                   // no word end in the line: the word ends with it

        // ---- digits (all lanes: the ballots are the whole wave's) ----
        uint32_t digit = 0;
        const uint32_t cls = fqdsizein::lane_digit(line, end, first, gl, &digit);
        const uint32_t digit_mask = uint32_t((__ballot(cls == fqdsizein::kDigit) >> (kGroup * g)) & 0xFFFFull);
        const uint32_t semi_mask = uint32_t((__ballot(cls == fqdsizein::kSemi) >> (kGroup * g)) & 0xFFFFull);
        const uint32_t other_mask = uint32_t((__ballot(cls == fqdsizein::kOther) >> (kGroup * g)) & 0xFFFFull);
        const uint32_t nd = fqdsizein::digits_in_front(digit_mask);
        const uint32_t behind = (semi_mask >> nd) & 1u ? uint32_t(fqdsizein::kSemi) : (other_mask >> nd) & 1u ? uint32_t(fqdsizein::kOther) : uint32_t(fqdsizein::kBehind);
        const unsigned long long value = fqdwave::group_sum<kGroup, unsigned long long>(fqdsizein::lane_value(digit, gl, nd));
        const fqdsizein::Parsed p = fqdsizein::judge(count, first, end, nd, behind, value);

        const int from = int((lane & 3u) * kGroup);
        const uint32_t got_weight = __shfl(p.weight, from, 64), got_at = __shfl(p.label_at, from, 64);
        const uint32_t got_cut = __shfl(p.cut, from, 64), got_reason = __shfl(p.reason, from, 64);
        if ((lane >> 2) == j) my = fqdsizein::Parsed{got_weight, got_at, got_cut, got_reason};   // record `lane` of the tile is group lane%4's at step lane/4
    }
    unsigned long long word = kNoBad, annotated = 0, extra = 0;
    if (mine < n) {
        if (!my.reason && my.cut && expect && expect[mine] != my.weight) my.reason = fqdsizein::kMatesDiffer;
        if (weight) weight[mine] = my.weight;
        if (label_at) label_at[mine] = my.label_at;
        if (cut) cut[mine] = my.cut;
        if (my.reason) word = fqdclusters::bad_word(mine, my.reason);
        else if (my.cut) { annotated = 1; extra = my.weight - 1u; }
    }
    word = fqdwave::wave_min(word);
    annotated = wave_sum(annotated);
    extra = wave_sum(extra);
    if (lane == 0) {
        if (word != kNoBad) atomicMin(&found->bad, word);
        if (annotated) atomicAdd(&found->annotated, annotated);
        if (extra) atomicAdd(&found->extra, extra);
    }
}

// ---- weights -----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ Seg seg_up(const Seg& v, int d)
{
    Seg o;
    o.sum = __shfl_up(static_cast<unsigned long long>(v.sum), d, 64);
    o.head = __shfl_up(v.head, d, 64);
    o.pad = 0;
    return o;
}

// The wave's inclusive combine: lane l holds combine(v(0), .., v(l)).  (A scan over another operation than the sum, as
// fqd_size.hip's and fqd_seq_pick.hip's: fqd_wave.hpp's scans are sums only.)
__device__ __forceinline__ Seg wave_scan(Seg v, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const Seg up = seg_up(v, d); if (int(lane) >= d) v = fqdsizein::combine(up, v); }
    return v;
}

struct WeightScratch { unsigned long long n_bad, over_record, over_sum; };

// Place k's element; a record outside 0 .. n-1 has weight 0, which is counted and refused.
__device__ __forceinline__ uint32_t weight_at(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ weight, uint64_t k, uint64_t n)
{
    const uint32_t r = perm[k];
    return r < n ? weight[r] : 0u;
}

__global__ __launch_bounds__(kBlock)
void weight_tiles_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ head, const uint32_t* __restrict__ weight, uint64_t n,
                         Seg* __restrict__ tile)
{
    __shared__ Seg ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    Seg v = fqdsizein::seg_none();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint64_t k = base + uint32_t(e);
        if (k < n) v = fqdsizein::combine(v, fqdsizein::seg_of(head[k] != 0, uint32_t(k), weight_at(perm, weight, k, n)));
    }
    const uint32_t lane = threadIdx.x & 63u;
    v = wave_scan(v, lane);
    if (lane == 63u) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) tile[blockIdx.x] = fqdsizein::combine(fqdsizein::combine(ws[0], ws[1]), fqdsizein::combine(ws[2], ws[3]));
}

// (size_carry_kernel's shape: exclusive, in place, by one block)
__global__ __launch_bounds__(1024)
void weight_carry_kernel(Seg* __restrict__ data, uint32_t n)
{
    __shared__ Seg wt[16];
    __shared__ Seg carry;
    if (threadIdx.x == 0) carry = fqdsizein::seg_none();
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t t0 = 0; t0 < n; t0 += 1024u) {
        const uint32_t i = t0 + threadIdx.x;
        const Seg v = i < n ? data[i] : fqdsizein::seg_none();
        const Seg inc = wave_scan(v, lane);
        const Seg left = seg_up(inc, 1);
        if (lane == 63u) wt[wave] = inc;
        __syncthreads();
        Seg before = carry;
        for (uint32_t w = 0; w < wave; ++w) before = fqdsizein::combine(before, wt[w]);
        if (i < n) data[i] = lane ? fqdsizein::combine(before, left) : before;
        __syncthreads();
        if (threadIdx.x == 1023u) carry = fqdsizein::combine(before, inc);
        __syncthreads();
    }
}

// want == kNone: the sizes, the levels and what is wrong.  Any other want: nothing is written but *over_sum, the sum of the
// run whose head place holds record `want`.
__global__ __launch_bounds__(kBlock)
void weight_places_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ head, const uint32_t* __restrict__ weight, uint64_t n,
                          const Seg* __restrict__ tile_carry, uint32_t* __restrict__ size, fqd_size_levels* levels, WeightScratch* out, uint32_t want)
{
    __shared__ Seg ws[4];
    __shared__ uint32_t s_clusters[fqdsize::kLevels];
    __shared__ unsigned long long s_records[fqdsize::kLevels];
    __shared__ uint32_t s_largest;
    if (threadIdx.x < fqdsize::kLevels) { s_clusters[threadIdx.x] = 0; s_records[threadIdx.x] = 0; }
    if (threadIdx.x == 0) s_largest = 0;
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    uint8_t h[9];                                            // h[8]: does the place behind this lane's eight start a run?
    uint32_t rec[8], w[8];
    Seg mine = fqdsizein::seg_none();
    uint32_t zeros = 0;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        const uint64_t k = base + uint32_t(e);
        h[e] = k < n ? head[k] : (k == n ? 1 : 0);           // (the place behind the last ends its run as a head would)
        if (e < 8) {
            rec[e] = k < n ? perm[k] : kNone;
            w[e] = rec[e] < n ? weight[rec[e]] : 0u;
            if (k < n) { mine = fqdsizein::combine(mine, fqdsizein::seg_of(h[e] != 0, uint32_t(k), w[e])); zeros += w[e] == 0u; }
        }
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const Seg inc = wave_scan(mine, lane);
    const Seg left = seg_up(inc, 1);
    if (lane == 63u) ws[wave] = inc;
    __syncthreads();
    Seg cur = tile_carry[blockIdx.x];
    for (uint32_t v = 0; v < wave; ++v) cur = fqdsizein::combine(cur, ws[v]);
    if (lane) cur = fqdsizein::combine(cur, left);
    const bool report = want != kNone;
    uint32_t largest = 0;
    unsigned long long over = kNoBad;                        // the lowest record at the head place of a run above 2^31-1
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint64_t k = base + uint32_t(e);
        uint32_t run = 0;                                    // the size of the run that ends here, 0: none does (or one that is refused)
        if (k < n) {
            cur = fqdsizein::combine(cur, fqdsizein::seg_of(h[e] != 0, uint32_t(k), w[e]));
            if (!report && !h[e] && rec[e] < n) size[rec[e]] = 0;      // (an order that is no permutation of 0 .. n-1 never leaves size[])
            if (h[e + 1] && cur.head != kNone) {
                const uint32_t r = perm[cur.head];
                if (report) { if (r == want) out->over_sum = cur.sum; }
                else if (cur.sum > fqdsizein::kMaxWeight) { if (r < over) over = r; }
                else { run = uint32_t(cur.sum); if (r < n) size[r] = run; }
            }
        }
        if (levels && !report) {                             // (the same for every lane: the ballots below are the whole wave's)
            largest = run > largest ? run : largest;
            const uint32_t lv = run ? fqdsize::level(run) : fqdsize::kLevels;
            unsigned long long todo = __ballot(lv < fqdsize::kLevels);
            while (todo) {
                const uint32_t L = __shfl(lv, __ffsll(todo) - 1, 64);
                const bool same = lv == L;
                const unsigned long long m = __ballot(same);
                // the rows 1 .. 9 hold one size each; the others take the sum
                const unsigned long long records = L < 9u ? uint64_t(__popcll(m)) * (L + 1u) : wave_sum<unsigned long long>(same ? run : 0u);
                if (lane == 0) { atomicAdd(&s_clusters[L], uint32_t(__popcll(m))); atomicAdd(&s_records[L], records); }
                todo &= ~m;
            }
        }
    }
    if (report) return;
    const unsigned long long bad = wave_sum<unsigned long long>(zeros);
    over = fqdwave::wave_min(over);
    if (lane == 0) {
        if (bad) atomicAdd(&out->n_bad, bad);
        if (over != kNoBad) atomicMin(&out->over_record, over);
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

// ---- relabel and copy --------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void size_relabel_kernel(const uint32_t* __restrict__ rec_size, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ size,
                         const uint32_t* __restrict__ cut, uint64_t n, uint32_t* __restrict__ out_size, unsigned long long* __restrict__ n_bad)
{
    unsigned long long bad = 0;
    for (uint64_t r = blockIdx.x * uint64_t(kBlock) + threadIdx.x; r < n; r += uint64_t(gridDim.x) * kBlock) {
        const bool kept = keep[r] != 0;
        const uint32_t N = kept ? size[r] : 0u;
        out_size[r] = kept ? fqdsizein::relabelled_len(rec_size[r], cut[r], N) : rec_size[r];
        bad += kept && N == 0u;
    }
    bad = wave_sum(bad);
    if ((threadIdx.x & 63u) == 0 && bad) atomicAdd(n_bad, bad);
}

__global__ __launch_bounds__(kBlock)
void copy_relabelled_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off, const uint32_t* __restrict__ len,
                            const uint32_t* __restrict__ label_at, const uint32_t* __restrict__ cut, const uint32_t* __restrict__ size, uint64_t n,
                            uint8_t* __restrict__ dst, const uint64_t* __restrict__ dst_off)
{
    const uint32_t l = threadIdx.x % kSpanLanes;
    for (uint64_t i = (blockIdx.x * uint64_t(kBlock) + threadIdx.x) / kSpanLanes; i < n; i += uint64_t(gridDim.x) * (kBlock / kSpanLanes)) {
        const uint32_t L = len[i];
        if (L == 0) continue;
        fqdsizein::copy_relabelled_lane(src + src_off[i], dst + dst_off[i], L, label_at[i], cut[i], size[i], l);
    }
}

// Is p memory the device can be handed?  Asked of the runtime's bookkeeping: nothing is allocated or touched.
struct WeightBuffers { Seg* tile; fqd_size_levels* levels; WeightScratch* out; };

size_t carve_weights(uint32_t tiles, char* base, WeightBuffers& b)
{
    Carver c{base};
    b.levels = c.take<fqd_size_levels>(1);
    b.out = c.take<WeightScratch>(1);
    b.tile = c.take<Seg>(tiles);
    return c.used + 256;
}

} // namespace

extern "C" {

int fqd_size_annotations(fqd_engine* e, const uint8_t* text, const uint64_t* start, const uint32_t* id_len, uint64_t n, const uint32_t* expect,
                         uint32_t* weight, uint32_t* label_at, uint32_t* cut, fqd_sizein_info* info)
{
    if (!e) return FQD_ERR_ARG;
    if (info) *info = fqd_sizein_info{FQD_UMI_NO_RECORD, FQD_SIZEIN_OK, 0, 0, n};
    if (!info || n > 0xFFFFFFFEull || (n && (!text || !start || !id_len)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_annotations: bad arguments (info, the text, and the ID lines' starts and lengths of at most 2^32-2 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(text, start, id_len) || (expect && !on_device(expect)) || (weight && !on_device(weight)) ||
        (label_at && !on_device(label_at)) || (cut && !on_device(cut)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_annotations: the text and every array are device memory");
    hipStream_t s = fqd_internal_stream(e);
    void* scratch = nullptr;
    const int rc = fqd_internal_scratch(e, 1, 4096, &scratch);
    if (rc) return rc;
    Found* found = static_cast<Found*>(scratch);
    FQD_TRY(e, zero_counters(found, s, &Found::bad));
    hipLaunchKernelGGL(size_annotations_kernel, dim3(uint32_t((n + kTile - 1) / kTile)), dim3(kBlock), 0, s, text, start, id_len, n, expect,
                       weight, label_at, cut, found);
    FQD_TRY(e, hipGetLastError());
    Found got{};
    FQD_TRY(e, read_back(got, found, s));
    if (got.bad != kNoBad) fqdclusters::bad_parts(got.bad, &info->bad_record, &info->bad_reason);
    info->annotated = got.annotated;
    info->total_weight = n + got.extra;
    return FQD_OK;
}

int fqd_cluster_weights(fqd_engine* e, const uint32_t* perm, const uint8_t* head, const uint32_t* weight, uint64_t n, uint32_t* size,
                        fqd_size_levels* levels, fqd_weights_info* info)
{
    if (!e) return FQD_ERR_ARG;
    if (levels) *levels = fqd_size_levels{};
    if (info) *info = fqd_weights_info{FQD_UMI_NO_RECORD, 0};
    if (!info || n >= 0x80000000ull || (n && (!perm || !head || !weight || !size)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_cluster_weights: bad arguments (info, the order, its head flags, the weights and room for the sizes of at most 2^31-1 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(perm, head, weight, size))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_cluster_weights: perm, head, weight and size are device memory");
    hipStream_t s = fqd_internal_stream(e);
    uint8_t head0 = 0;
    FQD_TRY(e, hipMemcpyAsync(&head0, head, 1, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (!head0) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_cluster_weights: head[0] is not set: place 0 starts the first cluster (nothing was written)");
    const uint32_t tiles = uint32_t((n + kOffTile - 1) / kOffTile);
    WeightBuffers b{};
    void* base = nullptr;
    const int rc = fqd_internal_scratch(e, 1, carve_weights(tiles, nullptr, b), &base);
    if (rc) return rc;
    (void)carve_weights(tiles, static_cast<char*>(base), b);
    if (levels) FQD_TRY(e, hipMemsetAsync(b.levels, 0, sizeof(fqd_size_levels), s));
    FQD_TRY(e, zero_counters(b.out, s, &WeightScratch::over_record));
    hipLaunchKernelGGL(weight_tiles_kernel, dim3(tiles), dim3(kBlock), 0, s, perm, head, weight, n, b.tile);
    hipLaunchKernelGGL(weight_carry_kernel, dim3(1), dim3(1024), 0, s, b.tile, tiles);
    hipLaunchKernelGGL(weight_places_kernel, dim3(tiles), dim3(kBlock), 0, s, perm, head, weight, n, static_cast<const Seg*>(b.tile), size,
                       levels ? b.levels : nullptr, b.out, kNone);
    FQD_TRY(e, hipGetLastError());
    WeightScratch got{};
    FQD_TRY(e, hipMemcpyAsync(&got, b.out, sizeof got, hipMemcpyDeviceToHost, s));
    if (levels) FQD_TRY(e, hipMemcpyAsync(levels, b.levels, sizeof(fqd_size_levels), hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (got.n_bad) {
        if (levels) *levels = fqd_size_levels{};
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_cluster_weights: a record has weight 0, or the order names a record outside 0 .. n-1 (weights are 1 .. 2^31-1)");
    }
    if (got.over_record != kNoBad) {
        // the run's exact sum: the places once more, writing nothing but it
        hipLaunchKernelGGL(weight_places_kernel, dim3(tiles), dim3(kBlock), 0, s, perm, head, weight, n, static_cast<const Seg*>(b.tile), size,
                           static_cast<fqd_size_levels*>(nullptr), b.out, uint32_t(got.over_record));
        FQD_TRY(e, hipGetLastError());
        FQD_TRY(e, read_back(got.over_sum, &b.out->over_sum, s));
        info->over_record = got.over_record;
        info->over_sum = got.over_sum;
        if (levels) *levels = fqd_size_levels{};
    }
    return FQD_OK;
}

int fqd_size_relabel(fqd_engine* e, const uint32_t* rec_size, const uint8_t* keep, const uint32_t* size, const uint32_t* cut, uint64_t n,
                     uint32_t* out_size)
{
    if (!e) return FQD_ERR_ARG;
    if (n >= 0x100000000ull || (n && (!rec_size || !keep || !size || !cut || !out_size)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_relabel: bad arguments (the records' sizes, keep flags, cluster sizes and cuts, and room for out_size of at most 2^32-1 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(rec_size, keep, size, cut, out_size))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_relabel: every array is device memory");
    hipStream_t s = fqd_internal_stream(e);
    void* small = nullptr;
    const int rc = fqd_internal_scratch(e, 1, 4096, &small);
    if (rc) return rc;
    unsigned long long* n_bad = static_cast<unsigned long long*>(small);
    FQD_TRY(e, hipMemsetAsync(n_bad, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(size_relabel_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, rec_size, keep, size, cut, n, out_size, n_bad);
    FQD_TRY(e, hipGetLastError());
    unsigned long long bad = 0;
    FQD_TRY(e, read_back(bad, n_bad, s));
    if (bad) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_size_relabel: a kept record has cluster size 0 (are keep and size those of one grouping, after fqd_heads_to_keep?)");
    return FQD_OK;
}

int fqd_copy_relabelled(fqd_engine* e, const uint8_t* src, const uint64_t* src_off, const uint32_t* len, const uint32_t* label_at,
                        const uint32_t* cut, const uint32_t* size, uint64_t n, uint8_t* dst, const uint64_t* dst_off)
{
    if (!e) return FQD_ERR_ARG;
    if (n && (!src || !src_off || !len || !label_at || !cut || !size || !dst || !dst_off)) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_copy_relabelled: bad arguments");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    hipLaunchKernelGGL(copy_relabelled_kernel, dim3(grid_for(n * kSpanLanes, kBlock, 8192)), dim3(kBlock), 0, fqd_internal_stream(e),
                       src, src_off, len, label_at, cut, size, n, dst, dst_off);
    FQD_TRY(e, hipGetLastError());
    return FQD_OK;
}

} // extern "C"
