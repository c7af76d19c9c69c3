// fqd_seq_pick.hip — FQD_SEQ_KEEP=best of the sequence-based modes (same library as fqd_seq.hip): the member of every
// cluster of duplicates with the best quality line takes the place of the cluster's head in the order, so that the
// unchanged output plan and writers write IT.  Rules and proofs: fqd_seq_pick_core.hpp.
//
//   scores   fqd_seq_scores: every record's score (the sum of its quality bytes above '!'), in input order.  Reads every
//            quality byte once: eight lanes to a record, 8 bytes a lane and step, from the record's END backwards until
//            a word holds the '\n' in front of the last line — the sum and the search are one pass.
//   pick     fqd_seq_pick_best: a segmented arg-max over the sorted order (segments start at the head flags), cut into
//            lanes, waves, workgroups and tiles: tile aggregates, one block over the aggregates, then every tile again
//            with what came before it.  The last place of a segment knows the segment's start and its best member.
//   swap     one lane per head swaps perm[head place] with perm[best place] where they differ.
#include <hip/hip_runtime.h>

#include "fqd_internal.hpp"
#include "fqd_seq_pick_core.hpp"

namespace {

using fqdseq::Pick;

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------------------------
// scores
constexpr uint32_t kScoreLanes = 8;                      // lanes per record: 8 x 8 bytes = 64 bytes a step

// Eight bytes of text at p + a; what lies below `lo` (the record's start) reads as '\n': the search ends there at the
// latest, and nothing in front of the record (or of the text) is touched.
__device__ __forceinline__ uint64_t word_at(const uint8_t* p, int64_t a, int64_t lo)
{
    uint64_t x;
    if (a >= lo) { __builtin_memcpy(&x, p + a, 8); return x; }
    x = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) x |= uint64_t(a + j >= lo ? p[a + j] : uint8_t('\n')) << (8 * j);
    return x;
}

// The score of the last line of the record at text[off, off + len), not yet saturated, in every lane of the record's
// group.  `live` and the record are the same in the eight lanes of a group; every lane of the wave takes every ballot.
__device__ __forceinline__ uint64_t last_line_sum(const uint8_t* text, uint64_t off, uint32_t len, bool live, uint32_t sub, uint32_t shift)
{
    const int64_t lo = int64_t(off);
    int64_t pos = lo + int64_t(len);                     // the line ends before pos
    bool active = live && len != 0;
    if (active && text[pos - 1] == uint8_t('\n')) --pos;
    uint64_t sum = 0;
    while (__any(active)) {
        bool has = false;
        uint32_t whole = 0, behind = 0;
        if (active) {
            const uint64_t x = word_at(text, pos - 8 * int64_t(sub + 1u), lo);
            whole = fqdseq::word_score(x);
            behind = fqdseq::word_score_after_newline(x, &has);
        }
        const uint32_t ended = uint32_t(__ballot(has) >> shift) & 0xFFu;     // lanes of my group whose word holds a '\n'
        if (active) {
            if (!ended) { sum += whole; pos -= 8 * int64_t(kScoreLanes); }
            else {
                const uint32_t first = uint32_t(__builtin_ctz(ended));       // the one nearest to the record's end
                if (sub < first) sum += whole;
                else if (sub == first) sum += behind;
                active = false;
            }
        }
    }
    sum += __shfl_xor(sum, 1, 64); sum += __shfl_xor(sum, 2, 64); sum += __shfl_xor(sum, 4, 64);
    return sum;
}

__global__ __launch_bounds__(kBlock)
void seq_scores_kernel(const uint8_t* __restrict__ t1, const uint64_t* __restrict__ o1, const uint32_t* __restrict__ l1,
                       const uint8_t* __restrict__ t2, const uint64_t* __restrict__ o2, const uint32_t* __restrict__ l2,
                       uint64_t n, uint32_t* __restrict__ score)
{
    const uint32_t sub = threadIdx.x & (kScoreLanes - 1u), shift = threadIdx.x & 63u & ~(kScoreLanes - 1u);
    const uint64_t group = (blockIdx.x * uint64_t(kBlock) + threadIdx.x) / kScoreLanes, groups = uint64_t(gridDim.x) * kBlock / kScoreLanes;
    const uint64_t rounds = (n + groups - 1) / groups;   // the same in every lane: the ballots stay whole
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t i = r * groups + group;
        const bool live = i < n;
        uint32_t s = fqdseq::saturate_score(last_line_sum(t1, live ? o1[i] : 0u, live ? l1[i] : 0u, live, sub, shift));
        if (t2) s = fqdseq::add_scores(s, fqdseq::saturate_score(last_line_sum(t2, live ? o2[i] : 0u, live ? l2[i] : 0u, live, sub, shift)));
        if (live && sub == 0) score[i] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// pick: a tile = kBlock lanes x kPickPer consecutive places each
constexpr uint32_t kPickPer = 8;
constexpr uint32_t kPickTile = kBlock * kPickPer;        // 2048

__device__ __forceinline__ Pick shfl_up_pick(Pick v, int d)
{
    return Pick{__shfl_up((unsigned long long)v.best, d, 64), __shfl_up(v.start, d, 64)};
}

// (A scan over fqdseq::combine, not a sum: it stays here.  fqd_wave.hpp's block_exclusive is for sums only — this one and
// fqd_size.hip's are too few users for a helper over operation, identity and shuffle.)
// The combined element of everything in the block BEFORE this lane (lanes in order), and the block's whole in `total`.
__device__ __forceinline__ Pick block_exclusive_pick(Pick v, Pick* ws, Pick& total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    Pick inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const Pick up = shfl_up_pick(inc, d); if (int(lane) >= d) inc = fqdseq::combine(up, inc); }
    if (lane == 63u) ws[wave] = inc;
    Pick ex = shfl_up_pick(inc, 1);
    if (lane == 0) ex = fqdseq::pick_identity();
    __syncthreads();
    Pick before = fqdseq::pick_identity();
    for (uint32_t k = 0; k < wave; ++k) before = fqdseq::combine(before, ws[k]);
    total = fqdseq::combine(fqdseq::combine(ws[0], ws[1]), fqdseq::combine(ws[2], ws[3]));
    __syncthreads();
    return fqdseq::combine(before, ex);
}

// The lane's kPickPer places from `base` on: their elements (identity behind n), and whether the place BEHIND each
// starts a segment (or is n).
__device__ __forceinline__ void load_places(const uint32_t* __restrict__ score, const uint8_t* __restrict__ head,
                                            const uint32_t* __restrict__ perm, uint64_t n, uint64_t base, Pick* el, bool* last)
{
#pragma unroll
    for (uint32_t e = 0; e < kPickPer; ++e) {
        const uint64_t k = base + e;
        el[e] = k < n ? fqdseq::pick_of(score[perm[k]], uint32_t(k), k == 0 || head[k] != 0) : fqdseq::pick_identity();
        if (last) last[e] = k < n && (k + 1 == n || head[k + 1] != 0);
    }
}

__global__ __launch_bounds__(kBlock)
void pick_tile_kernel(const uint32_t* __restrict__ score, const uint8_t* __restrict__ head, const uint32_t* __restrict__ perm,
                      uint64_t n, unsigned long long* __restrict__ tile_best, uint32_t* __restrict__ tile_start)
{
    __shared__ Pick ws[4];
    Pick el[kPickPer];
    load_places(score, head, perm, n, uint64_t(blockIdx.x) * kPickTile + uint64_t(threadIdx.x) * kPickPer, el, nullptr);
    Pick mine = el[0];
#pragma unroll
    for (uint32_t e = 1; e < kPickPer; ++e) mine = fqdseq::combine(mine, el[e]);
    Pick total;
    (void)block_exclusive_pick(mine, ws, total);
    if (threadIdx.x == 0) { tile_best[blockIdx.x] = total.best; tile_start[blockIdx.x] = total.start; }
}

// One block: every tile's aggregate becomes the combined element of the tiles before it.
__global__ __launch_bounds__(kBlock)
void pick_tile_scan_kernel(unsigned long long* __restrict__ tile_best, uint32_t* __restrict__ tile_start, uint64_t tiles)
{
    __shared__ Pick ws[4];
    Pick carry = fqdseq::pick_identity();
    for (uint64_t c0 = 0; c0 < tiles; c0 += kBlock) {
        const uint64_t i = c0 + threadIdx.x;
        const Pick v = i < tiles ? Pick{tile_best[i], tile_start[i]} : fqdseq::pick_identity();
        Pick total;
        const Pick ex = fqdseq::combine(carry, block_exclusive_pick(v, ws, total));
        if (i < tiles) { tile_best[i] = ex.best; tile_start[i] = ex.start; }
        carry = fqdseq::combine(carry, total);
    }
}

// best_at[h] = the place of the best member of the segment that starts at place h, written by the segment's last place.
__global__ __launch_bounds__(kBlock)
void pick_apply_kernel(const uint32_t* __restrict__ score, const uint8_t* __restrict__ head, const uint32_t* __restrict__ perm,
                       uint64_t n, const unsigned long long* __restrict__ tile_best, const uint32_t* __restrict__ tile_start,
                       uint32_t* __restrict__ best_at)
{
    __shared__ Pick ws[4];
    Pick el[kPickPer];
    bool last[kPickPer];
    load_places(score, head, perm, n, uint64_t(blockIdx.x) * kPickTile + uint64_t(threadIdx.x) * kPickPer, el, last);
    Pick mine = el[0];
#pragma unroll
    for (uint32_t e = 1; e < kPickPer; ++e) mine = fqdseq::combine(mine, el[e]);
    Pick total;
    Pick cur = block_exclusive_pick(mine, ws, total);
    cur = fqdseq::combine(Pick{tile_best[blockIdx.x], tile_start[blockIdx.x]}, cur);
#pragma unroll
    for (uint32_t e = 0; e < kPickPer; ++e) {
        cur = fqdseq::combine(cur, el[e]);
        // place 0 starts a segment, so cur.start is a place below n wherever `last` is set
        if (last[e]) best_at[cur.start] = fqdseq::picked_place(cur.best);
    }
}

__global__ __launch_bounds__(kBlock)
void pick_swap_kernel(const uint8_t* __restrict__ head, const uint32_t* __restrict__ best_at, uint64_t n, uint32_t* __restrict__ perm,
                      unsigned long long* __restrict__ moved)
{
    unsigned long long s = 0;
    for (uint64_t k = blockIdx.x * uint64_t(kBlock) + threadIdx.x; k < n; k += uint64_t(gridDim.x) * kBlock) {
        if (k != 0 && !head[k]) continue;
        const uint32_t b = best_at[k];                   // inside the segment of k: no other lane touches these two entries
        if (b == uint32_t(k)) continue;
        const uint32_t mine = perm[k];
        perm[k] = perm[b]; perm[b] = mine;
        ++s;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(moved, s);
}

// The scratch of the pick: 4 B a place (best_at) and 12 B a tile of 2048 places.
struct PickBuffers { unsigned long long* moved; uint32_t* best_at; unsigned long long* tile_best; uint32_t* tile_start; };

size_t carve_pick(uint64_t n, uint64_t tiles, char* base, PickBuffers& b)
{
    Carver c{base};
    b.moved = c.take<unsigned long long>(1); b.best_at = c.take<uint32_t>(n);
    b.tile_best = c.take<unsigned long long>(tiles); b.tile_start = c.take<uint32_t>(tiles);
    return c.used + 256;
}

bool bad_spans(const fqd_tags* t, uint64_t n)
{
    return !t || t->n != n || (n && (!t->bytes || !t->offsets || !t->lengths));
}

} // namespace

extern "C" {

int fqd_seq_scores(fqd_engine* e, const fqd_tags* rec1, const fqd_tags* rec2, uint32_t* score)
{
    if (!e) return FQD_ERR_ARG;
    if (!rec1 || bad_spans(rec1, rec1->n) || (rec2 && bad_spans(rec2, rec1->n)) || (rec1->n && !score))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_seq_scores: bad arguments (whole records as spans, mates of equal count)");
    const uint64_t n = rec1->n;
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    hipStream_t s = fqd_internal_stream(e);
    hipLaunchKernelGGL(seq_scores_kernel, dim3(grid_for(n * kScoreLanes, kBlock, 4096)), dim3(kBlock), 0, s,
                       rec1->bytes, rec1->offsets, rec1->lengths, rec2 ? rec2->bytes : static_cast<const uint8_t*>(nullptr),
                       rec2 ? rec2->offsets : static_cast<const uint64_t*>(nullptr), rec2 ? rec2->lengths : static_cast<const uint32_t*>(nullptr),
                       n, score);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, hipStreamSynchronize(s));
    return FQD_OK;
}

int fqd_seq_pick_best(fqd_engine* e, const uint32_t* score, const uint8_t* head, uint64_t n, uint32_t* perm, uint64_t* n_moved)
{
    if (!e) return FQD_ERR_ARG;
    if ((n && (!score || !head || !perm)) || n >= 0x80000000ull)
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_seq_pick_best: bad arguments (scores, head flags and the order of at most 2^31-1 records)");
    if (n_moved) *n_moved = 0;
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    hipStream_t s = fqd_internal_stream(e);
    const uint64_t tiles = (n + kPickTile - 1) / kPickTile;
    PickBuffers b{};
    void* base = nullptr;
    const int rc = fqd_internal_scratch(e, 0, carve_pick(n, tiles, nullptr, b), &base);
    if (rc) return rc;
    (void)carve_pick(n, tiles, static_cast<char*>(base), b);
    FQD_TRY(e, hipMemsetAsync(b.moved, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(pick_tile_kernel, dim3(uint32_t(tiles)), dim3(kBlock), 0, s, score, head, static_cast<const uint32_t*>(perm), n, b.tile_best, b.tile_start);
    hipLaunchKernelGGL(pick_tile_scan_kernel, dim3(1), dim3(kBlock), 0, s, b.tile_best, b.tile_start, tiles);
    hipLaunchKernelGGL(pick_apply_kernel, dim3(uint32_t(tiles)), dim3(kBlock), 0, s, score, head, static_cast<const uint32_t*>(perm), n,
                       static_cast<const unsigned long long*>(b.tile_best), static_cast<const uint32_t*>(b.tile_start), b.best_at);
    hipLaunchKernelGGL(pick_swap_kernel, dim3(grid_for(n, kBlock, 2048)), dim3(kBlock), 0, s, head, static_cast<const uint32_t*>(b.best_at), n, perm, b.moved);
    FQD_TRY(e, hipGetLastError());
    unsigned long long got = 0;
    FQD_TRY(e, hipMemcpyAsync(&got, b.moved, sizeof got, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (n_moved) *n_moved = got;
    return FQD_OK;
}

} // extern "C"
