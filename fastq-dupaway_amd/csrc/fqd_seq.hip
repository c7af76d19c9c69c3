// fqd_seq.hip — the sequence-based modes (`--compare-seq tight|loose|tail-hamming`) on the GPU (same library as
// fqd_engine.hip).
//
// The reference sorts every record by its sequence line on disk (ExternalSorter<T> / PairedExternalSorter<T>, order =
// FastqView::cmp, fastqview.cpp:56-67: strncmp over the shorter length including the '\n', shorter first; pairs by
// (mate 1, mate 2), paired_external_sort.hpp:20-33) and then walks the sorted file with one comparator
// (seq_dup_remover.hpp:54-218).  Here the records stay where they lie in HBM:
//
//   1. census   which byte values occur in any sequence (one 256-bit map), and the longest mate 1 / mate 2; a byte
//               below '\n' is refused (it would break the equivalence of strncmp and byte order, fqd_seq_core.hpp)
//   2. code     every byte value present gets a code 1..K in byte order, 0 = "the mate has ended"; w = bits for K+1
//               codes.  A record is the string of codes of positions 0 .. M1-1 of mate 1 then 0 .. M2-1 of mate 2 (M =
//               the longest mate): its order is the order of (mate 1 + '\n', mate 2 + '\n') and equal strings are equal
//               records.  A 64-bit key word holds P = 64 / w positions (21 of ACGTN).
//   3. sort     MSD by key words with a stable LSD radix sort inside: every record by word 0 (8 passes of the radix
//               kernels of fqd_join.hip); then, level by level, only the runs of equal words that hold records which
//               are NOT all equal are sorted again by (run, next word).  A run of equal records is final as it is (the
//               sort is stable, so they are in input order).  Random reads are apart after word 0; exact duplicates are
//               a compare of neighbours, not more passes.  Nothing caps the key width.
//   4. heads    head[k] = sorted record k is written (fqd_seq_core.hpp has the rules and their proofs): tight and loose
//               compare k with k-1; tail-hamming cuts the order at certain heads and one wave walks each segment,
//               64 records per step, jumping to the first record beyond the distance (a ballot).
//
// Inputs larger than HBM go through it in RANGES of the sort order (fqd_seq_range_core.hpp): fqd_seq_prefix_keys and
// fqd_seq_plan_ranges at the end of this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "fqd_internal.hpp"
#include "fqd_record_scan.hpp"
#include "fqd_seq_core.hpp"
#include "fqd_seq_range_core.hpp"

namespace {

using fqdseq::View;
using fqdwave::block_exclusive;
using fqdwave::wave_max;
using fqdwave::wave_sum;

constexpr int kBlock = 256;

// The records' sequences: mate 1, and mate 2 when b2 != nullptr.
struct Mates {
    const uint8_t* b1; const uint64_t* o1; const uint32_t* l1;
    const uint8_t* b2; const uint64_t* o2; const uint32_t* l2;
    __device__ __forceinline__ View m1(uint32_t r) const { return View{b1 + o1[r], l1[r]}; }
    __device__ __forceinline__ View m2(uint32_t r) const { return b2 ? View{b2 + o2[r], l2[r]} : View{b1, 0u}; }
    __device__ __forceinline__ bool equal(uint32_t a, uint32_t b) const
    {
        return fqdseq::tight_match(m1(a), m1(b)) && (!b2 || fqdseq::tight_match(m2(a), m2(b)));
    }
};

// ---------------------------------------------------------------------------------------------
// 1. census: info[0..7] = bitmap of the byte values present, info[8] / info[9] = longest mate 1 / mate 2.
__device__ __forceinline__ void census_bytes(View v, uint32_t* lb)
{
    uint32_t k = 0;
    for (; k + 8u <= v.len; k += 8u) {                     // eight bytes per load; a bit is tested before it is set
        uint64_t x;
        __builtin_memcpy(&x, v.p + k, 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t c = uint32_t(x >> (8 * j)) & 255u, w = c >> 5, bit = 1u << (c & 31u);
            if (!(lb[w] & bit)) atomicOr(&lb[w], bit);
        }
    }
    for (; k < v.len; ++k) {
        const uint32_t c = v.p[k], w = c >> 5, bit = 1u << (c & 31u);
        if (!(lb[w] & bit)) atomicOr(&lb[w], bit);
    }
}

__global__ __launch_bounds__(kBlock)
void census_kernel(Mates m, uint64_t n, uint32_t* __restrict__ info)
{
    __shared__ uint32_t lb[8];
    if (threadIdx.x < 8) lb[threadIdx.x] = 0;
    __syncthreads();
    uint32_t mx1 = 0, mx2 = 0;
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
        const View a = m.m1(uint32_t(i));
        mx1 = max(mx1, a.len);
        census_bytes(a, lb);
        if (m.b2) { const View b = m.m2(uint32_t(i)); mx2 = max(mx2, b.len); census_bytes(b, lb); }
    }
    mx1 = wave_max(mx1); mx2 = wave_max(mx2);
    if ((threadIdx.x & 63) == 0) { atomicMax(&info[8], mx1); atomicMax(&info[9], mx2); }
    __syncthreads();
    if (threadIdx.x < 8 && lb[threadIdx.x]) atomicOr(&info[threadIdx.x], lb[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------
// 2. key word: positions [pos0, pos0 + npos) of list element j's record (q[j]; q == nullptr: record j), w bits each,
// position pos0 most significant.  vals[j] = j (the payload the sort carries); word_copy (may be null) keeps the word.
__global__ __launch_bounds__(kBlock)
void encode_kernel(Mates m, uint32_t M1, const uint32_t* __restrict__ q, uint64_t count, uint32_t pos0, uint32_t npos,
                   uint32_t w, const uint8_t* __restrict__ rank, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                   uint64_t* __restrict__ word_copy)
{
    __shared__ uint8_t code[256];
    code[threadIdx.x] = rank[threadIdx.x];
    __syncthreads();
    for (uint64_t j = blockIdx.x * uint64_t(kBlock) + threadIdx.x; j < count; j += uint64_t(gridDim.x) * kBlock) {
        const uint32_t r = q ? q[j] : uint32_t(j);
        const View a = m.m1(r), b = m.m2(r);
        uint64_t key = 0;
        for (uint32_t t = 0; t < npos; ++t) {
            const uint32_t pos = pos0 + t;
            uint32_t c = 0;                                  // the mate has ended
            if (pos < M1) { if (pos < a.len) c = code[a.p[pos]]; }
            else if (pos - M1 < b.len) c = code[b.p[pos - M1]];
            key = (key << w) | c;
        }
        keys[j] = key;
        vals[j] = uint32_t(j);
        if (word_copy) word_copy[j] = key;
    }
}

// ---------------------------------------------------------------------------------------------
// 3. refinement over the current list (sorted records q, their places pos in perm, run starts bnd).
// After the first sort: the list is every record in word-0 order.
__global__ __launch_bounds__(kBlock)
void first_list_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t n,
                       uint32_t* __restrict__ q, uint32_t* __restrict__ pos, uint8_t* __restrict__ bnd, uint32_t* __restrict__ perm)
{
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
        q[i] = vals[i]; pos[i] = uint32_t(i); perm[i] = vals[i];
        bnd[i] = i == 0 || keys[i] != keys[i - 1];
    }
}

// diff[j] = element j is in the same run as j-1 but its record differs from j-1's.
__global__ __launch_bounds__(kBlock)
void diff_kernel(Mates m, const uint32_t* __restrict__ q, const uint8_t* __restrict__ bnd, uint64_t count, uint8_t* __restrict__ diff)
{
    for (uint64_t j = blockIdx.x * uint64_t(kBlock) + threadIdx.x; j < count; j += uint64_t(gridDim.x) * kBlock)
        diff[j] = !bnd[j] && !m.equal(q[j - 1], q[j]);
}

// Exclusive scan of byte flags: tile sums, one block over the tiles (fqd_record_scan.hpp's scan_tiles_kernel), then every
// element; inside a block, fqd_wave.hpp's block_exclusive.
constexpr uint32_t kScanPer = 16;
constexpr uint32_t kScanTile = kBlock * kScanPer;        // 4096

__global__ __launch_bounds__(kBlock)
void tile_sum_kernel(const uint8_t* __restrict__ f, uint64_t count, uint32_t* __restrict__ tile_sum)
{
    __shared__ uint32_t ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kScanTile + uint64_t(threadIdx.x) * kScanPer;
    uint32_t s = 0;
    for (uint32_t e = 0; e < kScanPer; ++e) s += base + e < count ? (f[base + e] ? 1u : 0u) : 0u;
    s = fqdwave::block_total<4>(s, ws);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBlock)
void tile_apply_kernel(const uint8_t* __restrict__ f, uint64_t count, const uint32_t* __restrict__ tile_base, uint32_t* __restrict__ excl)
{
    __shared__ uint32_t ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kScanTile + uint64_t(threadIdx.x) * kScanPer;
    uint32_t s = 0;
    for (uint32_t e = 0; e < kScanPer; ++e) s += base + e < count ? (f[base + e] ? 1u : 0u) : 0u;
    uint32_t total = 0;
    uint32_t at = tile_base[blockIdx.x] + block_exclusive<4>(s, ws, total);
    for (uint32_t e = 0; e < kScanPer; ++e)
        if (base + e < count) { excl[base + e] = at; at += f[base + e] ? 1u : 0u; }
}

// mixed[run of j] = 1 when some element of the run differs from its predecessor.  run of j = excl(bnd)[j] + bnd[j] - 1.
__global__ __launch_bounds__(kBlock)
void mixed_kernel(const uint8_t* __restrict__ diff, const uint8_t* __restrict__ bnd, const uint32_t* __restrict__ bnd_excl,
                  uint64_t count, uint8_t* __restrict__ mixed)
{
    for (uint64_t j = blockIdx.x * uint64_t(kBlock) + threadIdx.x; j < count; j += uint64_t(gridDim.x) * kBlock)
        if (diff[j]) mixed[bnd_excl[j] + bnd[j] - 1u] = 1;     // every writer writes the same value
}

__global__ __launch_bounds__(kBlock)
void keep_kernel(const uint8_t* __restrict__ bnd, const uint32_t* __restrict__ bnd_excl, const uint8_t* __restrict__ mixed,
                 uint64_t count, uint8_t* __restrict__ keep)
{
    for (uint64_t j = blockIdx.x * uint64_t(kBlock) + threadIdx.x; j < count; j += uint64_t(gridDim.x) * kBlock)
        keep[j] = mixed[bnd_excl[j] + bnd[j] - 1u];
}

// The elements of the mixed runs, in order: their record, place in perm and run.
__global__ __launch_bounds__(kBlock)
void compact_kernel(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ keep_excl, const uint32_t* __restrict__ q,
                    const uint32_t* __restrict__ pos, const uint8_t* __restrict__ bnd, const uint32_t* __restrict__ bnd_excl,
                    uint64_t count, uint32_t* __restrict__ nq, uint32_t* __restrict__ npos, uint32_t* __restrict__ nrid)
{
    for (uint64_t j = blockIdx.x * uint64_t(kBlock) + threadIdx.x; j < count; j += uint64_t(gridDim.x) * kBlock)
        if (keep[j]) { const uint32_t k = keep_excl[j]; nq[k] = q[j]; npos[k] = pos[j]; nrid[k] = bnd_excl[j] + bnd[j] - 1u; }
}

__global__ __launch_bounds__(kBlock)
void gather_rid_kernel(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ nrid, uint64_t count, uint64_t* __restrict__ keys)
{
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < count; i += uint64_t(gridDim.x) * kBlock)
        keys[i] = nrid[vals[i]];
}

// The list after a level: element i = element vals[i] of the compacted list (now sorted by run, then word); it takes
// the i-th of the mixed runs' places in perm (runs are contiguous, so the places of a run stay the run's).
__global__ __launch_bounds__(kBlock)
void relist_kernel(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ nq, const uint32_t* __restrict__ npos,
                   const uint32_t* __restrict__ nrid, const uint64_t* __restrict__ word, uint64_t count,
                   uint32_t* __restrict__ q, uint32_t* __restrict__ pos, uint8_t* __restrict__ bnd, uint32_t* __restrict__ perm)
{
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < count; i += uint64_t(gridDim.x) * kBlock) {
        const uint32_t k = vals[i];
        q[i] = nq[k]; pos[i] = npos[i]; perm[npos[i]] = nq[k];
        if (i == 0) bnd[i] = 1;
        else { const uint32_t p = vals[i - 1]; bnd[i] = nrid[k] != nrid[p] || word[k] != word[p]; }
    }
}

// ---------------------------------------------------------------------------------------------
// 4. heads (sorted position k; fqd_seq_core.hpp).  tight / loose: the head flags; tail-hamming: the certain heads.
__global__ __launch_bounds__(kBlock)
void neighbour_heads_kernel(Mates m, const uint32_t* __restrict__ perm, uint64_t n, int mode, uint32_t d, uint8_t* __restrict__ head)
{
    const bool paired = m.b2 != nullptr;
    for (uint64_t k = blockIdx.x * uint64_t(kBlock) + threadIdx.x; k < n; k += uint64_t(gridDim.x) * kBlock) {
        uint8_t h = 1;
        if (k > 0) {
            const uint32_t a = perm[k - 1], b = perm[k];
            if (mode == fqdseq::kHamming) h = fqdseq::hamming_certain_head(d, paired, m.m1(a), m.m2(a), m.m1(b), m.m2(b));
            else                          h = !fqdseq::matches(mode, d, paired, m.m1(a), m.m2(a), m.m1(b), m.m2(b));
        }
        head[k] = h;
    }
}

// tail-hamming: cut[k] = certain head.  A wave takes 64 sorted places at a time and walks every segment that starts
// among them: the head h stays the reference, the 64 records after the current place are compared with it at once,
// the first that does not match (a ballot) is the next head.  A segment ends before the next cut.  All values that
// steer the walk are the same in every lane (ballots), so the wave stays together.
__global__ __launch_bounds__(kBlock)
void hamming_walk_kernel(Mates m, const uint32_t* __restrict__ perm, uint64_t n, uint32_t d, const uint8_t* __restrict__ cut,
                         uint8_t* __restrict__ head)
{
    const bool paired = m.b2 != nullptr;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (blockIdx.x * uint64_t(kBlock) + threadIdx.x) >> 6, n_waves = (uint64_t(gridDim.x) * kBlock) >> 6;
    const uint64_t chunks = (n + 63u) / 64u;
    for (uint64_t c = wave; c < chunks; c += n_waves) {
        const uint64_t my = c * 64u + lane;
        unsigned long long starts = __ballot(my < n && cut[my]);
        while (starts) {
            const uint64_t s = c * 64u + uint64_t(__builtin_ctzll(starts));
            starts &= starts - 1ull;
            uint64_t h = s, x = s + 1u;
            if (lane == 0) head[s] = 1;
            for (;;) {
                const uint64_t idx = x + lane;
                const bool beyond = idx >= n || cut[idx];
                const unsigned long long ends = __ballot(beyond);
                const uint32_t limit = ends ? uint32_t(__builtin_ctzll(ends)) : 64u;
                bool differs = false;
                if (lane < limit) {
                    const uint32_t r = perm[h], y = perm[idx];
                    differs = !fqdseq::matches(fqdseq::kHamming, d, paired, m.m1(r), m.m2(r), m.m1(y), m.m2(y));
                }
                const unsigned long long nm = __ballot(differs);
                if (nm) {
                    h = x + uint64_t(__builtin_ctzll(nm));
                    if (lane == 0) head[h] = 1;
                    x = h + 1u;
                    continue;
                }
                if (limit < 64u) break;
                x += 64u;
            }
        }
    }
}

__global__ __launch_bounds__(kBlock)
void clear_kernel(uint8_t* __restrict__ f, uint64_t n)
{
    for (uint64_t k = blockIdx.x * uint64_t(kBlock) + threadIdx.x; k < n; k += uint64_t(gridDim.x) * kBlock) f[k] = 0;
}

__global__ __launch_bounds__(kBlock)
void count_kernel(const uint8_t* __restrict__ f, uint64_t n, unsigned long long* __restrict__ total)
{
    unsigned long long s = 0;
    for (uint64_t k = blockIdx.x * uint64_t(kBlock) + threadIdx.x; k < n; k += uint64_t(gridDim.x) * kBlock) s += f[k] ? 1u : 0u;
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}

// ---------------------------------------------------------------------------------------------
struct SortBuffers {
    uint64_t* keys[2]; uint32_t* vals[2]; uint32_t *counts, *tot;
    uint32_t *q, *pos, *nq, *npos, *nrid, *bnd_excl, *keep_excl, *tiles;
    unsigned long long* total;
    uint8_t *bnd, *diff, *mixed, *keep, *rank;
    uint64_t* word;
};

void carve(uint64_t n, SortBuffers& b, char* base, size_t* bytes)
{
    Carver c{base};
    const size_t tiles = (n + kScanTile - 1) / kScanTile + 1;
    b.keys[0] = c.take<uint64_t>(n); b.keys[1] = c.take<uint64_t>(n);
    b.vals[0] = c.take<uint32_t>(n); b.vals[1] = c.take<uint32_t>(n);
    b.counts = c.take<uint32_t>(fqd_internal_radix_counts(n)); b.tot = c.take<uint32_t>(256);
    b.q = c.take<uint32_t>(n); b.pos = c.take<uint32_t>(n); b.nq = c.take<uint32_t>(n); b.npos = c.take<uint32_t>(n);
    b.nrid = c.take<uint32_t>(n); b.bnd_excl = c.take<uint32_t>(n); b.keep_excl = c.take<uint32_t>(n);
    b.tiles = c.take<uint32_t>(tiles); b.total = c.take<unsigned long long>(32);
    b.bnd = c.take<uint8_t>(n); b.diff = c.take<uint8_t>(n); b.mixed = c.take<uint8_t>(n); b.keep = c.take<uint8_t>(n);
    b.rank = c.take<uint8_t>(256);
    b.word = c.take<uint64_t>(n);
    *bytes = c.used + 256;
}

// excl[j] = number of set flags among f[0..j) for j < count; *total (host, may be null) = all of them (waits for the stream).
int exclusive_scan(fqd_engine* e, hipStream_t s, const uint8_t* f, uint64_t count, const SortBuffers& b, uint32_t* excl, uint32_t* total)
{
    const uint32_t tiles = uint32_t((count + kScanTile - 1) / kScanTile);
    hipLaunchKernelGGL(tile_sum_kernel, dim3(tiles), dim3(kBlock), 0, s, f, count, b.tiles);
    hipLaunchKernelGGL(fqdscan::scan_tiles_kernel<uint32_t>, dim3(1), dim3(1024), 0, s, b.tiles, tiles, b.total);
    hipLaunchKernelGGL(tile_apply_kernel, dim3(tiles), dim3(kBlock), 0, s, f, count, static_cast<const uint32_t*>(b.tiles), excl);
    FQD_TRY(e, hipGetLastError());
    if (total) {
        unsigned long long all = 0;                          // (at most count, which fits 32 bits)
        FQD_TRY(e, hipMemcpyAsync(&all, b.total, sizeof(all), hipMemcpyDeviceToHost, s));
        FQD_TRY(e, hipStreamSynchronize(s));
        *total = uint32_t(all);
    }
    return FQD_OK;
}

inline uint32_t bits_for(uint64_t v) { return v ? 64u - uint32_t(__builtin_clzll(v)) : 0u; }

bool bad_tags(const fqd_tags* t, uint64_t n)
{
    return !t || t->n != n || (n && (!t->bytes || !t->offsets || !t->lengths));
}

int run_sort(fqd_engine* e, const fqd_tags* t1, const fqd_tags* t2, uint32_t* perm)
{
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    hipStream_t s = fqd_internal_stream(e);
    const uint64_t n = t1->n;
    const Mates m{t1->bytes, t1->offsets, t1->lengths, t2 ? t2->bytes : nullptr, t2 ? t2->offsets : nullptr, t2 ? t2->lengths : nullptr};

    // 1. census
    void* small = nullptr;
    int rc = fqd_internal_scratch(e, 1, 4096, &small);
    if (rc) return rc;
    uint32_t* d_info = static_cast<uint32_t*>(small);
    uint32_t info[16] = {};
    FQD_TRY(e, hipMemsetAsync(d_info, 0, sizeof info, s));
    hipLaunchKernelGGL(census_kernel, dim3(grid_for(n, kBlock, 1024)), dim3(kBlock), 0, s, m, n, d_info);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    for (uint32_t c = 0; c < uint32_t('\n'); ++c)
        if ((info[c >> 5] >> (c & 31u)) & 1u) {
            char msg[200];
            std::snprintf(msg, sizeof msg, FQD_SEQ_LOW_BYTE_FORMAT, c);
            return fqd_internal_fail(e, FQD_ERR_ARG, msg);
        }

    // 2. the code
    uint8_t rank[256] = {};
    uint32_t K = 0;
    for (uint32_t c = 0; c < 256u; ++c) if ((info[c >> 5] >> (c & 31u)) & 1u) rank[c] = uint8_t(++K);   // K <= 246
    const uint32_t w = std::max(1u, bits_for(K)), P = 64u / w;
    const uint32_t M1 = info[8], M2 = t2 ? info[9] : 0u;
    const uint64_t T = uint64_t(M1) + M2, W = K ? (T + P - 1) / P : 0;

    SortBuffers b{};
    size_t bytes = 0;
    carve(n, b, nullptr, &bytes);
    void* base = nullptr;
    if ((rc = fqd_internal_scratch(e, 0, bytes, &base))) return rc;
    carve(n, b, static_cast<char*>(base), &bytes);
    FQD_TRY(e, hipMemcpyAsync(b.rank, rank, sizeof rank, hipMemcpyHostToDevice, s));
    const uint8_t* d_rank = b.rank;

    // 3. the sort: every record by word 0, then the mixed runs level by level
    const uint32_t npos0 = W ? uint32_t(std::min<uint64_t>(P, T)) : 0u;
    hipLaunchKernelGGL(encode_kernel, dim3(grid_for(n, kBlock, 2048)), dim3(kBlock), 0, s, m, M1, static_cast<const uint32_t*>(nullptr), n,
                       0u, npos0, w, d_rank, b.keys[0], b.vals[0], static_cast<uint64_t*>(nullptr));
    FQD_TRY(e, hipGetLastError());
    int cur = 0;
    if ((rc = fqd_internal_radix_sort(e, s, b.keys, b.vals, b.counts, b.tot, n, npos0 * w, &cur))) return rc;
    hipLaunchKernelGGL(first_list_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, static_cast<const uint64_t*>(b.keys[cur]),
                       static_cast<const uint32_t*>(b.vals[cur]), n, b.q, b.pos, b.bnd, perm);
    FQD_TRY(e, hipGetLastError());
    uint64_t count = n;
    for (uint64_t level = 1; count > 1; ++level) {
        hipLaunchKernelGGL(diff_kernel, dim3(grid_for(count)), dim3(kBlock), 0, s, m, static_cast<const uint32_t*>(b.q),
                           static_cast<const uint8_t*>(b.bnd), count, b.diff);
        if ((rc = exclusive_scan(e, s, b.bnd, count, b, b.bnd_excl, nullptr))) return rc;
        hipLaunchKernelGGL(clear_kernel, dim3(grid_for(count)), dim3(kBlock), 0, s, b.mixed, count);
        hipLaunchKernelGGL(mixed_kernel, dim3(grid_for(count)), dim3(kBlock), 0, s, static_cast<const uint8_t*>(b.diff),
                           static_cast<const uint8_t*>(b.bnd), static_cast<const uint32_t*>(b.bnd_excl), count, b.mixed);
        hipLaunchKernelGGL(keep_kernel, dim3(grid_for(count)), dim3(kBlock), 0, s, static_cast<const uint8_t*>(b.bnd),
                           static_cast<const uint32_t*>(b.bnd_excl), static_cast<const uint8_t*>(b.mixed), count, b.keep);
        uint32_t next = 0;
        if ((rc = exclusive_scan(e, s, b.keep, count, b, b.keep_excl, &next))) return rc;
        if (next == 0) break;
        // records that differ agree on every word so far, so they differ in a later one: level < W
        if (level >= W) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_sort_seqs: internal error (records differ beyond the key)");
        hipLaunchKernelGGL(compact_kernel, dim3(grid_for(count)), dim3(kBlock), 0, s, static_cast<const uint8_t*>(b.keep),
                           static_cast<const uint32_t*>(b.keep_excl), static_cast<const uint32_t*>(b.q), static_cast<const uint32_t*>(b.pos),
                           static_cast<const uint8_t*>(b.bnd), static_cast<const uint32_t*>(b.bnd_excl), count, b.nq, b.npos, b.nrid);
        const uint64_t pos0 = level * P;
        const uint32_t npos = uint32_t(std::min<uint64_t>(P, T - pos0));
        hipLaunchKernelGGL(encode_kernel, dim3(grid_for(next, kBlock, 2048)), dim3(kBlock), 0, s, m, M1, static_cast<const uint32_t*>(b.nq),
                           uint64_t(next), uint32_t(pos0), npos, w, d_rank, b.keys[0], b.vals[0], b.word);
        FQD_TRY(e, hipGetLastError());
        cur = 0;
        if ((rc = fqd_internal_radix_sort(e, s, b.keys, b.vals, b.counts, b.tot, next, npos * w, &cur))) return rc;
        uint32_t max_rid = 0;                            // runs ascend along the list: the last one is the largest
        FQD_TRY(e, hipMemcpyAsync(&max_rid, b.nrid + (next - 1), sizeof max_rid, hipMemcpyDeviceToHost, s));
        FQD_TRY(e, hipStreamSynchronize(s));
        if (bits_for(max_rid)) {
            hipLaunchKernelGGL(gather_rid_kernel, dim3(grid_for(next)), dim3(kBlock), 0, s, static_cast<const uint32_t*>(b.vals[cur]),
                               static_cast<const uint32_t*>(b.nrid), uint64_t(next), b.keys[cur]);
            if ((rc = fqd_internal_radix_sort(e, s, b.keys, b.vals, b.counts, b.tot, next, bits_for(max_rid), &cur))) return rc;
        }
        hipLaunchKernelGGL(relist_kernel, dim3(grid_for(next)), dim3(kBlock), 0, s, static_cast<const uint32_t*>(b.vals[cur]),
                           static_cast<const uint32_t*>(b.nq), static_cast<const uint32_t*>(b.npos), static_cast<const uint32_t*>(b.nrid),
                           static_cast<const uint64_t*>(b.word), uint64_t(next), b.q, b.pos, b.bnd, perm);
        FQD_TRY(e, hipGetLastError());
        count = next;
    }
    FQD_TRY(e, hipStreamSynchronize(s));                // the scratch may be reused by the next call
    return FQD_OK;
}

} // namespace

extern "C" {

int fqd_sort_seqs(fqd_engine* e, const fqd_tags* mate1, const fqd_tags* mate2, uint32_t* perm)
{
    if (!e) return FQD_ERR_ARG;
    if (!mate1 || bad_tags(mate1, mate1->n) || (mate2 && bad_tags(mate2, mate1->n)) || (mate1->n && !perm) || mate1->n >= 0x80000000ull)
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_sort_seqs: bad arguments (mates of equal count, at most 2^31-1 records)");
    if (mate1->n == 0) return FQD_OK;
    return run_sort(e, mate1, mate2, perm);
}

int fqd_seq_heads(fqd_engine* e, const fqd_tags* mate1, const fqd_tags* mate2, const uint32_t* perm, int mode, uint32_t distance,
                  uint8_t* head, uint64_t* n_heads)
{
    if (!e) return FQD_ERR_ARG;
    if (!mate1 || bad_tags(mate1, mate1->n) || (mate2 && bad_tags(mate2, mate1->n)) || (mate1->n && (!perm || !head)) ||
        mate1->n >= 0x80000000ull || mode < FQD_SEQ_TIGHT || mode > FQD_SEQ_HAMMING)
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_seq_heads: bad arguments");
    if (n_heads) *n_heads = 0;
    const uint64_t n = mate1->n;
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    hipStream_t s = fqd_internal_stream(e);
    const Mates m{mate1->bytes, mate1->offsets, mate1->lengths, mate2 ? mate2->bytes : nullptr, mate2 ? mate2->offsets : nullptr,
                  mate2 ? mate2->lengths : nullptr};
    void* base = nullptr;
    int rc = fqd_internal_scratch(e, 1, n + 512, &base);
    if (rc) return rc;
    unsigned long long* d_total = static_cast<unsigned long long*>(base);
    uint8_t* cut = static_cast<uint8_t*>(base) + 256;
    hipLaunchKernelGGL(neighbour_heads_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, m, perm, n, mode, distance,
                       mode == FQD_SEQ_HAMMING ? cut : head);
    if (mode == FQD_SEQ_HAMMING) {
        hipLaunchKernelGGL(clear_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, head, n);
        hipLaunchKernelGGL(hamming_walk_kernel, dim3(grid_for(n, 64u)), dim3(kBlock), 0, s, m, perm, n, distance,
                           static_cast<const uint8_t*>(cut), head);
    }
    FQD_TRY(e, hipMemsetAsync(d_total, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(count_kernel, dim3(grid_for(n, kBlock, 1024)), dim3(kBlock), 0, s, static_cast<const uint8_t*>(head), n, d_total);
    FQD_TRY(e, hipGetLastError());
    unsigned long long got = 0;
    FQD_TRY(e, hipMemcpyAsync(&got, d_total, sizeof got, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (n_heads) *n_heads = got;
    return FQD_OK;
}

} // extern "C"

// =====================================================================================================================
// The ranged run: prefix keys of an uploaded block, and the exact plan of the ranges (fqd_seq_range_core.hpp).
namespace {

constexpr uint32_t kKeyLanes = 8;                        // lanes per record: 8 x 8 bytes = one 64-byte line per step

// slots of the block info on the device (unsigned long long each)
enum : uint32_t { kInfoLongest1 = 0, kInfoLongest2 = 1, kInfoBytes = 2, kInfoFirstWith = 3, kInfoSlots = 13 };

// Every byte of one sequence, eight lanes to a record, 8 bytes a lane and step (the lanes of a record read one 64-byte
// line, the eight records of a wave's step lie next to each other in the block); sub 0 takes the tail.
__device__ __forceinline__ void check_sequence(const uint8_t* p, uint32_t len, uint32_t sub, uint64_t record, unsigned long long* info)
{
    for (uint32_t k = sub * 8u; k + 8u <= len; k += kKeyLanes * 8u) {
        uint64_t x;
        __builtin_memcpy(&x, p + k, 8);
        if (fqdseq::word_has_byte_below_newline(x))
            for (uint32_t j = 0; j < 8u; ++j) { const uint32_t c = uint32_t(x >> (8u * j)) & 255u; if (c < uint32_t('\n')) atomicMin(&info[kInfoFirstWith + c], (unsigned long long)record); }
    }
    if (sub == 0)
        for (uint32_t k = len & ~7u; k < len; ++k) { const uint32_t c = p[k]; if (c < uint32_t('\n')) atomicMin(&info[kInfoFirstWith + c], (unsigned long long)record); }
}

__global__ __launch_bounds__(kBlock)
void prefix_keys_kernel(Mates m, const uint32_t* __restrict__ size1, const uint32_t* __restrict__ size2, int accumulate, uint64_t n,
                        uint64_t* __restrict__ key, uint32_t* __restrict__ bytes, unsigned long long* __restrict__ info)
{
    const uint32_t sub = threadIdx.x & (kKeyLanes - 1u);
    const uint64_t group = (blockIdx.x * uint64_t(kBlock) + threadIdx.x) / kKeyLanes, groups = uint64_t(gridDim.x) * kBlock / kKeyLanes;
    uint32_t mx1 = 0, mx2 = 0;
    unsigned long long sum = 0;
    for (uint64_t i = group; i < n; i += groups) {
        const uint8_t* p1 = m.b1 + m.o1[i];
        const uint32_t l1 = m.l1[i];
        check_sequence(p1, l1, sub, i, info);
        uint32_t l2 = 0;
        if (m.b2) { l2 = m.l2[i]; check_sequence(m.b2 + m.o2[i], l2, sub, i, info); }
        if (sub == 0) {
            mx1 = max(mx1, l1); mx2 = max(mx2, l2);
            if (key) {
                uint64_t k;
                if (l1 >= fqdseq::kKeyBytes) { __builtin_memcpy(&k, p1, 8); k = __builtin_bswap64(k); }
                else k = fqdseq::prefix_key(p1, l1);
                key[i] = k;
            }
            const uint64_t sz = uint64_t(size1 ? size1[i] : 0u) + (size2 ? size2[i] : 0u);
            sum += sz;
            if (bytes) { const uint64_t all = sz + (accumulate ? bytes[i] : 0u); bytes[i] = all > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(all); }
        }
    }
    mx1 = wave_max(mx1); mx2 = wave_max(mx2); sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) {
        if (mx1) atomicMax(&info[kInfoLongest1], (unsigned long long)mx1);
        if (mx2) atomicMax(&info[kInfoLongest2], (unsigned long long)mx2);
        if (sum) atomicAdd(&info[kInfoBytes], sum);
    }
}

__global__ __launch_bounds__(kBlock)
void fill_u64_kernel(unsigned long long* __restrict__ p, uint32_t n, unsigned long long v)
{
    if (threadIdx.x < n) p[threadIdx.x] = v;
}

// ---- the plan: exclusive scan of uint32 values in 64 bits (tile sums, one block over the tiles, every element) ------------
__global__ __launch_bounds__(kBlock)
void bytes_tile_sum_kernel(const uint32_t* __restrict__ v, uint64_t n, unsigned long long* __restrict__ tile_sum)
{
    __shared__ unsigned long long ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kScanTile + uint64_t(threadIdx.x) * kScanPer;
    unsigned long long s = 0;
    for (uint32_t e = 0; e < kScanPer; ++e) s += base + e < n ? v[base + e] : 0u;
    s = fqdwave::block_total<4>(s, ws);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = s;
}

// One block: tile_sum[] becomes its exclusive scan, tile_sum[tiles] the total.
__global__ __launch_bounds__(kBlock)
void bytes_tile_scan_kernel(unsigned long long* __restrict__ tile_sum, uint64_t tiles)
{
    __shared__ unsigned long long ws[4];
    unsigned long long carry = 0;
    for (uint64_t c0 = 0; c0 < tiles; c0 += kBlock) {
        const uint64_t i = c0 + threadIdx.x;
        const unsigned long long v = i < tiles ? tile_sum[i] : 0ull;
        unsigned long long total = 0;
        const unsigned long long ex = block_exclusive<4>(v, ws, total);
        if (i < tiles) tile_sum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tile_sum[tiles] = carry;
}

__global__ __launch_bounds__(kBlock)
void bytes_tile_apply_kernel(const uint32_t* __restrict__ v, uint64_t n, const unsigned long long* __restrict__ tile_base,
                             unsigned long long* __restrict__ prefix)
{
    __shared__ unsigned long long ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kScanTile + uint64_t(threadIdx.x) * kScanPer;
    unsigned long long s = 0;
    for (uint32_t e = 0; e < kScanPer; ++e) s += base + e < n ? v[base + e] : 0u;
    unsigned long long total = 0;
    unsigned long long at = tile_base[blockIdx.x] + block_exclusive<4>(s, ws, total);
    for (uint32_t e = 0; e < kScanPer; ++e)
        if (base + e < n) { prefix[base + e] = at; at += v[base + e]; }
}

constexpr uint64_t kRow = 5;                              // uint64 words of a row of the table = fqd_seq_range

// The cuts, one after the other (each is a few binary searches from the last one: fqdseq::next_cut); one lane.  Rows of
// the table: key_lo, key_hi, pairs, bytes, bytes of mate 1 (summed later).  *n_ranges counts every range, written or not,
// up to `give_up`: a walk that gets there ends (the plan is refused).
__global__ void cut_ranges_kernel(const uint64_t* __restrict__ key, const unsigned long long* __restrict__ prefix,
                                  const unsigned long long* __restrict__ total, uint64_t n, uint64_t target,
                                  uint64_t* __restrict__ table, uint32_t max_ranges, uint32_t give_up, uint32_t* __restrict__ n_ranges)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long all = *total;
    auto key_at = [&](uint64_t i) { return key[i]; };
    auto prefix_at = [&](uint64_t i) -> uint64_t { return i < n ? prefix[i] : all; };
    uint64_t start = 0;
    uint32_t r = 0;
    while (start < n && r <= give_up) {
        const uint64_t e = fqdseq::next_cut(start, n, target, key_at, prefix_at);
        if (r < max_ranges) {
            table[kRow * r + 0] = key[start]; table[kRow * r + 1] = key[e - 1];
            table[kRow * r + 2] = e - start;  table[kRow * r + 3] = prefix_at(e) - prefix_at(start);
            table[kRow * r + 4] = 0;
        }
        ++r;
        start = e;
    }
    *n_ranges = r;
}

// The range of every pair, in input order: a range is a set of whole key values, so the pair's own key says it.  The same
// pass sums mate 1's bytes per range (row word 4): in LDS first when the ranges fit there, one add a range and block after.
constexpr uint32_t kLdsRanges = 2048;

__global__ __launch_bounds__(kBlock)
void range_of_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ bytes_mate1, uint64_t n, uint64_t* __restrict__ table,
                     uint32_t n_ranges, uint32_t* __restrict__ range_of)
{
    __shared__ unsigned long long acc[kLdsRanges];
    const bool in_lds = bytes_mate1 && n_ranges <= kLdsRanges;
    if (in_lds) { for (uint32_t r = threadIdx.x; r < n_ranges; r += kBlock) acc[r] = 0; __syncthreads(); }
    auto hi = [&](uint32_t r) { return table[kRow * r + 1]; };
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
        const uint32_t r = fqdseq::range_of_key(key[i], n_ranges, hi);
        range_of[i] = r;
        if (bytes_mate1 && r < n_ranges) {
            if (in_lds) atomicAdd(&acc[r], (unsigned long long)bytes_mate1[i]);
            else atomicAdd(reinterpret_cast<unsigned long long*>(&table[kRow * r + 4]), (unsigned long long)bytes_mate1[i]);
        }
    }
    if (in_lds) {
        __syncthreads();
        for (uint32_t r = threadIdx.x; r < n_ranges; r += kBlock)
            if (acc[r]) atomicAdd(reinterpret_cast<unsigned long long*>(&table[kRow * r + 4]), acc[r]);
    }
}

struct PlanBuffers {
    uint64_t* keys[2]; uint32_t* vals[2]; uint32_t *counts, *tot;
    unsigned long long* tiles; uint64_t* table; uint32_t* n_ranges;
};

void carve_plan(uint64_t n, uint32_t max_ranges, PlanBuffers& b, char* base, size_t* bytes)
{
    Carver c{base};
    const size_t tiles = (n + kScanTile - 1) / kScanTile + 2;
    b.keys[0] = c.take<uint64_t>(n); b.keys[1] = c.take<uint64_t>(n);
    b.vals[0] = c.take<uint32_t>(n); b.vals[1] = c.take<uint32_t>(n);
    b.counts = c.take<uint32_t>(fqd_internal_radix_counts(n)); b.tot = c.take<uint32_t>(256);
    b.tiles = c.take<unsigned long long>(tiles);
    b.table = c.take<uint64_t>(kRow * std::max<uint32_t>(max_ranges, 1u));
    b.n_ranges = c.take<uint32_t>(64);
    *bytes = c.used + 256;
}

} // namespace

extern "C" {

int fqd_seq_prefix_keys(fqd_engine* e, const fqd_tags* mate1, const fqd_tags* mate2, const uint32_t* size1, const uint32_t* size2,
                        int accumulate, uint64_t* key, uint32_t* bytes, fqd_seq_block_info* info)
{
    if (!e) return FQD_ERR_ARG;
    if (!mate1 || !info || bad_tags(mate1, mate1->n) || (mate2 && bad_tags(mate2, mate1->n)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_seq_prefix_keys: bad arguments (mates of equal count)");
    *info = fqd_seq_block_info{};
    info->bad_byte = -1;
    for (uint64_t& f : info->first_with) f = ~0ull;
    const uint64_t n = mate1->n;
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    hipStream_t s = fqd_internal_stream(e);
    void* small = nullptr;
    int rc = fqd_internal_scratch(e, 1, 4096, &small);
    if (rc) return rc;
    unsigned long long* d_info = static_cast<unsigned long long*>(small);
    FQD_TRY(e, hipMemsetAsync(d_info, 0, kInfoFirstWith * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(fill_u64_kernel, dim3(1), dim3(kBlock), 0, s, d_info + kInfoFirstWith, 10u, ~0ull);
    const Mates m{mate1->bytes, mate1->offsets, mate1->lengths, mate2 ? mate2->bytes : nullptr, mate2 ? mate2->offsets : nullptr,
                  mate2 ? mate2->lengths : nullptr};
    hipLaunchKernelGGL(prefix_keys_kernel, dim3(grid_for(n * kKeyLanes, kBlock, 4096)), dim3(kBlock), 0, s, m, size1, size2, accumulate, n,
                       key, bytes, d_info);
    FQD_TRY(e, hipGetLastError());
    unsigned long long got[kInfoSlots] = {};
    FQD_TRY(e, hipMemcpyAsync(got, d_info, sizeof got, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    info->longest[0] = uint32_t(got[kInfoLongest1]); info->longest[1] = uint32_t(got[kInfoLongest2]);
    info->record_bytes = got[kInfoBytes];
    for (uint32_t c = 0; c < 10u; ++c) {
        info->first_with[c] = got[kInfoFirstWith + c];
        if (info->bad_byte < 0 && got[kInfoFirstWith + c] != ~0ull) info->bad_byte = int32_t(c);
    }
    return FQD_OK;
}

int fqd_seq_plan_ranges(fqd_engine* e, const uint64_t* key, const uint32_t* bytes, const uint32_t* bytes_mate1, uint64_t n,
                        uint64_t target_bytes, uint32_t* range_of, fqd_seq_range* table, uint32_t max_ranges, uint32_t* n_ranges)
{
    if (!e) return FQD_ERR_ARG;
    if (!n_ranges || (max_ranges && !table) || (n && (!key || !bytes || !range_of)) || n >= 0x100000000ull)
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_seq_plan_ranges: bad arguments (at most 2^32-1 pairs)");
    *n_ranges = 0;
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    hipStream_t s = fqd_internal_stream(e);
    PlanBuffers b{};
    size_t need = 0;
    carve_plan(n, max_ranges, b, nullptr, &need);
    void* base = nullptr;
    int rc = fqd_internal_scratch(e, 0, need, &base);
    if (rc) return rc;
    carve_plan(n, max_ranges, b, static_cast<char*>(base), &need);
    FQD_TRY(e, hipMemcpyAsync(b.keys[0], key, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    FQD_TRY(e, hipMemcpyAsync(b.vals[0], bytes, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    int cur = 0;
    if ((rc = fqd_internal_radix_sort(e, s, b.keys, b.vals, b.counts, b.tot, n, 64u, &cur))) return rc;
    // the bytes before every sorted place, in 64 bits, into the key buffer the sort has left over
    const uint64_t tiles = (n + kScanTile - 1) / kScanTile;
    unsigned long long* prefix = reinterpret_cast<unsigned long long*>(b.keys[cur ^ 1]);
    hipLaunchKernelGGL(bytes_tile_sum_kernel, dim3(uint32_t(tiles)), dim3(kBlock), 0, s, static_cast<const uint32_t*>(b.vals[cur]), n, b.tiles);
    hipLaunchKernelGGL(bytes_tile_scan_kernel, dim3(1), dim3(kBlock), 0, s, b.tiles, tiles);
    hipLaunchKernelGGL(bytes_tile_apply_kernel, dim3(uint32_t(tiles)), dim3(kBlock), 0, s, static_cast<const uint32_t*>(b.vals[cur]), n,
                       static_cast<const unsigned long long*>(b.tiles), prefix);
    hipLaunchKernelGGL(cut_ranges_kernel, dim3(1), dim3(64), 0, s, static_cast<const uint64_t*>(b.keys[cur]),
                       static_cast<const unsigned long long*>(prefix), static_cast<const unsigned long long*>(b.tiles + tiles), n, target_bytes,
                       b.table, max_ranges, FQD_SEQ_MAX_RANGES, b.n_ranges);
    FQD_TRY(e, hipGetLastError());
    uint32_t R = 0;
    FQD_TRY(e, hipMemcpyAsync(&R, b.n_ranges, sizeof R, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (R > FQD_SEQ_MAX_RANGES) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "fqd_seq_plan_ranges: a target of %llu bytes cuts the input into more than %u ranges",
                      (unsigned long long)target_bytes, FQD_SEQ_MAX_RANGES);
        return fqd_internal_fail(e, FQD_ERR_ARG, msg);
    }
    *n_ranges = R;
    const uint32_t rows = std::min(R, max_ranges);
    static_assert(sizeof(fqd_seq_range) == kRow * sizeof(uint64_t), "a row of the table is kRow uint64");
    if (R <= max_ranges) {
        hipLaunchKernelGGL(range_of_kernel, dim3(grid_for(n, kBlock, 1024)), dim3(kBlock), 0, s, key, bytes_mate1, n, b.table, R, range_of);
        FQD_TRY(e, hipGetLastError());
    }
    if (rows) FQD_TRY(e, hipMemcpyAsync(table, b.table, size_t(rows) * sizeof(fqd_seq_range), hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    return FQD_OK;
}

} // extern "C"
