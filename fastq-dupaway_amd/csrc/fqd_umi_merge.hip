// fqd_umi_merge.hip — FQD_FAST_UMI_MISMATCH=1|2 of the `--fast` mode (same library as fqd_engine.hip): the exact UMI
// clusters of one sequence that differ in a base or two merged by UMI-tools' directional rule.  Rule and proofs:
// fqd_umi_merge_core.hpp.
//
//   nodes    fqd_clusters.hpp's heads phase over another flag: node_count_kernel (tile_count with "the record owns itself in
//            the exact grouping", and the checks of the owners) + scan_tiles_kernel + node_write_kernel, which is this unit's:
//            the nodes compacted in input order as (key = their owner in the grouping by sequence, value = the record).
//            The count comes back to size the rest.
//   group    fqd_internal_radix_sort over the bits of n - 1: stable, so the nodes of a sequence stand together in the order
//            of their first records.  node_pack_kernel then packs every node's B(U) at its sorted place, four bits a base
//            through the shape's table (umi_pack_kernel's gather), and fetches its count.
//   classes  classify_kernel, a lane a sorted place: a place that starts no group is done; a group of ONE node — nearly all
//            of them — is settled there with one store; a longer one is measured by a gallop over the equal keys and put
//            on the list of its size class (list_append).  A group beyond the limit is reported
//            through one 64-bit atomicMin of (first record << 32 | nodes).  The three counts come back for the grids.
//   merge    merge_lanes_kernel<8>: eight lanes a group, eight groups a wave; merge_lanes_kernel<64>: a wave a group.  A
//            lane holds its node's in-edges as a 64-bit mask and its label; a sweep reads the other lanes' labels across
//            the lanes, and the wave sweeps until a ballot says nothing changed.  merge_block_kernel: a block a group, the
//            labels in LDS, four nodes a thread, the packed UMIs and counts read through the caches; a sweep's new labels
//            wait in registers for the barrier that ends its reads.  No block waits for another.
//   spread   spread_kernel: owner_out[i] = what the node of owner_exact[i] was given.  The only writer of owner_out.
#include <hip/hip_runtime.h>

#include "fqd_clusters.hpp"
#include "fqd_owner_core.hpp"
#include "fqd_umi_merge_core.hpp"

namespace {

constexpr int kBlock = fqdscan::kBlock;
constexpr int kOffTile = fqdscan::kOffTile;                  // records a block of the scan's two passes
constexpr int kMergeBlock = 1024;                            // threads of a group's block
constexpr int kNodesPerThread = int(fqdmerge::kMaxGroup) / kMergeBlock;
constexpr unsigned long long kNoGroup = ~0ull;

static_assert(kNodesPerThread * kMergeBlock == int(fqdmerge::kMaxGroup), "a block's threads share the largest group evenly");
static_assert(fqdmerge::kWave == 64 && 64 % fqdmerge::kSmall == 0, "the lane kernels' groups tile a wave");

using fqdclusters::entry_members;
using fqdclusters::entry_place;
using fqdwave::wave_max;
using fqdwave::wave_sum;

// What the kernels count (one in scratch, zeroed per call).
struct Counters {
    unsigned long long over;                                 // the lowest (first record << 32 | nodes) of a group beyond the limit
    unsigned long long bad;                                  // records whose owner, size or sequence owner cannot be
    unsigned long long merged;                               // nodes that are not their own root
    uint32_t listed[3];                                      // groups on the small, wave and block lists
    uint32_t over_groups, largest, sweeps;
};

// ---- nodes -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void node_count_kernel(const uint32_t* __restrict__ owner_exact, const uint32_t* __restrict__ owner_seq, const uint32_t* __restrict__ size,
                       uint64_t n, unsigned long long* __restrict__ tile_sum, Counters* counters)
{
    uint32_t bad = 0;
    fqdclusters::tile_count<4>(n, tile_sum, [&](uint64_t k) __attribute__((always_inline)) {
        const uint32_t o = owner_exact[k];
        if (o == k) bad += size[k] == 0 || owner_seq[k] > k;
        else bad += o > k || owner_exact[o] != o || owner_seq[k] > k;    // (an owner is its cluster's first record: never behind it)
        return o == k;
    });
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&counters->bad, static_cast<unsigned long long>(bad));
}

__global__ __launch_bounds__(kBlock)
void node_write_kernel(const uint32_t* __restrict__ owner_exact, const uint32_t* __restrict__ owner_seq, uint64_t n, uint64_t m,
                       const unsigned long long* __restrict__ tile_start, uint64_t* __restrict__ key, uint32_t* __restrict__ val)
{
    __shared__ uint32_t ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    bool is_node[8];
    uint32_t s = 0, total;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const uint64_t k = base + uint32_t(e); is_node[e] = k < n && owner_exact[k] == k; s += is_node[e]; }
    unsigned long long at = tile_start[blockIdx.x] + fqdwave::block_exclusive<4>(s, ws, total);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint64_t k = base + uint32_t(e);
        if (is_node[e] && at < m) { key[at] = fqdowner::group_key(owner_seq[k]); val[at] = uint32_t(k); }
        at += is_node[e];
    }
}

// ---- group -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void node_pack_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ id_start, const uint32_t* __restrict__ umi_off,
                      fqdumi::Table table, uint32_t lb, uint32_t W, const uint32_t* __restrict__ first, const uint32_t* __restrict__ size,
                      uint64_t m, uint64_t* __restrict__ packed, uint32_t* __restrict__ count)
{
    for (uint64_t k = blockIdx.x * uint64_t(kBlock) + threadIdx.x; k < m; k += uint64_t(gridDim.x) * kBlock) {
        const uint32_t r = first[k];
        const uint8_t* __restrict__ U = text + id_start[r] + umi_off[r];
        for (uint32_t w = 0; w < W; ++w) packed[k * W + w] = fqdmerge::pack_word(U, table, lb, w);
        count[k] = size[r];
    }
}

// ---- classes -----------------------------------------------------------------------------------------------------------------

// The places [k, end) hold key[k]: the first place behind k with another key, by doubling steps and a bisection.
__device__ __forceinline__ uint64_t group_end(const uint64_t* __restrict__ key, uint64_t m, uint64_t k)
{
    const uint64_t K = key[k];
    uint64_t lo = k, step = 1;                                // key[lo] == K
    while (k + step < m && key[k + step] == K) { lo = k + step; step <<= 1; }
    uint64_t hi = k + step < m ? k + step : m;                // key[hi] != K, or hi == m
    while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (key[mid] == K) lo = mid; else hi = mid; }
    return hi;
}

using Lists = fqdclusters::Lists<3>;                         // the small, wave and block lists; entries (first sorted place << 32 | nodes)

__global__ __launch_bounds__(kBlock)
void classify_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ first, uint64_t m, uint32_t* __restrict__ given,
                     Lists lists, Counters* counters)
{
    const uint64_t k = blockIdx.x * uint64_t(kBlock) + threadIdx.x;     // (no stride: every lane of a wave reaches the ballots)
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t s = 0;                                          // the nodes of the group that starts here, 0: none does
    if (k < m && fqdowner::group_starts(k, k ? key[k - 1] : 0ull, key[k])) {
        if (k + 1 == m || key[k + 1] != key[k]) { s = 1; given[first[k]] = first[k]; }
        else s = uint32_t(group_end(key, m, k) - k);
    }
    const uint32_t cls = s < 2u ? 3u : s <= fqdmerge::kSmall ? 0u : s <= fqdmerge::kWave ? 1u : s <= fqdmerge::kMaxGroup ? 2u : 4u;
    fqdclusters::list_append(lists, counters->listed, cls, uint32_t(k), s);   // (k < m < 2^31)
    if (cls == 4u) { atomicMin(&counters->over, (static_cast<unsigned long long>(first[k]) << 32) | s); atomicAdd(&counters->over_groups, 1u); }
    const uint32_t largest = wave_max(s);
    if (lane == 0 && largest > 1u) atomicMax(&counters->largest, largest);
}

// ---- merge -------------------------------------------------------------------------------------------------------------------

// G lanes a group (8 or 64), a lane a node; see the head of the file.
template <uint32_t G>
__global__ __launch_bounds__(kBlock)
void merge_lanes_kernel(const unsigned long long* __restrict__ list, uint32_t n_items, const uint64_t* __restrict__ packed,
                        const uint32_t* __restrict__ count, const uint32_t* __restrict__ first, uint32_t W, uint32_t D,
                        uint32_t* __restrict__ given, Counters* counters)
{
    const uint32_t lane = threadIdx.x & 63u, gl = lane % G;
    const uint64_t item = (blockIdx.x * uint64_t(kBlock) + threadIdx.x) / G;
    uint32_t s = 0;
    uint64_t k0 = 0;
    if (item < n_items) { const unsigned long long e = list[item]; k0 = entry_place(e); s = entry_members(e); }
    if (s > G) s = 0;                                        // (no list holds such an entry)
    const bool live = gl < s;
    const uint64_t* __restrict__ P = packed + k0 * W;
    const uint32_t* __restrict__ C = count + k0;
    const uint64_t in_edges = live ? fqdmerge::lane_in_edges(P, C, s, W, D, gl) : 0ull;
    unsigned long long label = live ? fqdmerge::label_of(C[gl], gl) : ~0ull;
    // every lane of the wave asks the same places: the group's nodes where a wave holds one group, all G where it holds several
    const uint32_t s_all = G == 64u ? uint32_t(__builtin_amdgcn_readfirstlane(int(s))) : G;
    uint32_t sweeps = 0;
    for (uint32_t t = 1; t <= G; ++t) {                      // (a group of s nodes is through after s - 1 sweeps that change a label)
        const unsigned long long old = label;
        label = fqdmerge::lane_sweep(in_edges, old, s_all, [&](uint32_t u) { return __shfl(old, int(u), int(G)); });
        const bool changed = label != old;
        if (changed) sweeps = t;
        if (!__any(changed)) break;
    }
    const unsigned long long ended = label;
    const uint32_t lowest = fqdmerge::lane_first_of_root(ended, s_all, [&](uint32_t u) { return __shfl(ended, int(u), int(G)); });
    if (live && lowest < s) given[first[k0 + gl]] = first[k0 + lowest];
    const uint32_t merged = uint32_t(__popcll(__ballot(live && fqdmerge::label_pos(ended) != gl)));
    sweeps = wave_max(sweeps);
    if (lane == 0) {
        if (merged) atomicAdd(&counters->merged, static_cast<unsigned long long>(merged));
        if (sweeps) atomicMax(&counters->sweeps, sweeps);
    }
}

// A block a group of up to kMaxGroup nodes; see the head of the file.
__global__ __launch_bounds__(kMergeBlock)
void merge_block_kernel(const unsigned long long* __restrict__ list, const uint64_t* __restrict__ packed, const uint32_t* __restrict__ count,
                        const uint32_t* __restrict__ first, uint32_t W, uint32_t D, uint32_t* __restrict__ given, Counters* counters)
{
    __shared__ unsigned long long labels[fqdmerge::kMaxGroup];
    __shared__ uint32_t lowest[fqdmerge::kMaxGroup];         // per root: the lowest place of its cluster
    const unsigned long long e = list[blockIdx.x];
    const uint64_t k0 = entry_place(e);
    uint32_t s = entry_members(e);
    if (s > fqdmerge::kMaxGroup) s = 0;                      // (no list holds such an entry)
    const uint64_t* __restrict__ P = packed + k0 * W;
    const uint32_t* __restrict__ C = count + k0;
    for (uint32_t v = threadIdx.x; v < s; v += kMergeBlock) { labels[v] = fqdmerge::label_of(C[v], v); lowest[v] = fqdmerge::kNoPos; }
    __syncthreads();
    uint32_t sweeps = 0;
    for (uint32_t t = 0; t < s; ++t) {
        unsigned long long next[kNodesPerThread];
        bool changed = false;
#pragma unroll
        for (int j = 0; j < kNodesPerThread; ++j) {
            const uint32_t v = threadIdx.x + uint32_t(j) * kMergeBlock;
            next[j] = 0;
            if (v < s) { next[j] = fqdmerge::block_sweep(P, C, reinterpret_cast<const uint64_t*>(labels), s, W, D, v); changed |= next[j] != labels[v]; }
        }
        if (!__syncthreads_or(changed)) break;               // (the barrier ends the sweep's reads)
#pragma unroll
        for (int j = 0; j < kNodesPerThread; ++j) { const uint32_t v = threadIdx.x + uint32_t(j) * kMergeBlock; if (v < s) labels[v] = next[j]; }
        ++sweeps;
        __syncthreads();
    }
    for (uint32_t v = threadIdx.x; v < s; v += kMergeBlock) atomicMin(&lowest[fqdmerge::label_pos(labels[v])], v);
    __syncthreads();
    uint32_t merged = 0;
    for (uint32_t v = threadIdx.x; v < s; v += kMergeBlock) {
        const uint32_t root = fqdmerge::label_pos(labels[v]);
        given[first[k0 + v]] = first[k0 + lowest[root]];
        merged += root != v;
    }
    merged = wave_sum(merged);
    if ((threadIdx.x & 63) == 0 && merged) atomicAdd(&counters->merged, static_cast<unsigned long long>(merged));
    if (threadIdx.x == 0 && sweeps) atomicMax(&counters->sweeps, sweeps);
}

// ---- spread ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void spread_kernel(const uint32_t* __restrict__ owner_exact, const uint32_t* __restrict__ given, uint64_t n, uint32_t* __restrict__ owner_out)
{
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock)
        owner_out[i] = given[owner_exact[i]];                // (owner_exact[i] <= i: node_count_kernel has seen to it)
}

__global__ __launch_bounds__(kBlock)
void owners_to_keep_kernel(const uint32_t* __restrict__ owner, uint64_t n, uint8_t* __restrict__ keep)
{
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) keep[i] = owner[i] == i ? 1 : 0;
}

struct MergeBuffers {
    uint64_t* keys[2]; uint32_t* vals[2]; uint32_t *counts, *tot;
    uint64_t* packed; uint32_t* count; uint32_t* given; Lists lists;
};

size_t carve_merge(uint64_t n, uint64_t m, uint32_t W, char* base, MergeBuffers& b)
{
    Carver c{base};
    b.keys[0] = c.take<uint64_t>(m); b.keys[1] = c.take<uint64_t>(m);
    b.vals[0] = c.take<uint32_t>(m); b.vals[1] = c.take<uint32_t>(m);
    b.counts = c.take<uint32_t>(fqd_internal_radix_counts(m)); b.tot = c.take<uint32_t>(256);
    b.packed = c.take<uint64_t>(m * W); b.count = c.take<uint32_t>(m); b.given = c.take<uint32_t>(n);
    fqdclusters::take_lists(c, m, {1u, fqdmerge::kSmall, fqdmerge::kWave}, b.lists);   // (groups among the m nodes)
    return c.used + 256;
}

} // namespace

extern "C" {

int fqd_umi_merge(fqd_engine* e, const uint8_t* text, const uint64_t* id_start, const uint32_t* umi_off, const fqd_umi_info* info,
                  const uint32_t* owner_exact, const uint32_t* owner_seq, const uint32_t* size, uint64_t n, uint32_t distance,
                  uint32_t* owner_out, fqd_umi_merge_info* out)
{
    if (!e) return FQD_ERR_ARG;
    if (out) *out = fqd_umi_merge_info{0, 0, 0, 0, 0, FQD_UMI_MERGE_MAX_GROUP, 0, FQD_UMI_NO_RECORD, {0, 0, 0, 0}};
    if (!out || !info || (distance != 1 && distance != 2) || n >= 0x80000000ull ||
        (n && (!text || !id_start || !umi_off || !owner_exact || !owner_seq || !size || !owner_out)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_merge: bad arguments (the info of the find and of the merge, a distance of 1 or 2, the text, and the ID lines' starts, the UMI offsets, the two owners, the sizes and room for the owners of at most 2^31-1 records)");
    if (info->bad_record != FQD_UMI_NO_RECORD || info->umi_len == 0 || info->umi_len > fqdumi::kMaxUmi ||
        (info->umi_len < 64 && (info->joiners >> info->umi_len)) || info->n_bases == 0 ||
        info->n_bases != info->umi_len - uint32_t(__builtin_popcountll(info->joiners)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_merge: info is not what fqd_umi_find leaves for records it does not refuse");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(text, id_start, umi_off, owner_exact, owner_seq, size, owner_out))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_merge: the text and every array are device memory");
    hipStream_t stream = fqd_internal_stream(e);
    fqdumi::Table table;
    const uint32_t lb = fqdumi::bases_table(info->umi_len, info->joiners, &table), W = fqdmerge::words(lb);
    StageTimer timer{out->stage_ms};

    // ---- nodes ----
    TileScratch<Counters> slot;
    int rc = slot.reserve(e, fqdclusters::tiles_of(n), stream, &Counters::over);
    if (rc) return rc;
    Counters* counters = slot.counters;
    unsigned long long m = 0;
    Counters got{};
    bool fits = false;
    rc = fqdclusters::count_heads(e, stream, slot, n, [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(node_count_kernel, grid, block, 0, stream, owner_exact, owner_seq, size, n, slot.tile_sum, counters);
    }, &m, &got, &fits);
    if (rc) return rc;
    if (got.bad || !fits)
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_merge: an owner that stands behind its record, or a record that owns itself with size 0 (are owner_exact, owner_seq and size those of fqd_owners and fqd_cluster_sizes over these records? nothing was written)");
    out->nodes = m;
    timer.mark(0);

    // ---- group ----
    MergeBuffers b{};
    void* base = nullptr;
    if ((rc = fqd_internal_scratch(e, 0, carve_merge(n, m, W, nullptr, b), &base))) return rc;
    (void)carve_merge(n, m, W, static_cast<char*>(base), b);
    hipLaunchKernelGGL(node_write_kernel, dim3(slot.tiles), dim3(kBlock), 0, stream, owner_exact, owner_seq, n, uint64_t(m),
                       static_cast<const unsigned long long*>(slot.tile_sum), b.keys[0], b.vals[0]);
    int cur = 0;
    if ((rc = fqd_internal_radix_sort(e, stream, b.keys, b.vals, b.counts, b.tot, m, fqdowner::group_bits(n), &cur))) return rc;
    const uint64_t* key = b.keys[cur];
    const uint32_t* first = b.vals[cur];
    hipLaunchKernelGGL(node_pack_kernel, dim3(grid_for(m, kBlock, 8192)), dim3(kBlock), 0, stream, text, id_start, umi_off, table, lb, W,
                       first, size, uint64_t(m), b.packed, b.count);

    // ---- classes ----
    hipLaunchKernelGGL(classify_kernel, dim3(uint32_t((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, key, first, uint64_t(m), b.given,
                       b.lists, counters);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, read_back(got, counters, stream));
    out->groups = uint64_t(got.listed[0]) + got.listed[1] + got.listed[2] + got.over_groups;
    out->largest = got.largest ? got.largest : 1u;
    timer.mark(1);
    if (got.over != kNoGroup) {                               // refused: owner_out stays as it is
        out->over_limit_first = got.over >> 32;
        out->over_limit_nodes = uint32_t(got.over);
        return FQD_OK;
    }

    // ---- merge, spread ----
    const uint32_t D = distance;
    if (got.listed[0])
        hipLaunchKernelGGL(merge_lanes_kernel<fqdmerge::kSmall>, dim3(uint32_t((uint64_t(got.listed[0]) * fqdmerge::kSmall + kBlock - 1) / kBlock)), dim3(kBlock),
                           0, stream, static_cast<const unsigned long long*>(b.lists.of[0]), got.listed[0], static_cast<const uint64_t*>(b.packed),
                           static_cast<const uint32_t*>(b.count), first, W, D, b.given, counters);
    if (got.listed[1])
        hipLaunchKernelGGL(merge_lanes_kernel<fqdmerge::kWave>, dim3(uint32_t((uint64_t(got.listed[1]) * fqdmerge::kWave + kBlock - 1) / kBlock)), dim3(kBlock),
                           0, stream, static_cast<const unsigned long long*>(b.lists.of[1]), got.listed[1], static_cast<const uint64_t*>(b.packed),
                           static_cast<const uint32_t*>(b.count), first, W, D, b.given, counters);
    if (got.listed[2])
        hipLaunchKernelGGL(merge_block_kernel, dim3(got.listed[2]), dim3(kMergeBlock), 0, stream, static_cast<const unsigned long long*>(b.lists.of[2]),
                           static_cast<const uint64_t*>(b.packed), static_cast<const uint32_t*>(b.count), first, W, D, b.given, counters);
    hipLaunchKernelGGL(spread_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, stream, owner_exact, static_cast<const uint32_t*>(b.given), n, owner_out);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, read_back(got, counters, stream));
    out->merged = got.merged;
    out->sweeps = got.sweeps;
    timer.mark(2);
    return FQD_OK;
}

int fqd_owners_to_keep(fqd_engine* e, const uint32_t* owner, uint64_t n, uint8_t* keep)
{
    if (!e) return FQD_ERR_ARG;
    if (n >= 0x100000000ull || (n && (!owner || !keep)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_owners_to_keep: bad arguments (the owners and room for the keep flags of at most 2^32-1 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(owner, keep)) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_owners_to_keep: owner and keep are device memory");
    hipLaunchKernelGGL(owners_to_keep_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, fqd_internal_stream(e), owner, n, keep);
    FQD_TRY(e, hipGetLastError());
    return FQD_OK;
}

} // extern "C"
