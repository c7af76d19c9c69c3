// fqd_centroid.hip — FQD_FAST_CENTROID=abundant of the `--fast` mode (same library as fqd_engine.hip): every record's
// abundance — the weight of the members of its cluster that share its exact key — so that fqd_seq_pick_best over it puts the
// first copy of the cluster's most abundant sequence at the head's place, and the scores masked to that sequence's copies for
// FQD_FAST_KEEP=best.  Rule and proofs: fqd_centroid_core.hpp.  Nothing in here is called unless the switch is set.
//
//   heads    fqd_clusters.hpp's: head_count_kernel (tile_count; its own part is what ends the call: a record of the order
//            or a label outside 0 .. n-1, and place 0 without a head) + scan_tiles_kernel + head_write_kernel.
//   classes  classify_kernel, a lane a cluster (cluster_at): a cluster of ONE member — most of them — is only counted;
//            a longer one goes on the list of its size class (list_append).
//   sums     singles_kernel: a lane a cluster of one, the abundance is the weight.  small_kernel: eight lanes a cluster,
//            eight clusters a wave, a lane sums the weights of the lanes of its group that hold its label.  wave_kernel: a
//            wave a cluster; the loop runs once per DISTINCT label — the lowest open lane's label is read across the wave
//            (v_readlane with the ballot's lowest bit: every lane is in the loop, so that is readfirstlane's lane without its
//            dependence on the branch), the lanes that hold it are found by ballot and their weights summed in 64 bits.
//            block_kernel: a workgroup a cluster of up to kBlockLimit, its labels in an open-addressing table in LDS that the
//            block clears itself (as many slots as the cluster needs), sums by 64-bit LDS atomics, the members' slots kept
//            in registers for the second pass.  The large tier, without a limit: many blocks a cluster, a table in scratch
//            keyed (head place << 32 | label) of twice the tier's members, inserted by 64-bit compare-and-swap and summed by
//            64-bit atomic add (large_add_kernel; a wave whose lanes all hold one key — the cluster of a million identical
//            reads — sums across its lanes first and adds once), looked up by a second launch (large_store_kernel).
//            Every kernel stores the abundance of its own clusters' members, each entry once.
//   masked   fqd_subcluster_scores: a max-scan of "the last head at or in front of this place" in three launches
//            (last_head_tiles_kernel, last_head_carry_kernel, masked_scores_kernel), and a gather of the head's label.
#include <hip/hip_runtime.h>

#include "fqd_centroid_core.hpp"
#include "fqd_clusters.hpp"

namespace {

using namespace fqdcentroid;

constexpr int kBlock = fqdscan::kBlock;
constexpr int kOffTile = fqdscan::kOffTile;                  // places a block of the scans' passes
constexpr int kTableBlock = 512;                             // threads of a cluster's block
constexpr int kPerThread = int(kBlockLimit) / kTableBlock;
constexpr uint32_t kLargeMaxX = 1024, kLargeBlocks = 16384;  // blocks a cluster at most, blocks a launch (about)

static_assert(kPerThread * kTableBlock == int(kBlockLimit), "a block's threads share the largest cluster in LDS evenly");
static_assert(64 % kSmall == 0 && kWave == 64, "the lane kernels' groups tile a wave");
static_assert(kBlockTableBytes + 64 <= 64 * 1024, "the table and the block's counter fit a workgroup's static LDS");

using fqdclusters::cluster_at;
using fqdclusters::entry_members;
using fqdclusters::entry_place;
using fqdwave::wave_max;
using fqdwave::wave_sum;

// ---- heads -------------------------------------------------------------------------------------------------------------------

// What ends a call (in scratch beside the tile sums, zeroed per call).
struct Checks { unsigned long long bad; };                   // places whose record, records whose label lies outside 0 .. n-1; place 0 without a head

// What the kernels count (in scratch in front of the lists, zeroed per call).
struct Counters {
    unsigned long long mixed, subclusters;                   // of the listed clusters
    unsigned long long large_members;                        // the members of the large tier's clusters
    uint32_t listed[4];                                      // clusters on the small, wave, block and large lists
    uint32_t singles, largest;
};

__global__ __launch_bounds__(kBlock)
void head_count_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ head, const uint32_t* __restrict__ label, uint64_t n,
                       unsigned long long* __restrict__ tile_sum, Checks* checks)
{
    uint32_t bad = 0;
    fqdclusters::tile_count<4>(n, tile_sum, [&](uint64_t k) __attribute__((always_inline)) {
        const bool h = head[k] != 0;
        bad += perm[k] >= n || (k == 0 && !h) || label[k] >= n;
        return h;
    });
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&checks->bad, static_cast<unsigned long long>(bad));
}

// ---- classes -----------------------------------------------------------------------------------------------------------------

using Lists = fqdclusters::Lists<4>;                         // the small, wave, block and large lists

__global__ __launch_bounds__(kBlock)
void classify_kernel(const uint32_t* __restrict__ head_place, uint64_t m, uint64_t n, Lists lists, Counters* counters)
{
    const uint64_t c = blockIdx.x * uint64_t(kBlock) + threadIdx.x;     // (no stride: every lane of a wave reaches the ballots)
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t s = 0, k0 = 0;
    if (c < m) s = cluster_at(head_place, m, n, c, &k0);
    const uint32_t tier = s == 0u ? 5u : tier_of(s);
    fqdclusters::list_append(lists, counters->listed, tier - 1u, k0, s);   // (tier 0, one member, and tier 5, none: on no list)
    const uint32_t singles = uint32_t(__popcll(__ballot(tier == kTierOne)));
    const unsigned long long large = wave_sum(tier == kTierLarge ? static_cast<unsigned long long>(s) : 0ull);
    const uint32_t largest = wave_max(s);
    if (lane == 0) {
        if (singles) atomicAdd(&counters->singles, singles);
        if (large) atomicAdd(&counters->large_members, large);
        if (largest) atomicMax(&counters->largest, largest);
    }
}

// ---- sums --------------------------------------------------------------------------------------------------------------------

struct Members { const uint32_t *perm, *label, *weight; };   // weight: nullptr for 1 each

__device__ __forceinline__ uint32_t weight_of(const Members& mb, uint32_t rec) { return mb.weight ? mb.weight[rec] : 1u; }

__global__ __launch_bounds__(kBlock)
void singles_kernel(const uint32_t* __restrict__ head_place, Members mb, uint64_t m, uint64_t n, uint32_t* __restrict__ abundance)
{
    for (uint64_t c = blockIdx.x * uint64_t(kBlock) + threadIdx.x; c < m; c += uint64_t(gridDim.x) * kBlock) {
        uint32_t k0;
        if (cluster_at(head_place, m, n, c, &k0) == 1u) { const uint32_t r = mb.perm[k0]; abundance[r] = weight_of(mb, r); }
    }
}

// Eight lanes a cluster, a lane a member; see the head of the file.
__global__ __launch_bounds__(kBlock)
void small_kernel(const unsigned long long* __restrict__ list, uint32_t n_items, Members mb, uint32_t* __restrict__ abundance, Counters* counters)
{
    constexpr uint32_t G = kSmall;
    const uint32_t lane = threadIdx.x & 63u, gl = lane % G;
    const uint64_t item = (blockIdx.x * uint64_t(kBlock) + threadIdx.x) / G;
    uint32_t s = 0;
    uint64_t k0 = 0;
    if (item < n_items) { const unsigned long long e = list[item]; k0 = entry_place(e); s = entry_members(e); }
    if (s > G) s = 0;                                        // (no list holds such an entry)
    const bool live = gl < s;
    uint32_t rec = 0, lab = kNoLabel, w = 0;
    if (live) { rec = mb.perm[k0 + gl]; lab = mb.label[rec]; w = weight_of(mb, rec); }
    unsigned long long sum = 0;
    bool first = true;                                       // no member in front of this one holds its label
#pragma unroll
    for (uint32_t u = 0; u < G; ++u) {
        const uint32_t lu = __shfl(lab, int(u), int(G)), wu = __shfl(w, int(u), int(G));
        if (u < s && lu == lab) { sum += wu; first &= u >= gl; }
    }
    if (live) abundance[rec] = saturate(sum);
    const uint32_t subs = uint32_t(__popcll(__ballot(live && first)));
    const uint32_t second = fqdwave::group_or<int(G)>(uint32_t(live && first && gl != 0u));   // a member behind the first starts a sub-cluster
    const uint32_t mixed = uint32_t(__popcll(__ballot(live && gl == 0u && second != 0u)));
    if (lane == 0) {
        if (subs) atomicAdd(&counters->subclusters, static_cast<unsigned long long>(subs));
        if (mixed) atomicAdd(&counters->mixed, static_cast<unsigned long long>(mixed));
    }
}

// A wave a cluster of up to 64, a lane a member; see the head of the file.
__global__ __launch_bounds__(kBlock)
void wave_kernel(const unsigned long long* __restrict__ list, uint32_t n_items, Members mb, uint32_t* __restrict__ abundance, Counters* counters)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = (blockIdx.x * uint64_t(kBlock) + threadIdx.x) / kWave;
    uint32_t s = 0;
    uint64_t k0 = 0;
    if (item < n_items) { const unsigned long long e = list[item]; k0 = entry_place(e); s = entry_members(e); }
    if (s > kWave) s = 0;                                    // (no list holds such an entry)
    const bool live = lane < s;
    uint32_t rec = 0, lab = kNoLabel, w = 0;
    if (live) { rec = mb.perm[k0 + lane]; lab = mb.label[rec]; w = weight_of(mb, rec); }
    unsigned long long sum = 0, open = __ballot(live);       // open: the lanes whose label has not been summed (the same in every lane)
    uint32_t subs = 0;
    while (open) {                                           // (the whole wave, once per distinct label)
        const uint32_t cur = uint32_t(__builtin_amdgcn_readlane(int(lab), __ffsll(open) - 1));
        const bool match = live && lab == cur;
        unsigned long long part = wave_sum(match ? static_cast<unsigned long long>(w) : 0ull);
        part = __shfl(part, 0, 64);
        if (match) sum = part;
        open &= ~__ballot(match);
        ++subs;
    }
    if (live) abundance[rec] = saturate(sum);
    if (lane == 0 && subs) {
        atomicAdd(&counters->subclusters, static_cast<unsigned long long>(subs));
        if (subs > 1u) atomicAdd(&counters->mixed, 1ull);
    }
}

// A block a cluster of up to kBlockLimit members; see the head of the file.
__global__ __launch_bounds__(kTableBlock)
void block_kernel(const unsigned long long* __restrict__ list, Members mb, uint32_t* __restrict__ abundance, Counters* counters)
{
    __shared__ unsigned long long sums[kBlockSlots];
    __shared__ uint32_t keys[kBlockSlots];
    __shared__ uint32_t distinct;
    const unsigned long long e = list[blockIdx.x];
    const uint64_t k0 = entry_place(e);
    uint32_t s = entry_members(e);
    if (s > kBlockLimit) s = 0;                              // (no list holds such an entry)
    const uint32_t slots = block_slots(s);
    for (uint32_t t = threadIdx.x; t < slots; t += kTableBlock) { keys[t] = kNoLabel; sums[t] = 0ull; }
    if (threadIdx.x == 0) distinct = 0;
    __syncthreads();
    uint32_t rec[kPerThread], at[kPerThread], fresh = 0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const uint32_t v = threadIdx.x + uint32_t(j) * kTableBlock;
        rec[j] = 0; at[j] = 0;
        if (v >= s) continue;
        rec[j] = mb.perm[k0 + v];
        const uint32_t lab = mb.label[rec[j]];
        uint32_t slot = block_slot(lab, slots);
        for (;;) {                                           // (at most half of the slots are taken: an empty one ends every probe)
            const uint32_t was = atomicCAS(&keys[slot], kNoLabel, lab);
            if (was == kNoLabel || was == lab) { fresh += was == kNoLabel; break; }
            slot = uint32_t(next_slot(slot, slots));
        }
        atomicAdd(&sums[slot], static_cast<unsigned long long>(weight_of(mb, rec[j])));
        at[j] = slot;
    }
    fresh = wave_sum(fresh);
    if ((threadIdx.x & 63) == 0 && fresh) atomicAdd(&distinct, fresh);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const uint32_t v = threadIdx.x + uint32_t(j) * kTableBlock;
        if (v < s) abundance[rec[j]] = saturate(sums[at[j]]);
    }
    if (threadIdx.x == 0 && distinct) {
        atomicAdd(&counters->subclusters, static_cast<unsigned long long>(distinct));
        if (distinct > 1u) atomicAdd(&counters->mixed, 1ull);
    }
}

// ---- the large tier: blockIdx.y strides over the clusters, blockIdx.x over a cluster's chunks of kBlock members ---------------

struct Table { unsigned long long *keys, *sums; uint64_t slots; uint32_t* distinct; };   // distinct: a word a cluster

__device__ __forceinline__ void table_add(const Table& t, uint32_t item, unsigned long long key, unsigned long long w)
{
    uint64_t slot = scratch_slot(key, t.slots);
    for (;;) {                                               // (at most half of the slots are taken: an empty one ends every probe)
        const unsigned long long was = atomicCAS(&t.keys[slot], static_cast<unsigned long long>(kNoKey), key);
        if (was == kNoKey) atomicAdd(&t.distinct[item], 1u);
        if (was == kNoKey || was == key) break;
        slot = next_slot(slot, t.slots);
    }
    atomicAdd(&t.sums[slot], w);
}

__global__ __launch_bounds__(kBlock)
void large_add_kernel(const unsigned long long* __restrict__ list, uint32_t n_items, Members mb, Table t)
{
    for (uint32_t item = blockIdx.y; item < n_items; item += gridDim.y) {
        const unsigned long long e = list[item];
        const uint32_t k0 = uint32_t(entry_place(e)), s = entry_members(e);
        for (uint64_t v0 = uint64_t(blockIdx.x) * kBlock; v0 < s; v0 += uint64_t(gridDim.x) * kBlock) {   // (the whole block)
            const uint64_t v = v0 + threadIdx.x;
            const bool live = v < s;
            unsigned long long key = kNoKey, w = 0;
            if (live) { const uint32_t rec = mb.perm[uint64_t(k0) + v]; key = pack_key(k0, mb.label[rec]); w = weight_of(mb, rec); }
            // the live lanes of a wave are its lowest: lane 0 is live where any is
            const unsigned long long key0 = __shfl(key, 0, 64);
            const bool one_key = __ballot(live && key != key0) == 0ull;
            if (one_key) {
                const unsigned long long total = wave_sum(w);
                if ((threadIdx.x & 63) == 0 && live) table_add(t, item, key0, total);
            } else if (live) table_add(t, item, key, w);
        }
    }
}

__global__ __launch_bounds__(kBlock)
void large_store_kernel(const unsigned long long* __restrict__ list, uint32_t n_items, Members mb, Table t, uint32_t* __restrict__ abundance,
                        Counters* counters)
{
    for (uint32_t item = blockIdx.y; item < n_items; item += gridDim.y) {
        const unsigned long long e = list[item];
        const uint32_t k0 = uint32_t(entry_place(e)), s = entry_members(e);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const uint32_t d = t.distinct[item];
            atomicAdd(&counters->subclusters, static_cast<unsigned long long>(d));
            if (d > 1u) atomicAdd(&counters->mixed, 1ull);
        }
        for (uint64_t v = uint64_t(blockIdx.x) * kBlock + threadIdx.x; v < s; v += uint64_t(gridDim.x) * kBlock) {
            const uint32_t rec = mb.perm[uint64_t(k0) + v];
            const unsigned long long key = pack_key(k0, mb.label[rec]);
            uint64_t slot = scratch_slot(key, t.slots);
            // (the key went in with the launch before this one; the bound is for a table that another call's arguments made)
            for (uint64_t tries = 0; t.keys[slot] != key && tries < t.slots; ++tries) slot = next_slot(slot, t.slots);
            abundance[rec] = saturate(t.sums[slot]);
        }
    }
}

// ---- masked scores -------------------------------------------------------------------------------------------------------------

// Maxima of (place + 1) over the head places: 0 is "none in front".
__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t v)
{
    const int l = int(threadIdx.x & 63u);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(v, d, 64); if (l >= d && up > v) v = up; }
    return v;
}

// The maximum over the threads in front of this one in the block (ws: kWaves words), and the block's in `total`.
template <int kWaves>
__device__ __forceinline__ uint32_t block_exclusive_max(uint32_t v, uint32_t* ws, uint32_t& total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_max(v);
    if (lane == 63u) ws[wave] = inc;
    uint32_t before = __shfl_up(inc, 1, 64);                 // (there is no taking v out of a maximum again)
    if (lane == 0u) before = 0;
    __syncthreads();
    total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) { const uint32_t c = ws[k]; if (uint32_t(k) < wave && c > before) before = c; if (c > total) total = c; }
    __syncthreads();
    return before;
}

// The thread's eight places from base on: 1 + the last head place among them (0: none); also the checks of the call.
__device__ __forceinline__ uint32_t last_head_of_eight(const uint8_t* __restrict__ head, uint64_t n, uint64_t base)
{
    uint32_t last = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const uint64_t k = base + uint32_t(e); if (k < n && head[k] != 0) last = uint32_t(k) + 1u; }
    return last;
}

__global__ __launch_bounds__(kBlock)
void last_head_tiles_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ head, uint64_t n, uint32_t* __restrict__ tile_last, Checks* checks)
{
    __shared__ uint32_t ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    uint32_t bad = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const uint64_t k = base + uint32_t(e); if (k < n) bad += perm[k] >= n || (k == 0 && head[k] == 0); }
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&checks->bad, static_cast<unsigned long long>(bad));
    uint32_t total;
    (void)block_exclusive_max<4>(last_head_of_eight(head, n, base), ws, total);
    if (threadIdx.x == 0) tile_last[blockIdx.x] = total;
}

// One block: every tile's value becomes the maximum of the tiles in front of it.
__global__ __launch_bounds__(1024)
void last_head_carry_kernel(uint32_t* __restrict__ tile_last, uint32_t tiles)
{
    __shared__ uint32_t ws[16];
    uint32_t carry = 0;                                      // (the same in every thread)
    for (uint32_t t0 = 0; t0 < tiles; t0 += 1024u) {
        const uint32_t i = t0 + threadIdx.x;
        uint32_t total;
        const uint32_t before = block_exclusive_max<16>(i < tiles ? tile_last[i] : 0u, ws, total);
        if (i < tiles) tile_last[i] = before > carry ? before : carry;
        if (total > carry) carry = total;
    }
}

__global__ __launch_bounds__(kBlock)
void masked_scores_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ head, const uint32_t* __restrict__ label,
                          const uint32_t* __restrict__ score, uint64_t n, const uint32_t* __restrict__ tile_last, uint32_t* __restrict__ masked)
{
    __shared__ uint32_t ws[4];
    const uint64_t base = uint64_t(blockIdx.x) * kOffTile + uint64_t(threadIdx.x) * 8u;
    uint32_t total;
    uint32_t cur = block_exclusive_max<4>(last_head_of_eight(head, n, base), ws, total);
    const uint32_t carried = tile_last[blockIdx.x];
    if (carried > cur) cur = carried;
    uint32_t head_label = cur ? label[perm[cur - 1u]] : kNoLabel;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint64_t k = base + uint32_t(e);
        if (k >= n) break;
        const uint32_t rec = perm[k];
        const uint32_t lab = label[rec];
        if (head[k] != 0) head_label = lab;                  // (place 0 is a head: head_label is a label wherever it is compared)
        masked[rec] = masked_score(score[rec], lab == head_label);
    }
}

struct SumBuffers { Counters* counters; uint32_t* head_place; Lists lists; };

size_t carve_sums(uint64_t n, uint64_t m, char* base, SumBuffers& b)
{
    Carver c{base};
    b.counters = c.take<Counters>(1);
    b.head_place = c.take<uint32_t>(m);
    fqdclusters::take_lists(c, n, {1u, kSmall, kWave, kBlockLimit}, b.lists);
    return c.used + 256;
}

size_t carve_table(uint64_t members, uint32_t items, char* base, Table& t)
{
    Carver c{base};
    t.slots = scratch_slots(members);
    t.keys = c.take<unsigned long long>(t.slots); t.sums = c.take<unsigned long long>(t.slots); t.distinct = c.take<uint32_t>(items);
    return c.used + 256;
}

} // namespace

extern "C" {

int fqd_subcluster_sizes(fqd_engine* e, const uint32_t* perm, const uint8_t* head, const uint32_t* label, const uint32_t* weight, uint64_t n,
                         uint32_t* abundance, fqd_centroid_info* info)
{
    if (!e) return FQD_ERR_ARG;
    if (info) *info = fqd_centroid_info{0, 0, 0, {0, 0, 0, 0, 0}, 0, 0};
    if (n >= 0x80000000ull || (n && (!perm || !head || !label || !abundance)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_subcluster_sizes: bad arguments (the order and its head flags, the exact owners, and room for the abundances of at most 2^31-1 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(perm, head, label, abundance) || (weight && !on_device(weight)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_subcluster_sizes: every array is device memory");
    const size_t words = size_t(n) * sizeof(uint32_t);
    if (overlap(abundance, words, perm, words) || overlap(abundance, words, head, size_t(n)) || overlap(abundance, words, label, words) ||
        overlap(abundance, words, weight, words))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_subcluster_sizes: abundance overlaps an input");
    hipStream_t stream = fqd_internal_stream(e);

    // ---- heads ----
    TileScratch<Checks> slot;
    int rc = slot.reserve(e, fqdclusters::tiles_of(n), stream);
    if (rc) return rc;
    unsigned long long m = 0;
    Checks found{};
    bool fits = false;
    rc = fqdclusters::count_heads(e, stream, slot, n, [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(head_count_kernel, grid, block, 0, stream, perm, head, label, n, slot.tile_sum, slot.counters);
    }, &m, &found, &fits);
    if (rc) return rc;
    if (found.bad || !fits)
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_subcluster_sizes: head[0] is not set, or the order names a record or a record's label is one outside 0 .. n-1 (are perm and head those of fqd_group_owners over these records, and the labels fqd_owners'? nothing was written)");

    // ---- classes ----
    SumBuffers b{};
    void* base = nullptr;
    if ((rc = fqd_internal_scratch(e, 0, carve_sums(n, m, nullptr, b), &base))) return rc;
    (void)carve_sums(n, m, static_cast<char*>(base), b);
    FQD_TRY(e, hipMemsetAsync(b.counters, 0, sizeof(Counters), stream));
    fqdclusters::write_heads(stream, slot, head, n, m, b.head_place);
    hipLaunchKernelGGL(classify_kernel, dim3(uint32_t((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, static_cast<const uint32_t*>(b.head_place), uint64_t(m), n,
                       b.lists, b.counters);
    FQD_TRY(e, hipGetLastError());
    Counters got{};
    FQD_TRY(e, read_back(got, b.counters, stream));          // (the tile sums have been read: the large tier may take their scratch)

    // ---- sums: the clusters of one, eight lanes, a wave, a block ----
    const Members mb{perm, label, weight};
    if (got.singles)
        hipLaunchKernelGGL(singles_kernel, dim3(grid_for(m, kBlock, 8192)), dim3(kBlock), 0, stream, static_cast<const uint32_t*>(b.head_place), mb, uint64_t(m), n,
                           abundance);
    if (got.listed[0])
        hipLaunchKernelGGL(small_kernel, dim3(uint32_t((uint64_t(got.listed[0]) * kSmall + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                           static_cast<const unsigned long long*>(b.lists.of[0]), got.listed[0], mb, abundance, b.counters);
    if (got.listed[1])
        hipLaunchKernelGGL(wave_kernel, dim3(uint32_t((uint64_t(got.listed[1]) * kWave + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                           static_cast<const unsigned long long*>(b.lists.of[1]), got.listed[1], mb, abundance, b.counters);
    if (got.listed[2])
        hipLaunchKernelGGL(block_kernel, dim3(got.listed[2]), dim3(kTableBlock), 0, stream, static_cast<const unsigned long long*>(b.lists.of[2]), mb, abundance,
                           b.counters);
    FQD_TRY(e, hipGetLastError());

    // ---- the large tier: a launch adds, a launch stores ----
    if (const uint32_t items = got.listed[3]) {
        Table t{};
        void* room = nullptr;
        if ((rc = fqd_internal_scratch(e, 1, carve_table(got.large_members, items, nullptr, t), &room))) return rc;
        (void)carve_table(got.large_members, items, static_cast<char*>(room), t);
        FQD_TRY(e, hipMemsetAsync(t.keys, 0xFF, size_t(t.slots) * sizeof(unsigned long long), stream));
        FQD_TRY(e, hipMemsetAsync(t.sums, 0, size_t(t.slots) * sizeof(unsigned long long), stream));
        FQD_TRY(e, hipMemsetAsync(t.distinct, 0, size_t(items) * sizeof(uint32_t), stream));
        const uint32_t gx = uint32_t(std::min<uint64_t>((uint64_t(got.largest) + kBlock - 1) / kBlock, kLargeMaxX));
        const dim3 grid(gx, std::min<uint32_t>(items, std::max<uint32_t>(1u, kLargeBlocks / gx)));
        const unsigned long long* list = b.lists.of[3];
        hipLaunchKernelGGL(large_add_kernel, grid, dim3(kBlock), 0, stream, list, items, mb, t);
        hipLaunchKernelGGL(large_store_kernel, grid, dim3(kBlock), 0, stream, list, items, mb, t, abundance, b.counters);
        FQD_TRY(e, hipGetLastError());
    }
    FQD_TRY(e, read_back(got, b.counters, stream));
    if (info) {
        info->clusters = m;
        info->mixed = got.mixed;
        info->subclusters = got.singles + got.subclusters;
        info->tier_clusters[0] = got.singles;
        for (int t = 0; t < 4; ++t) info->tier_clusters[t + 1] = got.listed[t];
        info->largest = got.largest;
    }
    return FQD_OK;
}

int fqd_subcluster_scores(fqd_engine* e, const uint32_t* perm, const uint8_t* head, const uint32_t* label, const uint32_t* score, uint64_t n,
                          uint32_t* masked)
{
    if (!e) return FQD_ERR_ARG;
    if (n >= 0x80000000ull || (n && (!perm || !head || !label || !score || !masked)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_subcluster_scores: bad arguments (the order and its head flags, the exact owners, the scores, and room for the masked scores of at most 2^31-1 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(perm, head, label, score, masked))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_subcluster_scores: every array is device memory");
    const size_t words = size_t(n) * sizeof(uint32_t);
    if (overlap(masked, words, perm, words) || overlap(masked, words, head, size_t(n)) || overlap(masked, words, label, words) || overlap(masked, words, score, words))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_subcluster_scores: masked overlaps an input");
    hipStream_t stream = fqd_internal_stream(e);
    const uint32_t tiles = uint32_t((n + kOffTile - 1) / kOffTile);
    void* small = nullptr;
    const int rc = fqd_internal_scratch(e, 1, size_t(tiles) * sizeof(uint32_t) + 512 + sizeof(Checks), &small);
    if (rc) return rc;
    Carver c{static_cast<char*>(small)};
    uint32_t* tile_last = c.take<uint32_t>(tiles);
    Checks* checks = c.take<Checks>(1);
    FQD_TRY(e, hipMemsetAsync(checks, 0, sizeof(Checks), stream));
    hipLaunchKernelGGL(last_head_tiles_kernel, dim3(tiles), dim3(kBlock), 0, stream, perm, head, n, tile_last, checks);
    hipLaunchKernelGGL(last_head_carry_kernel, dim3(1), dim3(1024), 0, stream, tile_last, tiles);
    FQD_TRY(e, hipGetLastError());
    Checks found{};
    FQD_TRY(e, read_back(found, checks, stream));
    if (found.bad)
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_subcluster_scores: head[0] is not set, or the order names a record outside 0 .. n-1 (are perm and head those of fqd_group_owners over these records? nothing was written)");
    hipLaunchKernelGGL(masked_scores_kernel, dim3(tiles), dim3(kBlock), 0, stream, perm, head, label, score, n, static_cast<const uint32_t*>(tile_last), masked);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, hipStreamSynchronize(stream));
    return FQD_OK;
}

} // extern "C"
