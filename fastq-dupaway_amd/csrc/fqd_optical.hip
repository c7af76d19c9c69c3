// fqd_optical.hip — FQD_FAST_OPTICAL=D of the `--fast` mode (same library as fqd_engine.hip): every record's place on the
// flow cell read off its ID line, and every cluster of identical reads split into its optical groups — the members that
// lie within D pixels of each other on one tile.  Rule and proofs: fqd_optical_core.hpp.  Nothing in here is called unless
// the switch is set.
//
//   places   read_places_kernel: size_annotations_kernel's shape — a wave takes a tile of 64 neighbouring records and works
//            through it four at a time, SIXTEEN LANES A RECORD, sixteen bytes a lane.  A lane's look (fqdumi::lane_look with
//            ':') gives the word ends and the colons of its chunk; an exclusive sum across the group ranks them, and the
//            group takes the places of the 4th .. 7th.  Lanes 0, 1 and 2 read tile, x and y; all sixteen hold the surface
//            against record 0's, a byte a lane.  The lowest refused record and its reason come back through one 64-bit
//            atomicMin a wave of (record << 3 | reason).  No load leaves the ID line.
//   heads    fqd_clusters.hpp's: head_count_kernel (tile_count; its own part: a place whose record lies outside 0 .. n-1,
//            place 0 without a head) + scan_tiles_kernel + head_write_kernel.  The count comes back to size the rest.
//   classes  classify_kernel, a lane a cluster (cluster_at): a cluster of ONE member — most of them — is only counted; a
//            longer one goes on the list of its size class (list_append).  A cluster beyond the limit is reported
//            through one 64-bit atomicMin of (first record << 32 | members).  The counts come back for the grids.
//   split    singles_kernel: a lane a cluster of one, one store.  split_lanes_kernel<8>: eight lanes a cluster, eight
//            clusters a wave; split_lanes_kernel<64>: a wave a cluster — a lane holds its member's neighbours as a 64-bit
//            mask and its label, and both steps of a sweep read the other lanes' labels across the lanes.
//            split_block_kernel: a workgroup a cluster of up to kBlockLimit, places and labels in LDS, two members a
//            thread; a step's results wait in registers for the barrier that ends its reads.  The large tier, up to
//            FQD_OPTICAL_MAX_CLUSTER: a thread a member, many blocks a cluster, the places read through perm from the
//            per-record arrays (a cluster's stay in L2) and the labels in two arrays in scratch; a step is a launch
//            (large_min_kernel, large_jump_kernel), and the host asks after every sweep whether a label changed.
//            Every kernel stores owner_out of its own clusters' members; nothing is stored where a cluster is refused.
#include <hip/hip_runtime.h>

#include "fqd_clusters.hpp"
#include "fqd_optical_core.hpp"

namespace {

using namespace fqdoptical;

constexpr int kBlock = fqdscan::kBlock;
constexpr uint32_t kWaveTile = 64;                           // records a wave (places)
constexpr uint32_t kTile = kWaveTile * (kBlock / 64);        // records a block (places)
constexpr int kSplitBlock = 1024;                            // threads of a cluster's block
constexpr int kPerThread = int(kBlockLimit) / kSplitBlock;
constexpr uint32_t kLargeChunks = (kMaxCluster + kBlock - 1) / kBlock;

static_assert(kPerThread * kSplitBlock == int(kBlockLimit), "a block's threads share the largest cluster in LDS evenly");
static_assert(kWave == 64 && 64 % kSmall == 0 && kGroup == 16, "the lane kernels' groups tile a wave");
static_assert(6 * kBlockLimit * sizeof(uint32_t) <= 64 * 1024, "places, records and labels of a cluster fit a workgroup's LDS");

using fqdclusters::cluster_at;
using fqdclusters::entry_members;
using fqdclusters::entry_place;
using fqdclusters::kNoBad;
using fqdwave::wave_max;
using fqdwave::wave_sum;

// ---- places ----------------------------------------------------------------------------------------------------------------

struct Found { unsigned long long bad, other; };             // the lowest (record << 3 | reason); records on another surface than record 0

// One wave per tile of kWaveTile records; see the head of the file.
__global__ __launch_bounds__(kBlock)
void read_places_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ id_start, const uint32_t* __restrict__ id_len, uint64_t n,
                        uint32_t* __restrict__ tile, uint32_t* __restrict__ x, uint32_t* __restrict__ y, uint32_t* __restrict__ surface, Found* found)
{
    const uint32_t lane = threadIdx.x & 63u, g = lane / kGroup, gl = lane % kGroup;
    const uint64_t tile0 = (uint64_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6)) * kWaveTile;
    if (tile0 >= n) return;                                  // (the whole wave)
    const uint64_t mine = tile0 + lane;
    unsigned long long line_at = 0;
    uint32_t line_len = 0;
    if (mine < n) { line_at = id_start[mine]; line_len = id_len[mine]; }
    const uint8_t* __restrict__ line0 = text + id_start[0];
    const uint32_t len0 = id_len[0];
    Place my{0u, 0u, 0u, 0u, kOk};
    for (uint32_t j = 0; j < kWaveTile / 4u && tile0 + 4u * j < n; ++j) {
        const int r = int(4u * j + g);                       // the group's record of this step (beyond n: an empty line)
        const uint8_t* __restrict__ line = text + __shfl(line_at, r, 64);
        const uint32_t L = __shfl(line_len, r, 64);

        // ---- rounds: the word's end, the colons' number and the places of the 4th .. 7th ----
        const uint32_t chunks = fqdumi::line_chunks(L);
        uint32_t end = fqdumi::kNone, colons = 0, c[4] = {kNone, kNone, kNone, kNone}, empty = 0;
        for (uint32_t c0 = 0; __any(end == fqdumi::kNone && c0 < chunks); c0 += kGroup) {
            const bool live = end == fqdumi::kNone && c0 < chunks;
            fqdumi::Look k{0u, 0u, 0u};
            if (live) k = fqdumi::lane_look(line, L, uint8_t(':'), c0, gl);
            const uint32_t e = fqdwave::group_min<kGroup>(fqdumi::look_end(k));
            const uint32_t own = live ? uint32_t(__builtin_popcount(colons_below(k, e))) : 0u;
            const uint32_t inc = fqdwave::wave_inclusive<uint32_t, kGroup>(own);
            Colons got{0u, {kNone, kNone, kNone, kNone}, false};
            if (live && own) got = lane_colons(line, k, e, colons + inc - own);
#pragma unroll
            for (int f = 0; f < 4; ++f) { const uint32_t at = fqdwave::group_min<kGroup>(got.at[f]); if (c[f] == kNone) c[f] = at; }
            empty |= fqdwave::group_or<kGroup>(got.empty ? 1u : 0u);
            colons += __shfl(inc, int(kGroup) - 1, int(kGroup));
            if (live) end = e;
        }
        if (end == fqdumi::kNone) end = L;                   // no word end in the line: the word ends with it

        // ---- fields: lanes 0, 1, 2 read tile, x, y ----
        uint32_t reason_f = kOk, value_f = 0;
        if (gl < 3u && colons >= 6u && !empty && c[2] + 1u < (colons >= 7u ? c[3] : end)) reason_f = field_number(line, c, colons, end, gl, &value_f);
        uint32_t reasons[3], values[3];
#pragma unroll
        for (int f = 0; f < 3; ++f) { reasons[f] = __shfl(reason_f, f, int(kGroup)); values[f] = __shfl(value_f, f, int(kGroup)); }
        Place p = judge(colons, c, end, empty != 0, reasons, values);

        // ---- the surface against record 0's, a byte a lane ----
        uint32_t differs = 0;
        if (p.reason == kOk)
            for (uint32_t b = 1u + gl; b <= c[0]; b += kGroup) differs |= surface_byte_same(line0, len0, line, b) ? 0u : 1u;
        if (p.reason == kOk && !fqdwave::group_or<kGroup>(differs)) p.surface |= kSameSurface;

        const int from = int((lane & 3u) * kGroup);
        const uint32_t got_tile = __shfl(p.tile, from, 64), got_x = __shfl(p.x, from, 64), got_y = __shfl(p.y, from, 64);
        const uint32_t got_surface = __shfl(p.surface, from, 64), got_reason = __shfl(p.reason, from, 64);
        if ((lane >> 2) == j) my = Place{got_tile, got_x, got_y, got_surface, got_reason};   // record `lane` of the tile is group lane%4's at step lane/4
    }
    unsigned long long word = kNoBad;
    uint32_t other = 0;
    if (mine < n) {
        tile[mine] = my.tile; x[mine] = my.x; y[mine] = my.y; surface[mine] = my.surface;
        if (my.reason) word = fqdclusters::bad_word(mine, my.reason);
        else other = my.surface & kSameSurface ? 0u : 1u;
    }
    word = fqdwave::wave_min(word);
    other = wave_sum(other);
    if (lane == 0) {
        if (word != kNoBad) atomicMin(&found->bad, word);
        if (other) atomicAdd(&found->other, static_cast<unsigned long long>(other));
    }
}

// ---- heads -------------------------------------------------------------------------------------------------------------------

// What the kernels count (one in scratch, zeroed per call).
struct Counters {
    unsigned long long over;                                 // the lowest (first record << 32 | members) of a cluster beyond the limit
    unsigned long long bad;                                  // places whose record lies outside 0 .. n-1; place 0 without a head
    unsigned long long groups;                               // optical groups of the listed clusters
    unsigned long long split;                                // listed clusters of more than one group
    uint32_t listed[4];                                      // clusters on the small, wave, block and large lists
    uint32_t singles, largest, sweeps, live;                 // live: large clusters a sweep changed
};

__global__ __launch_bounds__(kBlock)
void head_count_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ head, uint64_t n, unsigned long long* __restrict__ tile_sum,
                       Counters* counters)
{
    uint32_t bad = 0;
    fqdclusters::tile_count<4>(n, tile_sum, [&](uint64_t k) __attribute__((always_inline)) {
        const bool h = head[k] != 0;
        bad += perm[k] >= n || (k == 0 && !h);
        return h;
    });
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&counters->bad, static_cast<unsigned long long>(bad));
}

// ---- classes -----------------------------------------------------------------------------------------------------------------

using Lists = fqdclusters::Lists<4>;                         // the small, wave, block and large lists

__global__ __launch_bounds__(kBlock)
void classify_kernel(const uint32_t* __restrict__ head_place, const uint32_t* __restrict__ perm, uint64_t m, uint64_t n, Lists lists, Counters* counters)
{
    const uint64_t c = blockIdx.x * uint64_t(kBlock) + threadIdx.x;     // (no stride: every lane of a wave reaches the ballots)
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t s = 0, k0 = 0;
    if (c < m) s = cluster_at(head_place, m, n, c, &k0);
    const uint32_t cls = s == 0u ? 6u : s == 1u ? 5u : s <= kSmall ? 0u : s <= kWave ? 1u : s <= kBlockLimit ? 2u : s <= kMaxCluster ? 3u : 4u;
    fqdclusters::list_append(lists, counters->listed, cls, k0, s);
    if (cls == 4u) atomicMin(&counters->over, (static_cast<unsigned long long>(perm[k0]) << 32) | s);
    const uint32_t singles = uint32_t(__popcll(__ballot(cls == 5u)));
    const uint32_t largest = wave_max(s);
    if (lane == 0) {
        if (singles) atomicAdd(&counters->singles, singles);
        if (largest) atomicMax(&counters->largest, largest);
    }
}

// ---- split -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void singles_kernel(const uint32_t* __restrict__ head_place, const uint32_t* __restrict__ perm, uint64_t m, uint64_t n, uint32_t* __restrict__ owner_out)
{
    for (uint64_t c = blockIdx.x * uint64_t(kBlock) + threadIdx.x; c < m; c += uint64_t(gridDim.x) * kBlock) {
        uint32_t k0;
        if (cluster_at(head_place, m, n, c, &k0) == 1u) { const uint32_t r = perm[k0]; owner_out[r] = r; }
    }
}

struct Places { const uint8_t* text; const uint64_t* id_start; const uint32_t *tile, *x, *y, *surface; };

// G lanes a cluster (8 or 64), a lane a member; see the head of the file.
template <uint32_t G>
__global__ __launch_bounds__(kBlock)
void split_lanes_kernel(const unsigned long long* __restrict__ list, uint32_t n_items, const uint32_t* __restrict__ perm, Places pl, uint32_t D,
                        uint32_t* __restrict__ owner_out, Counters* counters)
{
    const uint32_t lane = threadIdx.x & 63u, gl = lane % G;
    const uint64_t item = (blockIdx.x * uint64_t(kBlock) + threadIdx.x) / G;
    uint32_t s = 0;
    uint64_t k0 = 0;
    if (item < n_items) { const unsigned long long e = list[item]; k0 = entry_place(e); s = entry_members(e); }
    if (s > G) s = 0;                                        // (no list holds such an entry)
    const bool live = gl < s;
    uint32_t rec = 0, t = 0, x = 0, y = 0, sw = 0;
    const uint8_t* bytes = pl.text;
    if (live) { rec = perm[k0 + gl]; t = pl.tile[rec]; x = pl.x[rec]; y = pl.y[rec]; sw = pl.surface[rec]; bytes = pl.text + pl.id_start[rec] + 1; }
    // every lane of the wave asks the same places: the cluster's members where a wave holds one cluster, all G where it holds several
    const uint32_t s_all = G == 64u ? uint32_t(__builtin_amdgcn_readfirstlane(int(s))) : G;
    const uint64_t neighbours = lane_neighbours(live, gl, s, s_all, t, x, y, sw, bytes, D,
        [&](uint32_t u, uint32_t* tu, uint32_t* xu, uint32_t* yu, uint32_t* su) {
            *tu = __shfl(t, int(u), int(G)); *xu = __shfl(x, int(u), int(G)); *yu = __shfl(y, int(u), int(G)); *su = __shfl(sw, int(u), int(G));
        },
        [&](uint32_t u) { return reinterpret_cast<const uint8_t*>(__shfl(reinterpret_cast<unsigned long long>(bytes), int(u), int(G))); });
    uint32_t label = gl, sweeps = 0;
    for (uint32_t round = 1; round <= G; ++round) {          // (a cluster of s members is through after s - 1 sweeps at most)
        const uint32_t old = label;
        const uint32_t low = lane_min(neighbours, old, s_all, [&](uint32_t u) { return __shfl(old, int(u), int(G)); });
        const bool changed = low != old;
        if (!__any(changed)) break;
        label = __shfl(low, int(low), int(G));               // (low <= gl < G; a cluster at rest jumps to where it is)
        if (changed) sweeps = round;
    }
    const uint32_t owner = __shfl(rec, int(label), int(G));
    if (live) owner_out[rec] = owner;
    const unsigned long long apart = __ballot(live && label != 0u);
    const bool fell_apart = live && gl == 0u && ((apart >> (lane & ~(G - 1u))) & (G == 64u ? ~0ull : ((1ull << (G & 63u)) - 1ull))) != 0ull;
    const uint32_t groups = uint32_t(__popcll(__ballot(live && label == gl)));
    const uint32_t split = uint32_t(__popcll(__ballot(fell_apart)));
    sweeps = wave_max(sweeps);
    if (lane == 0) {
        if (groups) atomicAdd(&counters->groups, static_cast<unsigned long long>(groups));
        if (split) atomicAdd(&counters->split, static_cast<unsigned long long>(split));
        if (sweeps) atomicMax(&counters->sweeps, sweeps);
    }
}

// A block a cluster of up to kBlockLimit members; see the head of the file.
__global__ __launch_bounds__(kSplitBlock)
void split_block_kernel(const unsigned long long* __restrict__ list, const uint32_t* __restrict__ perm, Places pl, uint32_t D,
                        uint32_t* __restrict__ owner_out, Counters* counters)
{
    __shared__ uint32_t T[kBlockLimit], X[kBlockLimit], Y[kBlockLimit], S[kBlockLimit], R[kBlockLimit], labels[kBlockLimit];
    const unsigned long long e = list[blockIdx.x];
    const uint64_t k0 = entry_place(e);
    uint32_t s = entry_members(e);
    if (s > kBlockLimit) s = 0;                              // (no list holds such an entry)
    for (uint32_t v = threadIdx.x; v < s; v += kSplitBlock) {
        const uint32_t r = perm[k0 + v];
        R[v] = r; T[v] = pl.tile[r]; X[v] = pl.x[r]; Y[v] = pl.y[r]; S[v] = pl.surface[r]; labels[v] = v;
    }
    __syncthreads();
    auto bytes_of = [&](uint32_t u) { return pl.text + pl.id_start[R[u]] + 1; };
    uint32_t sweeps = 0;
    for (uint32_t round = 0; round < s; ++round) {
        uint32_t next[kPerThread];
        bool changed = false;
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
            const uint32_t v = threadIdx.x + uint32_t(j) * kSplitBlock;
            next[j] = 0;
            if (v < s) { next[j] = array_min(T, X, Y, S, labels, s, D, v, bytes_of); changed |= next[j] != labels[v]; }
        }
        if (!__syncthreads_or(changed)) break;               // (the barrier ends the min step's reads)
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) { const uint32_t v = threadIdx.x + uint32_t(j) * kSplitBlock; if (v < s) labels[v] = next[j]; }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) { const uint32_t v = threadIdx.x + uint32_t(j) * kSplitBlock; if (v < s) next[j] = labels[next[j]]; }
        __syncthreads();                                     // (and this one the jump's)
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) { const uint32_t v = threadIdx.x + uint32_t(j) * kSplitBlock; if (v < s) labels[v] = next[j]; }
        ++sweeps;
        __syncthreads();
    }
    uint32_t groups = 0;
    bool apart = false;
    for (uint32_t v = threadIdx.x; v < s; v += kSplitBlock) {
        owner_out[R[v]] = R[labels[v]];
        groups += labels[v] == v;
        apart |= labels[v] != 0u;
    }
    const int fell_apart = __syncthreads_or(apart);
    groups = wave_sum(groups);
    if ((threadIdx.x & 63) == 0 && groups) atomicAdd(&counters->groups, static_cast<unsigned long long>(groups));
    if (threadIdx.x == 0) {
        if (fell_apart) atomicAdd(&counters->split, 1ull);
        if (sweeps) atomicMax(&counters->sweeps, sweeps);
    }
}

// ---- the large tier: a thread a member, blockIdx.x = the member's chunk of kBlock, blockIdx.y strides over the clusters ------

struct Large { uint32_t *labels, *next, *changed[2], *sweeps; };   // labels, next: a word a place; changed, sweeps: a word a cluster

__global__ __launch_bounds__(kBlock)
void large_start_kernel(const unsigned long long* __restrict__ list, uint32_t n_items, Large lg)
{
    for (uint32_t item = blockIdx.y; item < n_items; item += gridDim.y) {
        const unsigned long long e = list[item];
        const uint64_t k0 = entry_place(e);
        const uint32_t s = entry_members(e), v = blockIdx.x * kBlock + threadIdx.x;
        if (v < s && s <= kMaxCluster) lg.labels[k0 + v] = v;
        if (v == 0) lg.sweeps[item] = 0;
    }
}

// The min step; was = the flags of the sweep before (nullptr: the first), now = this one's, zeroed in front of the launch.
__global__ __launch_bounds__(kBlock)
void large_min_kernel(const unsigned long long* __restrict__ list, uint32_t n_items, const uint32_t* __restrict__ perm, Places pl, uint32_t D,
                      Large lg, const uint32_t* __restrict__ was, uint32_t* __restrict__ now)
{
    for (uint32_t item = blockIdx.y; item < n_items; item += gridDim.y) {
        const unsigned long long e = list[item];
        const uint64_t k0 = entry_place(e);
        const uint32_t s = entry_members(e), v = blockIdx.x * kBlock + threadIdx.x;
        if (blockIdx.x * kBlock >= s || s > kMaxCluster) continue;       // (the whole block)
        if (was && !was[item]) continue;                                 // (the whole block: the cluster is at rest)
        const bool live = v < s;
        const uint32_t* __restrict__ P = perm + k0;
        const uint32_t* __restrict__ labels = lg.labels + k0;
        uint32_t best = 0, t = 0, x = 0, y = 0, sw = 0;
        const uint8_t* bytes = pl.text;
        if (live) {
            const uint32_t r = P[v];
            best = labels[v]; t = pl.tile[r]; x = pl.x[r]; y = pl.y[r]; sw = pl.surface[r]; bytes = pl.text + pl.id_start[r] + 1;
        }
        const uint32_t old = best;
        for (uint32_t u = 0; u < s; ++u) {
            const uint32_t lu = labels[u];
            if (!live || lu >= best) continue;
            const uint32_t ru = P[u];
            if (!close(pl.tile[ru], pl.x[ru], pl.y[ru], t, x, y, D)) continue;
            const uint32_t q = surfaces_quick(pl.surface[ru], sw);
            if (q == 2u ? bytes_same(pl.text + pl.id_start[ru] + 1, bytes, sw) : q == 1u) best = lu;
        }
        if (live) lg.next[k0 + v] = best;
        if (__any(live && best != old) && (threadIdx.x & 63) == 0) now[item] = 1u;
    }
}

__global__ __launch_bounds__(kBlock)
void large_jump_kernel(const unsigned long long* __restrict__ list, uint32_t n_items, Large lg, const uint32_t* __restrict__ now, Counters* counters)
{
    for (uint32_t item = blockIdx.y; item < n_items; item += gridDim.y) {
        const unsigned long long e = list[item];
        const uint64_t k0 = entry_place(e);
        const uint32_t s = entry_members(e), v = blockIdx.x * kBlock + threadIdx.x;
        if (blockIdx.x * kBlock >= s || s > kMaxCluster || !now[item]) continue;
        if (v < s) lg.labels[k0 + v] = lg.next[k0 + lg.next[k0 + v]];
        if (v == 0) { lg.sweeps[item] += 1u; atomicAdd(&counters->live, 1u); }
    }
}

// apart: a word a cluster, zeroed in front of the launch.
__global__ __launch_bounds__(kBlock)
void large_finish_kernel(const unsigned long long* __restrict__ list, uint32_t n_items, const uint32_t* __restrict__ perm, Large lg,
                         uint32_t* __restrict__ apart, uint32_t* __restrict__ owner_out, Counters* counters)
{
    for (uint32_t item = blockIdx.y; item < n_items; item += gridDim.y) {
        const unsigned long long e = list[item];
        const uint64_t k0 = entry_place(e);
        const uint32_t s = entry_members(e), v = blockIdx.x * kBlock + threadIdx.x;
        if (blockIdx.x * kBlock >= s || s > kMaxCluster) continue;
        uint32_t label = 0;
        if (v < s) { label = lg.labels[k0 + v]; owner_out[perm[k0 + v]] = perm[k0 + label]; }
        const uint32_t groups = uint32_t(__popcll(__ballot(v < s && label == v)));
        const bool any_apart = __any(v < s && label != 0u);
        if ((threadIdx.x & 63) == 0) {
            if (groups) atomicAdd(&counters->groups, static_cast<unsigned long long>(groups));
            if (any_apart && atomicExch(&apart[item], 1u) == 0u) atomicAdd(&counters->split, 1ull);
        }
        if (v == 0 && lg.sweeps[item]) atomicMax(&counters->sweeps, lg.sweeps[item]);
    }
}

struct SplitBuffers { uint32_t* head_place; Lists lists; Large large; };

size_t carve_split(uint64_t n, uint64_t m, char* base, SplitBuffers& b)
{
    Carver c{base};
    b.head_place = c.take<uint32_t>(m);
    fqdclusters::take_lists(c, n, {1u, kSmall, kWave, kBlockLimit}, b.lists);
    const size_t large = fqdclusters::list_room(n, kBlockLimit);
    b.large.labels = c.take<uint32_t>(n > kBlockLimit ? n : 0); b.large.next = c.take<uint32_t>(n > kBlockLimit ? n : 0);
    b.large.changed[0] = c.take<uint32_t>(large); b.large.changed[1] = c.take<uint32_t>(large); b.large.sweeps = c.take<uint32_t>(large);
    return c.used + 256;
}

} // namespace

extern "C" {

int fqd_read_places(fqd_engine* e, const uint8_t* text, const uint64_t* id_start, const uint32_t* id_len, uint64_t n, uint32_t* tile, uint32_t* x,
                    uint32_t* y, uint32_t* surface, fqd_places_info* info)
{
    if (!e) return FQD_ERR_ARG;
    if (info) *info = fqd_places_info{FQD_UMI_NO_RECORD, FQD_PLACE_OK, 0, 0};
    if (!info || n > 0xFFFFFFFEull || (n && (!text || !id_start || !id_len || !tile || !x || !y || !surface)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_read_places: bad arguments (info, the text, the ID lines' starts and lengths, and room for tile, x, y and surface of at most 2^32-2 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(text, id_start, id_len, tile, x, y, surface))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_read_places: the text and every array are device memory");
    hipStream_t s = fqd_internal_stream(e);
    void* scratch = nullptr;
    const int rc = fqd_internal_scratch(e, 1, 4096, &scratch);
    if (rc) return rc;
    Found* found = static_cast<Found*>(scratch);
    FQD_TRY(e, zero_counters(found, s, &Found::bad));
    hipLaunchKernelGGL(read_places_kernel, dim3(uint32_t((n + kTile - 1) / kTile)), dim3(kBlock), 0, s, text, id_start, id_len, n, tile, x, y, surface, found);
    FQD_TRY(e, hipGetLastError());
    Found got{};
    FQD_TRY(e, read_back(got, found, s));
    if (got.bad != kNoBad) fqdclusters::bad_parts(got.bad, &info->bad_record, &info->bad_reason);
    info->other_surface = got.other;
    return FQD_OK;
}

int fqd_optical_split(fqd_engine* e, const uint32_t* perm, const uint8_t* head, const uint8_t* text, const uint64_t* id_start, const uint32_t* tile,
                      const uint32_t* x, const uint32_t* y, const uint32_t* surface, uint64_t n, uint32_t distance, uint32_t* owner_out,
                      fqd_optical_info* out)
{
    if (!e) return FQD_ERR_ARG;
    if (out) *out = fqd_optical_info{0, 0, 0, 0, 0, FQD_OPTICAL_MAX_CLUSTER, 0, FQD_UMI_NO_RECORD, {0, 0, 0, 0}};
    if (!out || distance == 0 || distance > 0x7FFFFFFFu || n >= 0x80000000ull ||
        (n && (!perm || !head || !text || !id_start || !tile || !x || !y || !surface || !owner_out)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_optical_split: bad arguments (the info, a distance of 1 .. 2^31-1, the order and its head flags, the text, the ID lines' starts, tile, x, y and surface, and room for the owners of at most 2^31-1 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(perm, head, text, id_start, tile, x, y, surface, owner_out))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_optical_split: the text and every array are device memory");
    const size_t words = size_t(n) * sizeof(uint32_t);
    if (overlap(owner_out, words, perm, words) || overlap(owner_out, words, head, size_t(n)) || overlap(owner_out, words, id_start, 2 * words) ||
        overlap(owner_out, words, tile, words) || overlap(owner_out, words, x, words) || overlap(owner_out, words, y, words) ||
        overlap(owner_out, words, surface, words))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_optical_split: owner_out overlaps an input");
    hipStream_t stream = fqd_internal_stream(e);
    StageTimer timer{out->stage_ms};

    // ---- heads ----
    TileScratch<Counters> slot;
    int rc = slot.reserve(e, fqdclusters::tiles_of(n), stream, &Counters::over);
    if (rc) return rc;
    Counters* counters = slot.counters;
    unsigned long long m = 0;
    Counters got{};
    bool fits = false;
    rc = fqdclusters::count_heads(e, stream, slot, n, [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(head_count_kernel, grid, block, 0, stream, perm, head, n, slot.tile_sum, counters);
    }, &m, &got, &fits);
    if (rc) return rc;
    if (got.bad || !fits)
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_optical_split: head[0] is not set, or the order names a record outside 0 .. n-1 (are perm and head those of fqd_group_owners over these records? nothing was written)");
    out->clusters_in = m;

    // ---- classes ----
    SplitBuffers b{};
    void* base = nullptr;
    if ((rc = fqd_internal_scratch(e, 0, carve_split(n, m, nullptr, b), &base))) return rc;
    (void)carve_split(n, m, static_cast<char*>(base), b);
    fqdclusters::write_heads(stream, slot, head, n, m, b.head_place);
    hipLaunchKernelGGL(classify_kernel, dim3(uint32_t((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, static_cast<const uint32_t*>(b.head_place), perm,
                       uint64_t(m), n, b.lists, counters);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, read_back(got, counters, stream));
    out->largest = got.largest;
    timer.mark(0);
    if (got.over != kNoBad) {                                 // refused: owner_out stays as it is
        out->over_limit_first = got.over >> 32;
        out->over_limit_members = uint32_t(got.over);
        return FQD_OK;
    }

    // ---- split: the clusters of one, eight lanes, a wave, a block ----
    const Places pl{text, id_start, tile, x, y, surface};
    const uint32_t D = distance;
    if (got.singles)
        hipLaunchKernelGGL(singles_kernel, dim3(grid_for(m, kBlock, 8192)), dim3(kBlock), 0, stream, static_cast<const uint32_t*>(b.head_place), perm, uint64_t(m), n,
                           owner_out);
    if (got.listed[0])
        hipLaunchKernelGGL(split_lanes_kernel<kSmall>, dim3(uint32_t((uint64_t(got.listed[0]) * kSmall + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                           static_cast<const unsigned long long*>(b.lists.of[0]), got.listed[0], perm, pl, D, owner_out, counters);
    if (got.listed[1])
        hipLaunchKernelGGL(split_lanes_kernel<kWave>, dim3(uint32_t((uint64_t(got.listed[1]) * kWave + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                           static_cast<const unsigned long long*>(b.lists.of[1]), got.listed[1], perm, pl, D, owner_out, counters);
    if (got.listed[2])
        hipLaunchKernelGGL(split_block_kernel, dim3(got.listed[2]), dim3(kSplitBlock), 0, stream, static_cast<const unsigned long long*>(b.lists.of[2]), perm, pl, D,
                           owner_out, counters);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, hipStreamSynchronize(stream));
    timer.mark(1);

    // ---- the large tier: a launch a step, a question a sweep ----
    if (const uint32_t items = got.listed[3]) {
        const unsigned long long* list = b.lists.of[3];
        const dim3 grid(kLargeChunks, std::min<uint32_t>(items, 65535u));
        hipLaunchKernelGGL(large_start_kernel, grid, dim3(kBlock), 0, stream, list, items, b.large);
        for (uint32_t round = 0; round < kMaxCluster; ++round) {
            uint32_t* now = b.large.changed[round & 1u];
            FQD_TRY(e, hipMemsetAsync(now, 0, size_t(items) * sizeof(uint32_t), stream));
            FQD_TRY(e, hipMemsetAsync(&counters->live, 0, sizeof(uint32_t), stream));
            hipLaunchKernelGGL(large_min_kernel, grid, dim3(kBlock), 0, stream, list, items, perm, pl, D, b.large,
                               round ? static_cast<const uint32_t*>(b.large.changed[(round - 1u) & 1u]) : static_cast<const uint32_t*>(nullptr), now);
            hipLaunchKernelGGL(large_jump_kernel, grid, dim3(kBlock), 0, stream, list, items, b.large, static_cast<const uint32_t*>(now), counters);
            FQD_TRY(e, hipGetLastError());
            uint32_t live = 0;
            FQD_TRY(e, read_back(live, &counters->live, stream));
            if (!live) break;
        }
        FQD_TRY(e, hipMemsetAsync(b.large.changed[0], 0, size_t(items) * sizeof(uint32_t), stream));
        hipLaunchKernelGGL(large_finish_kernel, grid, dim3(kBlock), 0, stream, list, items, perm, b.large, b.large.changed[0], owner_out, counters);
        FQD_TRY(e, hipGetLastError());
    }
    FQD_TRY(e, read_back(got, counters, stream));
    out->clusters_out = got.singles + got.groups;
    out->split = got.split;
    out->sweeps = got.sweeps;
    timer.mark(2);
    return FQD_OK;
}

} // extern "C"
