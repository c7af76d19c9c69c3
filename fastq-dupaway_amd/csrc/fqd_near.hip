// fqd_near.hip — FQD_FAST_HAMMING=D of the `--fast` mode (same library as fqd_engine.hip): the engine's exact clusters that
// differ in at most D substituted bases a mate are merged, through a seed join instead of all pairs.  Rule and proofs:
// fqd_near_core.hpp.  Nothing in here is called unless the switch is set.
// FQD_FAST_UMI_HAMMING=D (fqd_near_merge_umi; rule: fqd_near_umi_core.hpp) is the same join with every node's UMI tag in its
// seed keys and in front of the verification, and the links of FQD_FAST_UMI_MISMATCH in front of the near edges: seeds and
// verify are one body each with the tag compiled in or out (seeds_umi_kernel, verify_umi_kernel), count_links_kernel and
// links_kernel are its own, and everything else is shared as it stands.  The untagged kernels load no tag.
//
//   seeds    count_nodes_kernel counts the nodes (owner[i] == i) and holds the owners against their own rule; the count comes
//            back to size the rest.  seeds_kernel, a lane a record: a node takes D + 1 neighbouring places of the entry list —
//            a wave adds to the list's end with one atomic — and writes (seed key, node) for every segment of its mate 1,
//            sixteen bytes a load (fqdnear::seed_key).  In which order the nodes stand in the list depends on scheduling;
//            nothing behind the sort does.
//   sort     fqd_internal_radix_sort over the 64 key bits.  mark_kernel, a lane an entry: the first entry of a group finds
//            the group's end (a gallop and a binary search over the sorted keys) and with it the size; the groups are counted
//            and the largest is kept.  An entry with an equal key half the limit away on either side — every entry of a
//            group beyond the limit has one — finds both ends, and where the group is beyond the limit offers
//            (its node << 32 | size) to one 64-bit atomicMin: the lowest first record of such a group, and that group's size.
//            An entry that has a later entry in its group — few have — goes on the work list, a wave adding to it with one
//            atomic; the list lies in the sort's other key array, which nobody reads any more.
//   verify   verify_kernel, EIGHT LANES AN ENTRY OF THE WORK LIST: the later entries of its group are its candidates, one
//            after another.  An entry of the same node is skipped; the shapes are compared as numbers; then the lanes count the differing bytes
//            of mate 1, sixteen bytes a lane and round (fqdnear::chunk_mismatches), sum across the eight behind every round
//            and stop once the sum is above D; mate 2 likewise.  A pair that passes is appended to the edge list by the
//            group's first lane.  The list has a capacity: the kernel counts every edge and stores those that fit, and where
//            the count is above the capacity the host makes room for the count and runs the kernel once more (the count does
//            not depend on scheduling, so the second run fits).  Every loop's condition is a wave-wide vote, so the eight
//            lanes of a group are together at every cross-lane sum.
//   sweeps   the labels, a word a record, in scratch; owner_out serves as the array the min step writes.  A sweep:
//            copy labels -> next, edge_min_kernel (a lane an edge, atomicMin into next), the host asks whether an edge had two
//            labels, jump_kernel (labels[v] = next[next[v]]).  finish_kernel: owner_out[i] = labels[owner[i]].
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>

#include "fqd_groups.hpp"
#include "fqd_internal.hpp"
#include "fqd_near_core.hpp"
#include "fqd_near_umi_core.hpp"
#include "fqd_wave.hpp"

namespace {

using namespace fqdnear;

constexpr int kBlock = 256;
constexpr unsigned long long kNoOver = ~0ull;

static_assert(64 % kLanes == 0 && kLanes == 8, "the verify kernel's groups tile a wave");

struct Counters {
    unsigned long long nodes, bad, cursor, groups, largest, work, pairs, edges, merged, over;
    uint32_t changed, pad;
    unsigned long long links;
};

// One mate's reads as the kernels see them (fqd_reads).
struct Mate {
    const uint8_t* bases; const uint64_t* off; const uint32_t* len; uint32_t ulen, ustride;
    __device__ __forceinline__ const uint8_t* at(uint32_t r) const { return off ? bases + off[r] : bases + uint64_t(r) * ustride; }
    __device__ __forceinline__ uint32_t length(uint32_t r) const { return len ? len[r] : ulen; }
};

// FQD_FAST_UMI_HAMMING: where every record's UMI field U lies (fqd_umi_find's over file 1) and the run's one shape.
struct Tags {
    const uint8_t* text; const uint64_t* id_start; const uint32_t* umi_off; uint32_t umi_len; uint64_t joiners;
    __device__ __forceinline__ const uint8_t* at(uint32_t r) const { return text + id_start[r] + umi_off[r]; }
};

using fqdwave::wave_sum;

// ---- seeds -------------------------------------------------------------------------------------------------------------------

// bad: an owner above its record (that covers one outside 0 .. n-1), or one that is not its own owner.
__global__ __launch_bounds__(kBlock)
void count_nodes_kernel(const uint32_t* __restrict__ owner, uint64_t n, Counters* counters)
{
    unsigned long long nodes = 0, bad = 0;
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
        const uint32_t o = owner[i];
        if (o > i) { ++bad; continue; }
        nodes += o == i;
        bad += o != i && owner[o] != o;
    }
    nodes = wave_sum(nodes); bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0) {
        if (nodes) atomicAdd(&counters->nodes, nodes);
        if (bad) atomicAdd(&counters->bad, bad);
    }
}

// A lane a record, no stride: every lane of a wave reaches the ballot.  room = the entries the lists hold.  kTagged: the node
// loads its tag once and absorbs it into each of its D + 1 keys.
template <bool kTagged>
__device__ __forceinline__ void seeds_body(const Mate& m1, const Mate& m2, bool paired, const uint32_t* __restrict__ owner, uint64_t n, uint32_t D, bool weak,
                                           uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint64_t room, Counters* counters, const Tags& tags)
{
    const uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x;
    const bool node = i < n && owner[i] == uint32_t(i);
    const unsigned long long at = fqdwave::ballot_append(node, &counters->cursor, static_cast<unsigned long long>(D + 1u));
    if (!node) return;
    const uint32_t r = uint32_t(i), len1 = m1.length(r), len2 = paired ? m2.length(r) : 0u;
    const uint8_t* p = m1.at(r);
    if constexpr (kTagged) {
        const fqdnearumi::Tag t = fqdnearumi::load_tag(tags.at(r), tags.umi_len, tags.joiners);
        const uint32_t words = fqdnearumi::tag_words(tags.umi_len);
        for (uint32_t j = 0; j <= D; ++j)
            if (at + j < room) { keys[at + j] = fqdnearumi::tagged_seed(t, words, p, len1, len2, D, j, weak); vals[at + j] = r; }
    } else {
        for (uint32_t j = 0; j <= D; ++j)
            if (at + j < room) { keys[at + j] = node_seed(p, len1, len2, D, j, weak); vals[at + j] = r; }
    }
}

__global__ __launch_bounds__(kBlock)
void seeds_kernel(Mate m1, Mate m2, bool paired, const uint32_t* __restrict__ owner, uint64_t n, uint32_t D, bool weak, uint64_t* __restrict__ keys,
                  uint32_t* __restrict__ vals, uint64_t room, Counters* counters)
{
    seeds_body<false>(m1, m2, paired, owner, n, D, weak, keys, vals, room, counters, Tags{});
}

__global__ __launch_bounds__(kBlock)
void seeds_umi_kernel(Mate m1, Mate m2, bool paired, const uint32_t* __restrict__ owner, uint64_t n, uint32_t D, bool weak, uint64_t* __restrict__ keys,
                      uint32_t* __restrict__ vals, uint64_t room, Counters* counters, Tags tags)
{
    seeds_body<true>(m1, m2, paired, owner, n, D, weak, keys, vals, room, counters, tags);
}

// ---- links -------------------------------------------------------------------------------------------------------------------

// FQD_FAST_UMI_HAMMING with links: the nodes whose link is not themselves, and the links that are above their node or name no
// node (fqdnearumi::link_is_good), held against the rule before anything is written.
__global__ __launch_bounds__(kBlock)
void count_links_kernel(const uint32_t* __restrict__ owner, const uint32_t* __restrict__ link, uint64_t n, Counters* counters)
{
    unsigned long long links = 0, bad = 0;
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
        if (owner[i] != uint32_t(i)) continue;
        const uint32_t l = link[i];
        if (l == uint32_t(i)) continue;
        ++links;
        bad += !fqdnearumi::link_is_good(owner, uint32_t(i), l);     // (l <= i < n is looked at first: no load outside owner)
    }
    links = wave_sum(links); bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0) {
        if (links) atomicAdd(&counters->links, links);
        if (bad) atomicAdd(&counters->bad, bad);
    }
}

// (link[v], v) of every node v with link[v] != v goes to the edge list, a wave adding to its end with one atomic; the launch
// stands in front of the verification in the stream, so the links lie in front of the near edges.  A lane a record, no stride.
__global__ __launch_bounds__(kBlock)
void links_kernel(const uint32_t* __restrict__ owner, const uint32_t* __restrict__ link, uint64_t n, uint2* __restrict__ edges, unsigned long long room,
                  Counters* counters)
{
    const uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x;
    uint32_t l = 0;
    bool has = i < n && owner[i] == uint32_t(i);
    if (has) { l = link[i]; has = l != uint32_t(i); }
    const unsigned long long at = fqdwave::ballot_append(has, &counters->edges);
    if (has && at < room) edges[at] = make_uint2(l, uint32_t(i));
}

// ---- groups ------------------------------------------------------------------------------------------------------------------

// group_end over the sorted keys: fqd_groups_core.hpp; the pass that marks the groups: fqd_groups.hpp.
using fqdgroups::group_end;

// A lane an entry, no stride (fqdgroups::mark_groups).  work: room for N places — the entries that have a later entry in their group.
__global__ __launch_bounds__(kBlock)
void mark_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t N, uint64_t* __restrict__ work, Counters* counters)
{
    fqdgroups::mark_groups<kMaxGroup>(keys, vals, N, blockIdx.x * uint64_t(kBlock) + threadIdx.x, work, counters);
}

// ---- verify ------------------------------------------------------------------------------------------------------------------

// The differing bytes of a and b (n each), counted by the group's lanes until the sum is above D; all eight lanes return the
// sum.  on: the group has a pair to compare (the loop's condition is the wave's, see the head of the file).
__device__ __forceinline__ uint32_t lanes_count(bool on, const uint8_t* a, const uint8_t* b, uint32_t n, uint32_t D, uint32_t gl)
{
    uint32_t d = 0;
    for (uint32_t c0 = 0; __any(on && uint64_t(c0) * kChunk < n && d <= D); c0 += kLanes) {
        const bool go = on && uint64_t(c0) * kChunk < n && d <= D;
        d += fqdwave::group_sum<kLanes>(go ? chunk_mismatches(a, b, n, c0 + gl) : 0u);
    }
    return d;
}

// Eight lanes an entry of the work list (W places of entries below N), no stride.  edges: room pairs (a, b).  kTagged: lane gl
// holds word gl of the entry's tag and compares it with the candidate's, and the group's vote rejects the pair before the
// shapes and the mates are looked at (fqdnearumi::tags_differ).
template <bool kTagged>
__device__ __forceinline__ void verify_body(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t N, const uint64_t* __restrict__ work,
                                            uint64_t W, const Mate& m1, const Mate& m2, bool paired, uint32_t D, uint2* __restrict__ edges,
                                            unsigned long long room, Counters* counters, const Tags& tags)
{
    const uint32_t lane = threadIdx.x & 63u, gl = lane % kLanes;
    const uint64_t w = (blockIdx.x * uint64_t(kBlock) + threadIdx.x) / kLanes;
    uint64_t e = 0, end = 0;
    uint32_t a = 0, len1 = 0, len2 = 0;
    uint64_t tag_a = 0;
    const uint8_t *a1 = m1.bases, *a2 = m1.bases;
    if (w < W) e = work[w];
    if (w < W && e < N) {
        end = group_end(keys, N, e);
        a = vals[e]; len1 = m1.length(a); a1 = m1.at(a);
        if (paired) { len2 = m2.length(a); a2 = m2.at(a); }
        if constexpr (kTagged) tag_a = fqdnearumi::tag_word(tags.at(a), tags.umi_len, tags.joiners, gl);
    }
    unsigned long long pairs = 0;
    for (uint64_t c = e + 1; __any(c < end); ++c) {
        bool on = c < end;
        uint32_t b = 0;
        const uint8_t *b1 = a1, *b2 = a2;
        if (on) b = vals[c];
        on = on && b != a;                                   // an entry of the same node (its own keys collided)
        pairs += on && gl == 0u;
        if constexpr (kTagged) {
            uint32_t differs = 0;
            if (on) differs = fqdnearumi::tag_word(tags.at(b), tags.umi_len, tags.joiners, gl) != tag_a;
            on = on && fqdwave::group_sum<kLanes>(differs) == 0u;             // (called by every lane)
        }
        if (on) on = m1.length(b) == len1 && (!paired || m2.length(b) == len2);
        if (on) { b1 = m1.at(b); if (paired) b2 = m2.at(b); }
        const uint32_t d1 = lanes_count(on, a1, b1, len1, D, gl);   // (called by every lane: its loops vote)
        on = on && d1 <= D;
        if (paired) { const uint32_t d2 = lanes_count(on, a2, b2, len2, D, gl); on = on && d2 <= D; }
        if (on && gl == 0u) {
            const unsigned long long at = atomicAdd(&counters->edges, 1ull);
            if (at < room) edges[at] = make_uint2(a, b);
        }
    }
    pairs = wave_sum(pairs);
    if (lane == 0 && pairs) atomicAdd(&counters->pairs, pairs);
}

__global__ __launch_bounds__(kBlock)
void verify_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t N, const uint64_t* __restrict__ work, uint64_t W, Mate m1,
                   Mate m2, bool paired, uint32_t D, uint2* __restrict__ edges, unsigned long long room, Counters* counters)
{
    verify_body<false>(keys, vals, N, work, W, m1, m2, paired, D, edges, room, counters, Tags{});
}

__global__ __launch_bounds__(kBlock)
void verify_umi_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t N, const uint64_t* __restrict__ work, uint64_t W, Mate m1,
                       Mate m2, bool paired, uint32_t D, uint2* __restrict__ edges, unsigned long long room, Counters* counters, Tags tags)
{
    verify_body<true>(keys, vals, N, work, W, m1, m2, paired, D, edges, room, counters, tags);
}

// ---- sweeps ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void start_labels_kernel(uint32_t* __restrict__ labels, uint64_t n)
{
    for (uint64_t v = blockIdx.x * uint64_t(kBlock) + threadIdx.x; v < n; v += uint64_t(gridDim.x) * kBlock) labels[v] = uint32_t(v);
}

// The min step; next is a copy of labels when the launch begins.  Every edge's ends are nodes below n (verify wrote them
// from the entry list, which holds records below n).
__global__ __launch_bounds__(kBlock)
void edge_min_kernel(const uint2* __restrict__ edges, uint64_t m, const uint32_t* __restrict__ labels, uint32_t* __restrict__ next, uint32_t* changed)
{
    bool any = false;
    for (uint64_t k = blockIdx.x * uint64_t(kBlock) + threadIdx.x; k < m; k += uint64_t(gridDim.x) * kBlock) {
        const uint2 ed = edges[k];
        uint32_t to, low;
        if (!edge_min(labels, ed.x, ed.y, &to, &low)) continue;
        atomicMin(&next[to], low);
        any = true;
    }
    if (any) *changed = 1u;                                   // (every writer writes the same value)
}

__global__ __launch_bounds__(kBlock)
void jump_kernel(const uint32_t* __restrict__ next, uint32_t* __restrict__ labels, uint64_t n)
{
    for (uint64_t v = blockIdx.x * uint64_t(kBlock) + threadIdx.x; v < n; v += uint64_t(gridDim.x) * kBlock) labels[v] = next[next[v]];
}

__global__ __launch_bounds__(kBlock)
void finish_kernel(const uint32_t* __restrict__ owner, const uint32_t* __restrict__ labels, uint64_t n, uint32_t* __restrict__ owner_out, Counters* counters)
{
    unsigned long long merged = 0;
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
        const uint32_t o = owner[i], l = labels[o];
        owner_out[i] = l;
        merged += o == i && l == o;
    }
    merged = wave_sum(merged);
    if ((threadIdx.x & 63) == 0 && merged) atomicAdd(&counters->merged, merged);
}

struct Buffers { uint64_t* keys[2]; uint32_t* vals[2]; uint32_t *counts, *tot, *labels; };

size_t carve(uint64_t n, uint64_t N, char* base, Buffers& b)
{
    Carver c{base};
    for (int k = 0; k < 2; ++k) { b.keys[k] = c.take<uint64_t>(N); b.vals[k] = c.take<uint32_t>(N); }
    b.counts = c.take<uint32_t>(fqd_internal_radix_counts(N)); b.tot = c.take<uint32_t>(256);
    b.labels = c.take<uint32_t>(n);
    return c.used + 256;
}

// Counters in front, the edges behind them.
constexpr size_t kEdgesAt = 256;
static_assert(sizeof(Counters) <= kEdgesAt, "the counters fit in front of the edges");

// FQD_NEAR_EDGE_ROOM=K (tests): the edge list starts with room for K edges, so that a small input goes through the regrowth.
unsigned long long first_edge_room(uint64_t N)
{
    if (const char* v = std::getenv("FQD_NEAR_EDGE_ROOM")) { const long long k = std::atoll(v); if (k > 0) return static_cast<unsigned long long>(k); }
    return std::max<unsigned long long>(N, 1024);
}

// Both entries.  name: "fqd_near_merge" / "fqd_near_merge_umi", for the messages.  tags (fqd_near_merge_umi; its arrays are
// checked by the caller): the tagged seeds and verification are launched in place of the untagged ones; link (with tags
// only, may be null): the links are held against their rule, counted into *links and stand in front of the near edges.
// Without tags the launches and their arguments are fqd_near_merge's as they always were.
int merge(fqd_engine* e, const char* name, const fqd_reads* reads, const uint32_t* owner, const uint32_t* link, uint64_t n, uint32_t distance, uint32_t flags,
          const Tags* tags, uint32_t* owner_out, fqd_near_info* out, uint64_t* links)
{
    auto fail = [&](int code, const char* text) { return fqd_internal_fail(e, code, (std::string(name) + text).c_str()); };
    const int S = fqd_internal_segments(e);
    bool fine = out && distance >= 1 && distance <= kMaxDistance && n < 0x80000000ull && !(flags & ~FQD_NEAR_WEAK_SEEDS) && (n == 0 || (reads && owner && owner_out));
    for (int s = 0; fine && n && s < S; ++s)
        fine = reads[s].bases && (reads[s].offsets == nullptr) == (reads[s].lengths == nullptr) && (reads[s].offsets || reads[s].uniform_stride >= reads[s].uniform_len);
    if (!fine)
        return fail(FQD_ERR_ARG, ": bad arguments (the info, a distance of 1 .. 3, no flag but FQD_NEAR_WEAK_SEEDS, the engine's segments as fqd_reads — offsets and lengths both or neither — the owners and room for the merged owners of at most 2^31-1 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    bool device = all_on_device(owner, owner_out) && (!link || on_device(link));
    for (int s = 0; s < S; ++s) device = device && on_device(reads[s].bases) && (!reads[s].offsets || all_on_device(reads[s].offsets, reads[s].lengths));
    if (!device) return fail(FQD_ERR_ARG, ": the reads and every array are device memory");
    const size_t words = size_t(n) * sizeof(uint32_t);
    bool overlaps = overlap(owner_out, words, owner, words) || overlap(owner_out, words, link, words);
    if (tags) overlaps = overlaps || overlap(owner_out, words, tags->id_start, 2 * words) || overlap(owner_out, words, tags->umi_off, words);
    for (int s = 0; s < S; ++s)
        overlaps = overlaps || overlap(owner_out, words, reads[s].offsets, 2 * words) || overlap(owner_out, words, reads[s].lengths, words) ||
                   (!reads[s].offsets && overlap(owner_out, words, reads[s].bases, size_t(n - 1) * reads[s].uniform_stride + reads[s].uniform_len));
    if (overlaps) return fail(FQD_ERR_ARG, ": owner_out overlaps an input");
    hipStream_t stream = fqd_internal_stream(e);
    StageTimer timer{out->stage_ms};
    const uint32_t D = distance;
    const bool paired = S == 2, weak = (flags & FQD_NEAR_WEAK_SEEDS) != 0;
    const Mate m1{reads[0].bases, reads[0].offsets, reads[0].lengths, reads[0].uniform_len, reads[0].uniform_stride};
    const Mate m2 = paired ? Mate{reads[1].bases, reads[1].offsets, reads[1].lengths, reads[1].uniform_len, reads[1].uniform_stride} : m1;

    // ---- seeds ----
    void* small = nullptr;
    int rc = fqd_internal_scratch(e, 1, kEdgesAt, &small);
    if (rc) return rc;
    Counters* counters = static_cast<Counters*>(small);
    Counters got{};
    FQD_TRY(e, zero_counters(counters, stream, &Counters::over));
    hipLaunchKernelGGL(count_nodes_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, stream, owner, n, counters);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, read_back(got, counters, stream));
    if (got.bad || got.nodes == 0 || got.nodes > n)
        return fail(FQD_ERR_ARG, ": an owner lies above its record or is not its own owner (is owner that of fqd_owners over these records? nothing was written)");
    uint64_t L = 0;
    if (link) {
        hipLaunchKernelGGL(count_links_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, stream, owner, link, n, counters);
        FQD_TRY(e, hipGetLastError());
        FQD_TRY(e, read_back(got, counters, stream));
        if (got.bad || got.links >= got.nodes)
            return fail(FQD_ERR_ARG, ": a node's link lies above it or names a record that is no node (is link fqd_umi_merge's owner_out over these owners? nothing was written)");
        *links = L = got.links;
    }
    const uint64_t nodes = got.nodes, N = nodes * (D + 1u);
    out->nodes = nodes; out->entries = N;
    Buffers b{};
    void* base = nullptr;
    if ((rc = fqd_internal_scratch(e, 0, carve(n, N, nullptr, b), &base))) return rc;
    (void)carve(n, N, static_cast<char*>(base), b);
    if (tags)
        hipLaunchKernelGGL(seeds_umi_kernel, dim3(uint32_t((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, m1, m2, paired, owner, n, D, weak, b.keys[0],
                           b.vals[0], N, counters, *tags);
    else
        hipLaunchKernelGGL(seeds_kernel, dim3(uint32_t((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, m1, m2, paired, owner, n, D, weak, b.keys[0], b.vals[0],
                           N, counters);
    FQD_TRY(e, hipGetLastError());

    // ---- sort, groups ----
    int cur = 0;
    if ((rc = fqd_internal_radix_sort(e, stream, b.keys, b.vals, b.counts, b.tot, N, 64u, &cur))) return rc;
    const uint64_t* keys = b.keys[cur];
    const uint32_t* vals = b.vals[cur];
    uint64_t* work = b.keys[cur ^ 1];                         // (the sort's other key array is free from here on)
    hipLaunchKernelGGL(mark_kernel, dim3(uint32_t((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, keys, vals, N, work, counters);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, read_back(got, counters, stream));
    if (got.cursor != N) return fail(FQD_ERR_HIP, ": internal error (the nodes counted and the nodes listed differ)");
    out->groups = got.groups; out->largest_group = got.largest;
    const uint64_t W = got.work;
    if (W > N) return fail(FQD_ERR_HIP, ": internal error (more entries with a successor than entries)");
    timer.mark(0);
    if (got.over != kNoOver) {                                // refused: owner_out stays unspecified
        out->over_limit_first = got.over >> 32;
        out->over_limit_nodes = got.over & 0xFFFFFFFFull;
        return FQD_OK;
    }

    // ---- verify ----
    unsigned long long room = first_edge_room(N);
    uint2* edges = nullptr;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if ((rc = fqd_internal_scratch(e, 1, kEdgesAt + size_t(room) * sizeof(uint2), &small))) return rc;
        counters = static_cast<Counters*>(small);               // (a larger block is a new one: the counters verify adds to start at 0 either way)
        edges = reinterpret_cast<uint2*>(static_cast<char*>(small) + kEdgesAt);
        FQD_TRY(e, zero_counters(counters, stream));
        if (L) hipLaunchKernelGGL(links_kernel, dim3(uint32_t((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, owner, link, n, edges, room, counters);
        if (W && tags)
            hipLaunchKernelGGL(verify_umi_kernel, dim3(uint32_t((W * kLanes + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, keys, vals, N,
                               static_cast<const uint64_t*>(work), W, m1, m2, paired, D, edges, room, counters, *tags);
        else if (W)
            hipLaunchKernelGGL(verify_kernel, dim3(uint32_t((W * kLanes + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, keys, vals, N,
                               static_cast<const uint64_t*>(work), W, m1, m2, paired, D, edges, room, counters);
        FQD_TRY(e, hipGetLastError());
        FQD_TRY(e, read_back(got, counters, stream));
        if (got.edges <= room) break;
        if (attempt) return fail(FQD_ERR_HIP, ": internal error (two runs of the verification count different edges)");
        room = got.edges;
    }
    const uint64_t m = got.edges;                               // (the links in front, the near edges behind them)
    if (m < L) return fail(FQD_ERR_HIP, ": internal error (fewer edges than links)");
    out->pairs = got.pairs; out->edges = m - L;
    timer.mark(1);

    // ---- sweeps ----
    uint32_t* next = owner_out;
    hipLaunchKernelGGL(start_labels_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, stream, b.labels, n);
    uint64_t sweeps = 0;
    for (; m && sweeps < nodes; ++sweeps) {
        FQD_TRY(e, hipMemsetAsync(&counters->changed, 0, sizeof(uint32_t), stream));
        FQD_TRY(e, hipMemcpyAsync(next, b.labels, words, hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL(edge_min_kernel, dim3(grid_for(m, kBlock, 8192)), dim3(kBlock), 0, stream, static_cast<const uint2*>(edges), m,
                           static_cast<const uint32_t*>(b.labels), next, &counters->changed);
        FQD_TRY(e, hipGetLastError());
        uint32_t changed = 0;
        FQD_TRY(e, read_back(changed, &counters->changed, stream));
        if (!changed) break;
        hipLaunchKernelGGL(jump_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, stream, static_cast<const uint32_t*>(next), b.labels, n);
    }
    hipLaunchKernelGGL(finish_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, stream, owner, static_cast<const uint32_t*>(b.labels), n, owner_out, counters);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, read_back(got, counters, stream));
    out->merged = got.merged; out->sweeps = sweeps;
    timer.mark(2);
    return FQD_OK;
}

} // namespace

extern "C" {

int fqd_near_merge(fqd_engine* e, const fqd_reads* reads, const uint32_t* owner, uint64_t n, uint32_t distance, uint32_t flags, uint32_t* owner_out,
                   fqd_near_info* out)
{
    if (!e) return FQD_ERR_ARG;
    if (out) { *out = fqd_near_info{}; out->over_limit_first = FQD_UMI_NO_RECORD; out->max_group = FQD_NEAR_MAX_GROUP; }
    return merge(e, "fqd_near_merge", reads, owner, nullptr, n, distance, flags, nullptr, owner_out, out, nullptr);
}

int fqd_near_merge_umi(fqd_engine* e, const fqd_reads* reads, const uint32_t* owner, const uint32_t* link, uint64_t n, uint32_t distance, uint32_t flags,
                       const uint8_t* text, const uint64_t* id_start, const uint32_t* umi_off, const fqd_umi_info* info, uint32_t* owner_out,
                       fqd_near_umi_info* out)
{
    if (!e) return FQD_ERR_ARG;
    if (out) { *out = fqd_near_umi_info{}; out->near.over_limit_first = FQD_UMI_NO_RECORD; out->near.max_group = FQD_NEAR_MAX_GROUP; }
    if (!out || !info || info->bad_record != FQD_UMI_NO_RECORD || info->umi_len < 1 || info->umi_len > fqdumi::kMaxUmi || (n && (!text || !id_start || !umi_off)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_near_merge_umi: bad arguments (the info, fqd_umi_find's text, ID starts, UMI offsets and its info with no record refused and a UMI of 1 .. 64 bytes)");
    if (n) {
        FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
        if (!all_on_device(text, id_start, umi_off))
            return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_near_merge_umi: the text, the ID starts and the UMI offsets are device memory");
    }
    const Tags tags{text, id_start, umi_off, info->umi_len, info->joiners};
    return merge(e, "fqd_near_merge_umi", reads, owner, link, n, distance, flags, &tags, owner_out, &out->near, &out->links);
}

} // extern "C"
