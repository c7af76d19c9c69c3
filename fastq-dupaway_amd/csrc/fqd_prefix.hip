// fqd_prefix.hip — FQD_FAST_PREFIX=L of the `--fast` mode (same library as fqd_engine.hip): the engine's exact clusters that
// are prefixes of another, over at least L bases a mate, go to the shortest such cluster, through a seed join instead of all
// pairs.  Rule and proofs: fqd_prefix_core.hpp.  Nothing in here is called unless the switch is set.
//
//   seeds    count_kernel counts the nodes (owner[i] == i), the eligible ones among them (every mate >= L) and the mates of
//            2^31 bytes or more, and holds the owners against their own rule; the counts come back to size the rest.
//            seeds_kernel, a lane a record: an eligible node takes one place of the entry list — a wave adds to the list's end
//            with one atomic — and writes (seed key, node), the key over the first L bytes of each mate, sixteen bytes a load
//            (fqdprefix::node_seed); every record's word of `best` starts as all ones.  In which order the nodes stand in the
//            list depends on scheduling; nothing behind the sort does.
//   sort     fqd_internal_radix_sort over the 64 key bits.  mark_kernel, a lane an entry, as in fqd_near.hip: the groups are
//            counted and the largest kept, a group beyond the limit offers (its node << 32 | size) to one 64-bit atomicMin, and
//            an entry that has a later entry in its group goes on the work list, which lies in the sort's other key array.
//   verify   verify_kernel, EIGHT LANES AN ENTRY OF THE WORK LIST: the later entries of its group are its candidates, one after
//            another.  The lengths decide who can be whose prefix (fqdprefix::direction); then the lanes compare the overlap —
//            the short node's length — of mate 1, sixteen bytes a lane and round (fqdprefix::chunk_differs), or across the
//            eight behind every round and stop at the first round with a difference; mate 2 likewise.  A related pair: the
//            group's first lane does atomicMin(&best[short], span(long) << 32 | long).  Every loop's condition is a wave-wide
//            vote, so the eight lanes of a group are together at every cross-lane or.
//   trees    start_kernel: up[v] = the low word of best[v] (v where there is none), the children counted, every child's chain
//            walked once for `deepest`.  jump_kernel: next[v] = up[up[v]], one array read and the other written (owner_out
//            serves as the second); the host ends at the first jump that changes nothing.  `best` is used up by then and its
//            bytes hold `first`: first_kernel does atomicMin(&first[root[v]], v) over the nodes, finish_kernel writes
//            owner_out[i] = first[root[owner[i]]] and span_out.
#include <hip/hip_runtime.h>

#include <string>

#include "fqd_groups.hpp"
#include "fqd_internal.hpp"
#include "fqd_prefix_core.hpp"
#include "fqd_wave.hpp"

namespace {

using namespace fqdprefix;
using fqdgroups::group_end;
using fqdwave::wave_max;
using fqdwave::wave_sum;

constexpr int kBlock = 256;
constexpr unsigned long long kNoOver = ~0ull;

static_assert(64 % kLanes == 0 && kLanes == 8, "the verify kernel's groups tile a wave");

struct Counters {
    unsigned long long nodes, bad, eligible, long_mates, cursor, groups, largest, work, pairs, related, merged, children, over;
    uint32_t deepest, changed;
};

// One mate's reads as the kernels see them (fqd_reads).
struct Mate {
    const uint8_t* bases; const uint64_t* off; const uint32_t* len; uint32_t ulen, ustride;
    __device__ __forceinline__ const uint8_t* at(uint32_t r) const { return off ? bases + off[r] : bases + uint64_t(r) * ustride; }
    __device__ __forceinline__ uint32_t length(uint32_t r) const { return len ? len[r] : ulen; }
};

// ---- seeds -------------------------------------------------------------------------------------------------------------------

// bad: an owner above its record (that covers one outside 0 .. n-1), or one that is not its own owner.  long_mates: the
// records with a mate of 2^31 bytes or more, whose span would not fit 32 bits.
__global__ __launch_bounds__(kBlock)
void count_kernel(Mate m1, Mate m2, bool paired, const uint32_t* __restrict__ owner, uint64_t n, uint32_t L, Counters* counters)
{
    unsigned long long nodes = 0, bad = 0, fit = 0, lng = 0;
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
        const uint32_t len1 = m1.length(uint32_t(i)), len2 = paired ? m2.length(uint32_t(i)) : 0u;
        lng += (len1 | len2) >= 0x80000000u;
        const uint32_t o = owner[i];
        if (o > i) { ++bad; continue; }
        nodes += o == i;
        fit += o == i && eligible(paired, len1, len2, L);
        bad += o != i && owner[o] != o;
    }
    nodes = wave_sum(nodes); bad = wave_sum(bad); fit = wave_sum(fit); lng = wave_sum(lng);
    if ((threadIdx.x & 63) == 0) {
        if (nodes) atomicAdd(&counters->nodes, nodes);
        if (bad) atomicAdd(&counters->bad, bad);
        if (fit) atomicAdd(&counters->eligible, fit);
        if (lng) atomicAdd(&counters->long_mates, lng);
    }
}

// A lane a record, no stride: every lane of a wave reaches the ballot.  room = the entries the lists hold.
__global__ __launch_bounds__(kBlock)
void seeds_kernel(Mate m1, Mate m2, bool paired, const uint32_t* __restrict__ owner, uint64_t n, uint32_t L, bool weak, uint64_t* __restrict__ keys,
                  uint32_t* __restrict__ vals, uint64_t room, uint64_t* __restrict__ best, Counters* counters)
{
    const uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x;
    const uint32_t r = uint32_t(i);
    bool mine = i < n && owner[i] == r;
    if (i < n) best[i] = kNoParent;
    if (mine) mine = eligible(paired, m1.length(r), paired ? m2.length(r) : 0u, L);
    const unsigned long long at = fqdwave::ballot_append(mine, &counters->cursor);
    if (!mine || at >= room) return;
    keys[at] = node_seed(paired, m1.at(r), paired ? m2.at(r) : nullptr, L, weak);
    vals[at] = r;
}

// ---- groups ------------------------------------------------------------------------------------------------------------------

// A lane an entry, no stride: fqd_groups.hpp.  work: room for N places — the entries that have a later entry in their group.
__global__ __launch_bounds__(kBlock)
void mark_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t N, uint64_t* __restrict__ work, Counters* counters)
{
    fqdgroups::mark_groups<kMaxGroup>(keys, vals, N, blockIdx.x * uint64_t(kBlock) + threadIdx.x, work, counters);
}

// ---- verify ------------------------------------------------------------------------------------------------------------------

// Do the first n bytes of a and b agree?  Compared by the group's lanes round by round, until a round finds a difference; all
// eight lanes return the answer.  on: the group has a pair to compare (the loop's condition is the wave's, see the head of
// the file); a group that is not on loads nothing.
__device__ __forceinline__ bool lanes_agree(bool on, const uint8_t* a, const uint8_t* b, uint32_t n, uint32_t gl)
{
    bool differs = false;
    for (uint32_t c0 = 0; __any(on && !differs && uint64_t(c0) * kChunk < n); c0 += kLanes) {
        const bool go = on && !differs && uint64_t(c0) * kChunk < n;
        const uint32_t mine = go && chunk_differs(a, b, n, c0 + gl) ? 1u : 0u;
        differs = fqdwave::group_or<kLanes>(mine) != 0u || differs;
    }
    return on && !differs;
}

// Eight lanes an entry of the work list (W places of entries below N), no stride.  best: a word a record.
__global__ __launch_bounds__(kBlock)
void verify_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t N, const uint64_t* __restrict__ work, uint64_t W, Mate m1,
                   Mate m2, bool paired, unsigned long long* __restrict__ best, Counters* counters)
{
    const uint32_t lane = threadIdx.x & 63u, gl = lane % kLanes;
    const uint64_t w = (blockIdx.x * uint64_t(kBlock) + threadIdx.x) / kLanes;
    uint64_t e = 0, end = 0;
    uint32_t a = 0, len1 = 0, len2 = 0;
    const uint8_t *a1 = m1.bases, *a2 = m1.bases;
    if (w < W) e = work[w];
    if (w < W && e < N) {
        end = group_end(keys, N, e);
        a = vals[e]; len1 = m1.length(a); a1 = m1.at(a);
        if (paired) { len2 = m2.length(a); a2 = m2.at(a); }
    }
    unsigned long long pairs = 0, related = 0;
    for (uint64_t c = e + 1; __any(c < end); ++c) {
        bool on = c < end;
        uint32_t b = 0, bl1 = 0, bl2 = 0;
        const uint8_t *b1 = a1, *b2 = a2;
        if (on) { b = vals[c]; bl1 = m1.length(b); if (paired) bl2 = m2.length(b); }
        const int dir = on ? direction(paired, len1, len2, bl1, bl2) : 0;
        on = dir != 0;                                           // (one shape, or opposite sides: nothing is compared)
        pairs += on && gl == 0u;
        if (on) { b1 = m1.at(b); if (paired) b2 = m2.at(b); }
        on = lanes_agree(on, a1, b1, dir == 1 ? len1 : bl1, gl);   // (called by every lane: its loop votes)
        if (paired) on = lanes_agree(on, a2, b2, dir == 1 ? len2 : bl2, gl);
        if (on && gl == 0u) {
            const uint32_t shorter = dir == 1 ? a : b, longer = dir == 1 ? b : a, span = dir == 1 ? bl1 + bl2 : len1 + len2;
            atomicMin(&best[shorter], static_cast<unsigned long long>(pack(span, longer)));
            ++related;
        }
    }
    pairs = wave_sum(pairs); related = wave_sum(related);
    if (lane == 0) {
        if (pairs) atomicAdd(&counters->pairs, pairs);
        if (related) atomicAdd(&counters->related, related);
    }
}

// ---- trees -------------------------------------------------------------------------------------------------------------------

// up[v] = v's parent, v itself where it has none (a record that is no node has none: its word is still all ones).
__global__ __launch_bounds__(kBlock)
void start_kernel(const uint64_t* __restrict__ best, uint64_t n, uint32_t* __restrict__ up, Counters* counters)
{
    unsigned long long children = 0;
    uint32_t deepest = 0;
    for (uint64_t v = blockIdx.x * uint64_t(kBlock) + threadIdx.x; v < n; v += uint64_t(gridDim.x) * kBlock) {
        const uint64_t b = best[v];
        up[v] = parent_of(b, uint32_t(v));
        if (!has_parent(b)) continue;
        ++children;
        const uint32_t depth = chain_depth(best, uint32_t(v));
        deepest = depth > deepest ? depth : deepest;
    }
    children = wave_sum(children); deepest = wave_max(deepest);
    if ((threadIdx.x & 63) == 0) {
        if (children) atomicAdd(&counters->children, children);
        if (deepest) atomicMax(&counters->deepest, deepest);
    }
}

__global__ __launch_bounds__(kBlock)
void jump_kernel(const uint32_t* __restrict__ up, uint32_t* __restrict__ next, uint64_t n, uint32_t* changed)
{
    bool any = false;
    for (uint64_t v = blockIdx.x * uint64_t(kBlock) + threadIdx.x; v < n; v += uint64_t(gridDim.x) * kBlock) {
        const uint32_t u = up[v], t = up[u];
        next[v] = t;
        any |= t != u;
    }
    if (any) *changed = 1u;                                   // (every writer writes the same value)
}

// first: a word a record, all ones when the launch begins.
__global__ __launch_bounds__(kBlock)
void first_kernel(const uint32_t* __restrict__ owner, const uint32_t* __restrict__ root, uint64_t n, uint32_t* __restrict__ first)
{
    for (uint64_t v = blockIdx.x * uint64_t(kBlock) + threadIdx.x; v < n; v += uint64_t(gridDim.x) * kBlock)
        if (owner[v] == uint32_t(v)) atomicMin(&first[root[v]], uint32_t(v));
}

// merged: the nodes that are their own root — the trees, and the nodes that are not eligible.
__global__ __launch_bounds__(kBlock)
void finish_kernel(Mate m1, Mate m2, bool paired, const uint32_t* __restrict__ owner, const uint32_t* __restrict__ root, const uint32_t* __restrict__ first,
                   uint64_t n, uint32_t* __restrict__ owner_out, uint32_t* __restrict__ span_out, Counters* counters)
{
    unsigned long long merged = 0;
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
        const uint32_t o = owner[i], r = root[o];
        owner_out[i] = first[r];
        if (span_out) span_out[i] = m1.length(uint32_t(i)) + (paired ? m2.length(uint32_t(i)) : 0u);
        merged += o == i && r == o;
    }
    merged = wave_sum(merged);
    if ((threadIdx.x & 63) == 0 && merged) atomicAdd(&counters->merged, merged);
}

struct Buffers { uint64_t* keys[2]; uint32_t* vals[2]; uint32_t *counts, *tot; uint64_t* best; uint32_t* up; };

size_t carve(uint64_t n, uint64_t N, char* base, Buffers& b)
{
    Carver c{base};
    for (int k = 0; k < 2; ++k) { b.keys[k] = c.take<uint64_t>(N); b.vals[k] = c.take<uint32_t>(N); }
    b.counts = c.take<uint32_t>(fqd_internal_radix_counts(N)); b.tot = c.take<uint32_t>(256);
    b.best = c.take<uint64_t>(n); b.up = c.take<uint32_t>(n);
    return c.used + 256;
}

int merge(fqd_engine* e, const fqd_reads* reads, const uint32_t* owner, uint64_t n, uint32_t L, uint32_t flags, uint32_t* owner_out, uint32_t* span_out,
          fqd_prefix_info* out)
{
    auto fail = [&](int code, const char* text) { return fqd_internal_fail(e, code, (std::string("fqd_prefix_merge") + text).c_str()); };
    const int S = fqd_internal_segments(e);
    bool fine = out && L >= kMinOverlap && L <= kMaxOverlap && n < 0x80000000ull && !(flags & ~FQD_PREFIX_WEAK_SEEDS) && (n == 0 || (reads && owner && owner_out));
    for (int s = 0; fine && n && s < S; ++s)
        fine = reads[s].bases && (reads[s].offsets == nullptr) == (reads[s].lengths == nullptr) && (reads[s].offsets || reads[s].uniform_stride >= reads[s].uniform_len) &&
               (reads[s].offsets || reads[s].uniform_len < 0x80000000u);
    if (!fine)
        return fail(FQD_ERR_ARG, ": bad arguments (the info, a minimum overlap of 1 .. 65535, no flag but FQD_PREFIX_WEAK_SEEDS, the engine's segments as fqd_reads — offsets and lengths both or neither, a uniform length below 2^31 — the owners and room for the merged owners of at most 2^31-1 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    bool device = all_on_device(owner, owner_out) && (!span_out || on_device(span_out));
    for (int s = 0; s < S; ++s) device = device && on_device(reads[s].bases) && (!reads[s].offsets || all_on_device(reads[s].offsets, reads[s].lengths));
    if (!device) return fail(FQD_ERR_ARG, ": the reads and every array are device memory");
    const size_t words = size_t(n) * sizeof(uint32_t);
    bool overlaps = overlap(owner_out, words, span_out, words);
    for (const uint32_t* written : {static_cast<const uint32_t*>(owner_out), static_cast<const uint32_t*>(span_out)}) {
        if (!written) continue;
        overlaps = overlaps || overlap(written, words, owner, words);
        for (int s = 0; s < S; ++s)
            overlaps = overlaps || overlap(written, words, reads[s].offsets, 2 * words) || overlap(written, words, reads[s].lengths, words) ||
                       (!reads[s].offsets && overlap(written, words, reads[s].bases, size_t(n - 1) * reads[s].uniform_stride + reads[s].uniform_len));
    }
    if (overlaps) return fail(FQD_ERR_ARG, ": owner_out or span_out overlaps an input or the other");
    hipStream_t stream = fqd_internal_stream(e);
    StageTimer timer{out->stage_ms};
    const bool paired = S == 2, weak = (flags & FQD_PREFIX_WEAK_SEEDS) != 0;
    const Mate m1{reads[0].bases, reads[0].offsets, reads[0].lengths, reads[0].uniform_len, reads[0].uniform_stride};
    const Mate m2 = paired ? Mate{reads[1].bases, reads[1].offsets, reads[1].lengths, reads[1].uniform_len, reads[1].uniform_stride} : m1;

    // ---- seeds ----
    void* small = nullptr;
    int rc = fqd_internal_scratch(e, 1, 256, &small);
    if (rc) return rc;
    static_assert(sizeof(Counters) <= 256, "the counters fit their block");
    Counters* counters = static_cast<Counters*>(small);
    Counters got{};
    FQD_TRY(e, zero_counters(counters, stream, &Counters::over));
    hipLaunchKernelGGL(count_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, stream, m1, m2, paired, owner, n, L, counters);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, read_back(got, counters, stream));
    if (got.bad || got.nodes == 0 || got.nodes > n)
        return fail(FQD_ERR_ARG, ": an owner lies above its record or is not its own owner (is owner that of fqd_owners over these records? nothing was written)");
    if (got.long_mates) return fail(FQD_ERR_ARG, ": a mate of 2^31 bytes or more (a record's span would not fit 32 bits; nothing was written)");
    if (got.eligible > got.nodes) return fail(FQD_ERR_HIP, ": internal error (more eligible nodes than nodes)");
    const uint64_t nodes = got.nodes, N = got.eligible;
    out->nodes = nodes; out->eligible = N;
    Buffers b{};
    void* base = nullptr;
    if ((rc = fqd_internal_scratch(e, 0, carve(n, N, nullptr, b), &base))) return rc;
    (void)carve(n, N, static_cast<char*>(base), b);
    hipLaunchKernelGGL(seeds_kernel, dim3(uint32_t((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, m1, m2, paired, owner, n, L, weak, b.keys[0], b.vals[0], N,
                       b.best, counters);
    FQD_TRY(e, hipGetLastError());

    // ---- sort, groups ----
    uint64_t W = 0;
    const uint64_t* keys = b.keys[0];
    const uint32_t* vals = b.vals[0];
    uint64_t* work = b.keys[1];
    if (N) {
        int cur = 0;
        if ((rc = fqd_internal_radix_sort(e, stream, b.keys, b.vals, b.counts, b.tot, N, 64u, &cur))) return rc;
        keys = b.keys[cur]; vals = b.vals[cur];
        work = b.keys[cur ^ 1];                                  // (the sort's other key array is free from here on)
        hipLaunchKernelGGL(mark_kernel, dim3(uint32_t((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, keys, vals, N, work, counters);
        FQD_TRY(e, hipGetLastError());
    }
    FQD_TRY(e, read_back(got, counters, stream));
    if (got.cursor != N) return fail(FQD_ERR_HIP, ": internal error (the eligible nodes counted and the nodes listed differ)");
    out->groups = got.groups; out->largest_group = got.largest;
    W = got.work;
    if (W > N) return fail(FQD_ERR_HIP, ": internal error (more entries with a successor than entries)");
    timer.mark(0);
    if (got.over != kNoOver) {                                // refused: owner_out and span_out stay unspecified
        out->over_limit_first = got.over >> 32;
        out->over_limit_nodes = got.over & 0xFFFFFFFFull;
        return FQD_OK;
    }

    // ---- verify ----
    if (W) {
        hipLaunchKernelGGL(verify_kernel, dim3(uint32_t((W * kLanes + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, keys, vals, N,
                           static_cast<const uint64_t*>(work), W, m1, m2, paired, reinterpret_cast<unsigned long long*>(b.best), counters);
        FQD_TRY(e, hipGetLastError());
    }
    FQD_TRY(e, read_back(got, counters, stream));
    out->pairs = got.pairs; out->related = got.related;
    timer.mark(1);

    // ---- trees ----
    uint32_t *up = b.up, *next = owner_out;
    hipLaunchKernelGGL(start_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, stream, static_cast<const uint64_t*>(b.best), n, up, counters);
    FQD_TRY(e, hipGetLastError());
    uint64_t jumps = 0;
    for (; jumps <= 32; ++jumps) {                            // (a jump doubles what a pointer spans: 2^31 records need 31)
        FQD_TRY(e, hipMemsetAsync(&counters->changed, 0, sizeof(uint32_t), stream));
        hipLaunchKernelGGL(jump_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, stream, static_cast<const uint32_t*>(up), next, n, &counters->changed);
        FQD_TRY(e, hipGetLastError());
        uint32_t changed = 0;
        FQD_TRY(e, read_back(changed, &counters->changed, stream));
        if (!changed) break;                                  // (up holds the roots, and so does next)
        std::swap(up, next);
    }
    if (jumps > 32) return fail(FQD_ERR_HIP, ": internal error (the parents do not form a forest)");
    uint32_t* first = reinterpret_cast<uint32_t*>(b.best);    // (start_kernel was best's last reader, and the stream has drained since)
    FQD_TRY(e, hipMemsetAsync(first, 0xFF, words, stream));
    hipLaunchKernelGGL(first_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, stream, owner, static_cast<const uint32_t*>(b.up), n, first);
    hipLaunchKernelGGL(finish_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, stream, m1, m2, paired, owner, static_cast<const uint32_t*>(b.up),
                       static_cast<const uint32_t*>(first), n, owner_out, span_out, counters);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, read_back(got, counters, stream));
    out->merged = got.merged; out->children = got.children; out->deepest = got.deepest; out->jumps = jumps;
    timer.mark(2);
    return FQD_OK;
}

} // namespace

extern "C" {

int fqd_prefix_merge(fqd_engine* e, const fqd_reads* reads, const uint32_t* owner, uint64_t n, uint32_t min_overlap, uint32_t flags, uint32_t* owner_out,
                     uint32_t* span_out, fqd_prefix_info* out)
{
    if (!e) return FQD_ERR_ARG;
    if (out) { *out = fqd_prefix_info{}; out->over_limit_first = FQD_UMI_NO_RECORD; out->max_group = FQD_PREFIX_MAX_GROUP; }
    return merge(e, reads, owner, n, min_overlap, flags, owner_out, span_out, out);
}

} // extern "C"
