// fqd_consensus.hip — FQD_FAST_CONSENSUS=1 of the `--fast` mode (same library as fqd_engine.hip): the sequence and quality lines
// of every cluster's written member replaced, where they lie in the text, by the cluster's column-wise consensus.  Rule and
// proofs: fqd_consensus_core.hpp.  Nothing in here is called unless the switch is set.
//
//   heads    fqd_clusters.hpp's: check_heads_kernel (tile_count) + scan_tiles_kernel + head_write_kernel.  check_heads_kernel's
//            own part: it holds every record's lines against lines_fit, every member's sequence length against the member in
//            front of it, and finds the longest sequence.  The counts come back; a bad one ends the call here, before any
//            store to the text.
//   classes  classify_kernel, a lane a cluster (cluster_at): a cluster of ONE member — most of them — is passed over; a longer
//            one goes on the list of its tier.  NOT through fqd_clusters.hpp's list_append: a block's waves count in LDS and the
//            block adds to a list with one atomic (a wave-wide atomic a list was this kernel's 3.43 ms).  The lists'
//            lengths come back for the grids.
//   votes    LANES RUN ALONG COLUMNS, kChunk = 4 columns a lane and load, and the members go one after the other within a lane:
//            a member's row is read by neighbouring lanes at neighbouring addresses.  A whole chunk is one 4-byte load a line;
//            the last, partial one goes byte by byte: no load leaves a read's line.  A lane keeps the states of its 4 columns
//            in registers (Sum32, bounded by the tier).
//            vote_lanes_kernel    SIXTEEN LANES A CLUSTER of up to `small` members, four clusters a wave, 64 columns a round.
//                                 The lanes of a group read the places of sixteen members at once — once for all rounds
//                                 where the cluster has no more — and hand them round.
//            vote_block_kernel    A WORKGROUP A CLUSTER of up to `block` members: wave w takes members w, w + 4, ..., 256
//                                 columns a round; the four waves' states meet in LDS, and thread (w, lane) decides column
//                                 4 * lane + w of the round.
//            vote_block_kernel<many>, finish_many_kernel    a cluster ABOVE `block`: ceil(members / share) workgroups, each
//                                 with every 4 * workgroups-th member as above, add their 32-bit sums as 64-bit atomics, and
//                                 their masks with an atomic or, to 6 words a column in scratch; a launch of its own, a thread a
//                                 column, decides and stores.  One such cluster at a time, its place and size as arguments.
//
// EVERY STORE TO THE WRITTEN MEMBER'S ROW COMES AFTER THE LAST READ OF IT.  The row's bytes of column c are read only by the
// lanes that vote on c's chunk, in the round of c.  Lane groups: one lane reads a chunk — of every member, the written one among
// them — and then, in program order, stores it; no other lane touches those columns.  Workgroup: the four waves read the
// round's columns, write their states to LDS and meet at a barrier; the stores of the round stand behind it, and a later
// round reads other columns.  Many workgroups: every read is in vote_block_kernel<many>, every store in finish_many_kernel,
// which the stream starts when the first has ended.  Other clusters' rows are other records' bytes.
//
// No rocPRIM, hipCUB or Thrust; scratch is the engine's two blocks.
#include <hip/hip_runtime.h>

#include <vector>

#include "fqd_clusters.hpp"
#include "fqd_consensus_core.hpp"

namespace {

using namespace fqdconsensus;

constexpr int kBlock = fqdscan::kBlock;
constexpr uint32_t kGroup = 16;                              // lanes a small cluster
constexpr uint32_t kWaves = kBlock / 64;
constexpr uint32_t kRound = 64 * kChunk;                     // columns a wave and round
constexpr uint32_t kWords = kLetters + 1;                    // words of a column's state
constexpr uint32_t kMaxGroups = 2048;                        // workgroups of one cluster at most
static_assert((1ull << 31) / kMaxGroups <= kMax32, "a workgroup's share of a cluster below 2^31 members fits Sum32");

static_assert(kWaves == kChunk, "thread (w, lane) decides column kChunk * lane + w of a round: as many waves as columns a lane");
static_assert(kWaves * kWords * kRound * sizeof(uint32_t) <= 64 * 1024, "the four waves' states of a round fit a workgroup's LDS");

using fqdclusters::entry_members;
using fqdclusters::entry_place;
using fqdwave::wave_max;
using fqdwave::wave_sum;

// The text and the record arrays of one file, and the order.
struct Rows { uint8_t* text; const uint32_t* perm; const uint64_t* start; const uint32_t* size; const uint64_t* seq_off; const uint32_t* seq_len; };

// What the kernels count (one in scratch, zeroed per call).
struct Counters {
    unsigned long long bad_place;                            // places whose record lies outside 0 .. n-1; place 0 without a head
    unsigned long long bad_lines;                            // records whose quality line does not lie behind the sequence line inside the record
    unsigned long long bad_len;                              // members whose sequence length is not that of the member in front
    unsigned long long clusters, members, bases_changed, reads_changed;
    uint32_t listed[3];                                      // clusters on the lanes', the workgroup's and the many-workgroups list
    uint32_t largest, longest;                               // members of the largest cluster; the longest sequence line
};

// ---- heads -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock)
void check_heads_kernel(Rows R, const uint8_t* __restrict__ head, uint64_t n, unsigned long long* __restrict__ tile_sum, Counters* counters)
{
    uint32_t bad_place = 0, bad_lines = 0, bad_len = 0, longest = 0;
    fqdclusters::tile_count<int(kWaves)>(n, tile_sum, [&](uint64_t k) __attribute__((always_inline)) {
        const bool h = head[k] != 0;
        const uint32_t r = R.perm[k];
        const bool lost = r >= n || (k == 0 && !h);
        uint32_t L = 0;
        bool lines = false, len = false;
        if (!lost) {
            L = R.seq_len[r];
            lines = !lines_fit(R.start[r], R.size[r], R.seq_off[r], L);
            if (!h) { const uint32_t before = R.perm[k - 1]; len = before < n && R.seq_len[before] != L; }
        }
        // (one add a count whatever the place was: counts that branches add to apart end up in private memory)
        bad_place += lost; bad_lines += lines; bad_len += len;
        longest = L > longest ? L : longest;
        return h;
    });
    bad_place = wave_sum(bad_place); bad_lines = wave_sum(bad_lines); bad_len = wave_sum(bad_len); longest = wave_max(longest);
    if ((threadIdx.x & 63) == 0) {
        if (bad_place) atomicAdd(&counters->bad_place, static_cast<unsigned long long>(bad_place));
        if (bad_lines) atomicAdd(&counters->bad_lines, static_cast<unsigned long long>(bad_lines));
        if (bad_len) atomicAdd(&counters->bad_len, static_cast<unsigned long long>(bad_len));
        if (longest) atomicMax(&counters->longest, longest);
    }
}

// ---- classes -----------------------------------------------------------------------------------------------------------------

struct Lists : fqdclusters::Lists<3> { uint32_t* many_len; };   // the lanes', the workgroup's and the many-workgroups list; the sequence length of every entry of of[2]

constexpr int kClassBlock = 1024;                            // clusters a block of classify_kernel

// The waves of a block take their places on the lists from counts in LDS, and the block takes its own with ONE global atomic
// a list (and one a counter): a wave-wide atomic a list on one address for every 64 clusters is what the kernel would wait for.
__global__ __launch_bounds__(kClassBlock)
void classify_kernel(const uint32_t* __restrict__ head_place, Rows R, uint64_t m, uint64_t n, Tiers tiers, Lists lists, Counters* counters)
{
    __shared__ uint32_t count[3], base[3], clusters_b, largest_b;
    __shared__ unsigned long long members_b;
    if (threadIdx.x < 3) count[threadIdx.x] = 0;
    if (threadIdx.x == 0) { clusters_b = 0; largest_b = 0; members_b = 0; }
    __syncthreads();
    const uint64_t c = blockIdx.x * uint64_t(kClassBlock) + threadIdx.x;   // (no stride: every lane of a wave reaches the ballots)
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t s = 0, k0 = 0;
    if (c < m) s = fqdclusters::cluster_at(head_place, m, n, c, &k0);
    const uint32_t cls = s < 2u ? 3u : s <= tiers.small ? 0u : s <= tiers.block ? 1u : 2u;
    uint32_t at = 0;                                         // the cluster's place among the block's of its class
#pragma unroll
    for (uint32_t t = 0; t < 3u; ++t) at += fqdwave::ballot_append(cls == t, &count[t]);
    const uint32_t clusters = uint32_t(__popcll(__ballot(cls != 3u)));
    const unsigned long long members = wave_sum<unsigned long long>(cls != 3u ? s : 0u);
    const uint32_t largest = wave_max(s);
    if (lane == 0) {
        if (clusters) { atomicAdd(&clusters_b, clusters); atomicAdd(&members_b, members); }
        if (largest) atomicMax(&largest_b, largest);
    }
    __syncthreads();
    if (threadIdx.x < 3 && count[threadIdx.x]) base[threadIdx.x] = atomicAdd(&counters->listed[threadIdx.x], count[threadIdx.x]);
    if (threadIdx.x == 64) {
        if (clusters_b) { atomicAdd(&counters->clusters, static_cast<unsigned long long>(clusters_b)); atomicAdd(&counters->members, members_b); }
        if (largest_b) atomicMax(&counters->largest, largest_b);
    }
    __syncthreads();
    if (cls < 3u) {
        lists.of[cls][base[cls] + at] = fqdclusters::entry(k0, s);
        if (cls == 2u) lists.many_len[base[cls] + at] = R.seq_len[R.perm[k0]];
    }
}

// ---- votes -------------------------------------------------------------------------------------------------------------------

// One member's bytes of a lane's chunk (`width` columns of it lie inside the line) into the lane's states.
__device__ __forceinline__ void add_chunk(State32 (&st)[kChunk], const uint8_t* __restrict__ seq, const uint8_t* __restrict__ qual, uint32_t width)
{
    if (width == kChunk) {
        uint32_t b, q;
        __builtin_memcpy(&b, seq, kChunk); __builtin_memcpy(&q, qual, kChunk);
#pragma unroll
        for (uint32_t e = 0; e < kChunk; ++e) add(st[e], uint8_t(b >> (8u * e)), uint8_t(q >> (8u * e)));
    } else {
#pragma unroll
        for (uint32_t e = 0; e < kChunk; ++e) if (e < width) add(st[e], seq[e], qual[e]);
    }
}

// A decided column into the written member's lines; returns whether its letter changed.
__device__ __forceinline__ uint32_t store_column(const Verdict& v, uint8_t* seq, uint8_t* qual)
{
    if (v.changed) *seq = byte_of(v.letter);
    *qual = v.quality;
    return v.changed ? 1u : 0u;
}

// A written record with a changed column: counted once a record whatever the call (see fqdupaway.h, `changed`).
__device__ __forceinline__ void mark_read(uint32_t record, uint8_t* changed, Counters* counters)
{
    bool fresh = true;
    if (changed) { fresh = changed[record] == 0; changed[record] = 1; }
    if (fresh) atomicAdd(&counters->reads_changed, 1ull);
}

// Sixteen lanes a cluster; see the head of the file.
__global__ __launch_bounds__(kBlock)
void vote_lanes_kernel(const unsigned long long* __restrict__ list, uint32_t n_items, Rows R, uint32_t limit, uint8_t* changed, Counters* counters)
{
    const uint32_t lane = threadIdx.x & 63u, gl = lane % kGroup;
    const uint64_t item = (blockIdx.x * uint64_t(kBlock) + threadIdx.x) / kGroup;
    uint32_t m = 0;
    uint64_t k0 = 0;
    if (item < n_items) { const unsigned long long e = list[item]; k0 = entry_place(e); m = entry_members(e); }
    if (m > limit) m = 0;                                    // (no list holds such an entry)
    uint32_t written = 0, L = 0;
    unsigned long long own_seq = 0, own_qual = 0;
    if (m) {
        written = R.perm[k0]; L = R.seq_len[written];
        own_seq = R.seq_off[written]; own_qual = quality_at(R.start[written], R.size[written], L);
    }
    // (m and L are the group's: its lanes stay together.)  Up to sixteen members — nearly every cluster — have their places
    // read once, a lane a member, for all rounds
    const bool few = m <= kGroup;
    unsigned long long seq_few = 0, qual_few = 0;
    if (few && gl < m) {
        const uint32_t r = R.perm[k0 + gl];
        seq_few = R.seq_off[r]; qual_few = quality_at(R.start[r], R.size[r], L);
    }
    uint32_t n_changed = 0;
    for (uint32_t c0 = 0; uint64_t(c0) * kChunk < L; c0 += kGroup) {
        const uint64_t col = uint64_t(c0 + gl) * kChunk;
        const uint32_t width = col >= L ? 0u : uint32_t(L - col < kChunk ? L - col : kChunk);
        State32 st[kChunk];
#pragma unroll
        for (uint32_t e = 0; e < kChunk; ++e) clear(st[e]);
        for (uint32_t i0 = 0; i0 < m; i0 += kGroup) {
            unsigned long long seq_at = seq_few, qual_at = qual_few;
            if (!few && i0 + gl < m) {
                const uint32_t r = R.perm[k0 + i0 + gl];
                seq_at = R.seq_off[r]; qual_at = quality_at(R.start[r], R.size[r], L);
            }
            const uint32_t count = m - i0 < kGroup ? m - i0 : kGroup;
            for (uint32_t j = 0; j < count; ++j) {
                const unsigned long long s_j = __shfl(seq_at, int(j), int(kGroup)), q_j = __shfl(qual_at, int(j), int(kGroup));
                if (width) add_chunk(st, R.text + s_j + col, R.text + q_j + col, width);
            }
        }
        // the lane's own columns of the written member: read (add_chunk above, and here), then stored
        uint8_t own[kChunk];
#pragma unroll
        for (uint32_t e = 0; e < kChunk; ++e) own[e] = e < width ? R.text[own_seq + col + e] : uint8_t(0);
#pragma unroll
        for (uint32_t e = 0; e < kChunk; ++e)
            if (e < width) n_changed += store_column(decide(st[e], own[e]), R.text + own_seq + col + e, R.text + own_qual + col + e);
    }
    const uint32_t any = fqdwave::group_or<int(kGroup)>(n_changed);
    if (m && gl == 0u && any) mark_read(written, changed, counters);
    n_changed = wave_sum(n_changed);
    if (lane == 0 && n_changed) atomicAdd(&counters->bases_changed, static_cast<unsigned long long>(n_changed));
}

// A workgroup a cluster (kMany: a share of the one cluster at k0 with m members); see the head of the file.
// columns (kMany): kWords 64-bit words a column, zeroed in front of the launch.
template <bool kMany>
__global__ __launch_bounds__(kBlock)
void vote_block_kernel(const unsigned long long* __restrict__ list, Rows R, uint64_t k0, uint32_t m, uint32_t limit, unsigned long long* __restrict__ columns,
                       uint8_t* changed, Counters* counters)
{
    __shared__ uint32_t part[kWaves][kWords][kChunk][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (!kMany) {
        const unsigned long long e = list[blockIdx.x];
        k0 = entry_place(e); m = entry_members(e);
        if (m > limit) m = 0;                                // (no list holds such an entry)
    }
    // this wave's members: first, first + stride, ... below m; a workgroup's are at most `share` <= kMax32 of them (Sum32)
    const uint64_t first = (kMany ? uint64_t(blockIdx.x) * kWaves : 0u) + wave, stride = uint64_t(kWaves) * (kMany ? gridDim.x : 1u);
    uint32_t written = 0, L = 0;
    unsigned long long own_seq = 0, own_qual = 0;
    if (m) {
        written = R.perm[k0]; L = R.seq_len[written];
        own_seq = R.seq_off[written]; own_qual = quality_at(R.start[written], R.size[written], L);
    }
    uint32_t n_changed = 0;
    for (uint64_t col0 = 0; col0 < L; col0 += kRound) {                     // (the same for every thread of the workgroup)
        const uint64_t col = col0 + uint64_t(lane) * kChunk;
        const uint32_t width = col >= L ? 0u : uint32_t(L - col < kChunk ? L - col : kChunk);
        State32 st[kChunk];
#pragma unroll
        for (uint32_t e = 0; e < kChunk; ++e) clear(st[e]);
        for (uint64_t from = first; from < m; from += 64u * stride) {      // (the same for every lane of the wave)
            const uint64_t mine = from + uint64_t(lane) * stride;
            unsigned long long seq_at = 0, qual_at = 0;
            if (mine < m) {
                const uint32_t r = R.perm[k0 + mine];
                seq_at = R.seq_off[r]; qual_at = quality_at(R.start[r], R.size[r], L);
            }
            const uint64_t left = (m - from + stride - 1u) / stride;
            const uint32_t count = left < 64u ? uint32_t(left) : 64u;
            for (uint32_t j = 0; j < count; ++j) {
                const unsigned long long s_j = __shfl(seq_at, int(j), 64), q_j = __shfl(qual_at, int(j), 64);
                if (width) add_chunk(st, R.text + s_j + col, R.text + q_j + col, width);
            }
        }
#pragma unroll
        for (uint32_t e = 0; e < kChunk; ++e) {
#pragma unroll
            for (uint32_t x = 0; x < kLetters; ++x) part[wave][x][e][lane] = st[e].s[x];
            part[wave][kLetters][e][lane] = st[e].mask;
        }
        __syncthreads();                                     // (every read of the round's columns lies in front of this)
        State32 sum;
        clear(sum);
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            State32 one;
#pragma unroll
            for (uint32_t x = 0; x < kLetters; ++x) one.s[x] = part[w][x][wave][lane];
            one.mask = part[w][kLetters][wave][lane];
            combine(sum, one);
        }
        const uint64_t c = col0 + uint64_t(lane) * kChunk + wave;
        if (c < L) {
            if (kMany) {
                unsigned long long* at = columns + c * kWords;
#pragma unroll
                for (uint32_t x = 0; x < kLetters; ++x) if (sum.s[x]) atomicAdd(at + x, static_cast<unsigned long long>(sum.s[x]));
                if (sum.mask) atomicOr(at + kLetters, static_cast<unsigned long long>(sum.mask));
            } else {
                n_changed += store_column(decide(sum, R.text[own_seq + c]), R.text + own_seq + c, R.text + own_qual + c);
            }
        }
        __syncthreads();                                     // (the states are read: the next round may write its own)
    }
    if (kMany) return;
    const int any = __syncthreads_or(int(n_changed));
    if (threadIdx.x == 0 && m && any) mark_read(written, changed, counters);
    n_changed = wave_sum(n_changed);
    if (lane == 0 && n_changed) atomicAdd(&counters->bases_changed, static_cast<unsigned long long>(n_changed));
}

// A thread a column of the one cluster at k0; marked: a word, zeroed in front of the launch.
__global__ __launch_bounds__(kBlock)
void finish_many_kernel(Rows R, uint64_t k0, const unsigned long long* __restrict__ columns, uint32_t* marked, uint8_t* changed, Counters* counters)
{
    const uint32_t written = R.perm[k0], L = R.seq_len[written];
    const unsigned long long own_seq = R.seq_off[written], own_qual = quality_at(R.start[written], R.size[written], L);
    const uint64_t c = blockIdx.x * uint64_t(kBlock) + threadIdx.x;
    uint32_t n_changed = 0;
    if (c < L) {
        State64 sum;
#pragma unroll
        for (uint32_t x = 0; x < kLetters; ++x) sum.s[x] = columns[c * kWords + x];
        sum.mask = uint32_t(columns[c * kWords + kLetters]);
        n_changed = store_column(decide(sum, R.text[own_seq + c]), R.text + own_seq + c, R.text + own_qual + c);
    }
    const int any = __syncthreads_or(int(n_changed));
    if (threadIdx.x == 0 && any && atomicExch(marked, 1u) == 0u) mark_read(written, changed, counters);
    n_changed = wave_sum(n_changed);
    if ((threadIdx.x & 63) == 0 && n_changed) atomicAdd(&counters->bases_changed, static_cast<unsigned long long>(n_changed));
}

struct VoteBuffers { uint32_t* head_place; Lists lists; unsigned long long* columns; uint32_t* marked; };

size_t carve_votes(uint64_t n, uint64_t m, uint32_t longest, const Tiers& tiers, char* base, VoteBuffers& b)
{
    Carver c{base};
    b.head_place = c.take<uint32_t>(m);
    fqdclusters::take_lists<3>(c, n, {1u, tiers.small, tiers.block}, b.lists);
    b.lists.many_len = c.take<uint32_t>(fqdclusters::list_room(n, tiers.block));
    b.columns = c.take<unsigned long long>(n > tiers.block ? size_t(longest) * kWords : 0);
    b.marked = c.take<uint32_t>(1);
    return c.used + 256;
}

} // namespace

extern "C" {

int fqd_consensus(fqd_engine* e, const uint32_t* perm, const uint8_t* head, uint64_t n, uint8_t* text, const uint64_t* start, const uint32_t* size,
                  const uint64_t* seq_off, const uint32_t* seq_len, uint32_t flags, uint8_t* changed, fqd_consensus_info* info)
{
    if (!e) return FQD_ERR_ARG;
    if (info) *info = fqd_consensus_info{0, 0, 0, 0, 0};
    if (!info || n >= 0x80000000ull || (flags & ~FQD_CONSENSUS_SMALL_TIERS) || (n && (!perm || !head || !text || !start || !size || !seq_off || !seq_len)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_consensus: bad arguments (the info, flags of 0 or FQD_CONSENSUS_SMALL_TIERS, the order and its head flags, the text, and the starts, sizes, sequence offsets and sequence lengths of at most 2^31-1 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(perm, head, text, start, size, seq_off, seq_len) || (changed && !on_device(changed)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_consensus: the text and every array are device memory");
    hipStream_t stream = fqd_internal_stream(e);
    const Tiers tiers = flags & FQD_CONSENSUS_SMALL_TIERS ? kSmallTiers : kTiers;
    const Rows R{text, perm, start, size, seq_off, seq_len};

    // ---- heads, and everything that can refuse the call ----
    TileScratch<Counters> slot;
    int rc = slot.reserve(e, fqdclusters::tiles_of(n), stream);
    if (rc) return rc;
    Counters* counters = slot.counters;
    unsigned long long m = 0;
    Counters got{};
    bool fits = false;
    rc = fqdclusters::count_heads(e, stream, slot, n, [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(check_heads_kernel, grid, block, 0, stream, R, head, n, slot.tile_sum, counters);
    }, &m, &got, &fits);
    if (rc) return rc;
    if (got.bad_place || !fits)
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_consensus: head[0] is not set, or the order names a record outside 0 .. n-1 (are perm and head those of fqd_group_owners over these records? nothing was written)");
    if (got.bad_lines)
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_consensus: a record's quality line, seq_len bytes at start + size - 1 - seq_len, does not lie behind its sequence line inside the record (FASTQ records only; nothing was written)");
    if (got.bad_len)
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_consensus: the members of a cluster differ in their sequence lengths (nothing was written)");

    // ---- classes ----
    VoteBuffers b{};
    void* base = nullptr;
    if ((rc = fqd_internal_scratch(e, 0, carve_votes(n, m, got.longest, tiers, nullptr, b), &base))) return rc;
    (void)carve_votes(n, m, got.longest, tiers, static_cast<char*>(base), b);
    fqdclusters::write_heads(stream, slot, head, n, m, b.head_place);
    hipLaunchKernelGGL(classify_kernel, dim3(uint32_t((m + kClassBlock - 1) / kClassBlock)), dim3(kClassBlock), 0, stream, static_cast<const uint32_t*>(b.head_place), R,
                       uint64_t(m), n, tiers, b.lists, counters);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, read_back(got, counters, stream));
    std::vector<unsigned long long> many(got.listed[2]);
    std::vector<uint32_t> many_len(got.listed[2]);
    if (!many.empty()) {
        FQD_TRY(e, hipMemcpyAsync(many.data(), b.lists.of[2], many.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        FQD_TRY(e, hipMemcpyAsync(many_len.data(), b.lists.many_len, many_len.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        FQD_TRY(e, hipStreamSynchronize(stream));
    }

    // ---- votes: sixteen lanes, a workgroup, many workgroups ----
    if (got.listed[0])
        hipLaunchKernelGGL(vote_lanes_kernel, dim3(uint32_t((uint64_t(got.listed[0]) * kGroup + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                           static_cast<const unsigned long long*>(b.lists.of[0]), got.listed[0], R, tiers.small, changed, counters);
    if (got.listed[1])
        hipLaunchKernelGGL(vote_block_kernel<false>, dim3(got.listed[1]), dim3(kBlock), 0, stream, static_cast<const unsigned long long*>(b.lists.of[1]), R,
                           uint64_t(0), 0u, tiers.block, static_cast<unsigned long long*>(nullptr), changed, counters);
    FQD_TRY(e, hipGetLastError());
    for (size_t k = 0; k < many.size(); ++k) {
        const uint64_t k0 = entry_place(many[k]);
        const uint32_t members = entry_members(many[k]), L = many_len[k];
        if (L == 0 || L > got.longest) continue;             // (no column; the second cannot be)
        // (a workgroup's members: every groups-th run of kWaves, at most max(share, 2^31 / kMaxGroups) = kMax32 of them)
        const uint32_t groups = std::min<uint32_t>((members + tiers.share - 1) / tiers.share, kMaxGroups);
        FQD_TRY(e, hipMemsetAsync(b.columns, 0, size_t(L) * kWords * sizeof(unsigned long long), stream));
        FQD_TRY(e, hipMemsetAsync(b.marked, 0, sizeof(uint32_t), stream));
        hipLaunchKernelGGL(vote_block_kernel<true>, dim3(groups), dim3(kBlock), 0, stream, static_cast<const unsigned long long*>(nullptr), R, k0, members,
                           0u, b.columns, changed, counters);
        hipLaunchKernelGGL(finish_many_kernel, dim3((L + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, R, k0, static_cast<const unsigned long long*>(b.columns),
                           b.marked, changed, counters);
        FQD_TRY(e, hipGetLastError());
    }
    FQD_TRY(e, read_back(got, counters, stream));
    *info = fqd_consensus_info{got.clusters, got.members, got.bases_changed, got.reads_changed, got.largest};
    return FQD_OK;
}

} // extern "C"
