// fqd_umi.hip — FQD_FAST_UMI=colon|underscore of the `--fast` mode (same library as fqd_engine.hip): every record's unique
// molecular identifier found in its ID line, and mate 1 packed as `UMI bases ‖ sequence` with descriptors the engine takes
// as they are.  Rule and proofs: fqd_umi_core.hpp.
//
//   find     umi_find_kernel: a wave takes a tile of 64 neighbouring records — their descriptors with one coalesced load a
//            lane — and works through it four records at a time, SIXTEEN LANES A RECORD, sixteen bytes a lane (the layout
//            of canon_kernel in fqd_strand.hip): a round covers 256 bytes of an ID line.  A lane turns its sixteen bytes
//            into two 16-bit masks, word ends and separators; the group takes the minimum over its lanes' first word end
//            and then the maximum over their last separator below it (four exchanges inside the sixteen lanes each).  Further
//            rounds run only while no lane of the group has seen the word's end.  The field behind the separator, at most
//            64 bytes, is classified four bytes a lane and collected with ballots into the joiner set; the verdict
//            compares it with record 0's shape, which a first launch over record 0 alone has left in scratch.  The
//            lowest refused record and its reason come back through one 64-bit atomicMin a wave of (record << 3 | reason).
//            Nothing is written besides umi_off and that word.
//   sizes    record_bytes_kernel + scan_tiles_kernel + record_offsets_kernel (fqd_record_scan.hpp, shared with
//            fqd_strand.hip): a record's bytes are Lb + len0, the Lb entering as a second, uniform "mate" of that length.
//   pack     umi_pack_kernel: sixteen lanes a record again.  The Lb bases go one byte a lane through a table of their
//            places in the field, passed by value: the shape is fixed, so taking the joiners out is a constant gather.
//            The sequence follows with fqdstrand::copy_lane: 16-byte loads and stores, the destination at any alignment.
#include <hip/hip_runtime.h>

#include "fqd_clusters_core.hpp"
#include "fqd_internal.hpp"
#include "fqd_record_scan.hpp"
#include "fqd_strand_core.hpp"
#include "fqd_umi_core.hpp"

namespace {

constexpr int kBlock = fqdscan::kBlock;
constexpr uint32_t kGroup = 16;                              // lanes a record
constexpr uint32_t kWaveTile = 64;                           // records a wave
constexpr uint32_t kTile = kWaveTile * (kBlock / 64);        // records a block of the two kernels
constexpr int kOffTile = fqdscan::kOffTile;                  // records a block of the scan's two passes
using fqdclusters::kNoBad;

using fqdscan::Mate;
using fqdscan::mate_off;
using fqdscan::mate_len;
using fqdscan::record_bytes_kernel;
using fqdscan::scan_tiles_kernel;
using fqdscan::record_offsets_kernel;

// What comes back from a find: the lowest (record << 3 | reason), and record 0's shape (ulen 0: record 0 is refused).
struct Found { unsigned long long bad; unsigned long long joiners; uint32_t ulen, reserved; };

// One wave per tile of kWaveTile records; see the head of the file.  define_shape: the launch over record 0 alone that
// leaves its shape in *found; every other launch compares with it.
__global__ __launch_bounds__(kBlock)
void umi_find_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ id_start, const uint32_t* __restrict__ id_len,
                     uint64_t n, uint32_t sep, int define_shape, Found* found, uint32_t* __restrict__ umi_off)
{
    const uint32_t lane = threadIdx.x & 63u, g = lane / kGroup, gl = lane % kGroup;
    const uint64_t tile0 = (uint64_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6)) * kWaveTile;
    if (tile0 >= n) return;                                  // (the whole wave)
    const uint64_t mine = tile0 + lane;
    unsigned long long line_at = 0;
    uint32_t line_len = 0;
    if (mine < n) { line_at = id_start[mine]; line_len = id_len[mine]; }
    const bool have0 = !define_shape;
    const uint32_t ulen0 = have0 ? found->ulen : 0u;
    const unsigned long long joiners0 = have0 ? found->joiners : 0ull;
    uint32_t my_off = 0, my_reason = 0;
    for (uint32_t j = 0; j < kWaveTile / 4u && tile0 + 4u * j < n; ++j) {
        const int r = int(4u * j + g);                       // the group's record of this step (beyond n: an empty line)
        const uint8_t* __restrict__ line = text + __shfl(line_at, r, 64);
        const uint32_t L = __shfl(line_len, r, 64);

        // ---- find (the lanes' looks: fqd_umi_core.hpp) ----
        const uint32_t chunks = fqdumi::line_chunks(L);
        uint32_t end = fqdumi::kNone, sep1 = 0;              // the word's end; 1 + the last separator's position
        for (uint32_t c0 = 0; __any(end == fqdumi::kNone && c0 < chunks); c0 += kGroup) {
            const bool live = end == fqdumi::kNone && c0 < chunks;
            fqdumi::Look k{0u, 0u, 0u};
            if (live) k = fqdumi::lane_look(line, L, uint8_t(sep), c0, gl);
            const uint32_t e = fqdwave::group_min<kGroup>(fqdumi::look_end(k));
            const uint32_t s = fqdwave::group_max<kGroup>(fqdumi::look_sep(k, e));
            if (live) { end = e; if (s) sep1 = s; }
        }
        if (end == fqdumi::kNone) end = L;                   // no word end in the line: the word ends with it

        // ---- class and verdict ----
        const bool has_sep = sep1 != 0;
        const uint32_t ulen = has_sep ? end - sep1 : 0u;
        uint32_t j4 = 0;
        bool bad_byte = false;
        if (has_sep && ulen <= fqdumi::kMaxUmi) fqdumi::lane_class(line + sep1, ulen, gl, &j4, &bad_byte);
        unsigned long long joiners = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
            joiners |= ((__ballot((j4 >> k) & 1u) >> (kGroup * g)) & 0xFFFFull) << (16u * k);
        const bool any_bad = ((__ballot(bad_byte) >> (kGroup * g)) & 0xFFFFull) != 0;
        const uint32_t reason = fqdumi::verdict(has_sep, ulen, joiners, any_bad, have0, ulen0, joiners0);
        if (define_shape && lane == 0) { found->ulen = reason ? 0u : ulen; found->joiners = reason ? 0ull : joiners; found->reserved = 0; }

        const uint32_t got_off = __shfl(sep1, int((lane & 3u) * kGroup), 64);
        const uint32_t got_reason = __shfl(reason, int((lane & 3u) * kGroup), 64);
        if ((lane >> 2) == j) { my_off = got_off; my_reason = got_reason; }   // record `lane` of the tile is group lane%4's at step lane/4
    }
    unsigned long long word = kNoBad;
    if (mine < n) {
        umi_off[mine] = my_off;
        if (my_reason) word = fqdclusters::bad_word(mine, my_reason);
    }
    word = fqdwave::wave_min(word);
    if (lane == 0 && word != kNoBad) atomicMin(&found->bad, word);
}

// One wave per tile of kWaveTile records, sixteen lanes a record.  rec_off = out_off as record_offsets_kernel left it.
__global__ __launch_bounds__(kBlock)
void umi_pack_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ id_start, const uint32_t* __restrict__ umi_off,
                     fqdumi::Table table, uint32_t lb, Mate m0, uint64_t n, uint8_t* __restrict__ out,
                     const uint64_t* __restrict__ rec_off, uint32_t* __restrict__ out_len)
{
    const uint32_t lane = threadIdx.x & 63u, g = lane / kGroup, gl = lane % kGroup;
    const uint64_t tile0 = (uint64_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6)) * kWaveTile;
    if (tile0 >= n) return;                                  // (the whole wave)
    const uint64_t mine = tile0 + lane;
    unsigned long long umi_at = 0, off_a = 0, base = 0;
    uint32_t len_a = 0;
    if (mine < n) { umi_at = id_start[mine] + umi_off[mine]; off_a = mate_off(m0, mine); len_a = mate_len(m0, mine); base = rec_off[mine]; }
    for (uint32_t j = 0; j < kWaveTile / 4u && tile0 + 4u * j < n; ++j) {
        const int r = int(4u * j + g);
        const uint8_t* __restrict__ U = text + __shfl(umi_at, r, 64);
        const uint8_t* __restrict__ a = m0.bases + __shfl(off_a, r, 64);
        const uint32_t la = __shfl(len_a, r, 64);
        uint8_t* __restrict__ dst = out + __shfl(base, r, 64);
        if (tile0 + uint32_t(r) < n) {                       // (the group; nothing in here crosses lanes)
            fqdumi::gather_lane(U, table, lb, dst, gl);
            fqdstrand::copy_lane(a, dst + lb, la, false, gl);
        }
    }
    if (mine < n) out_len[mine] = lb + len_a;
}

bool is_uniform(const fqd_reads& r) { return r.offsets == nullptr && r.lengths == nullptr; }

} // namespace

extern "C" {

int fqd_umi_find(fqd_engine* e, const uint8_t* text, const uint64_t* id_start, const uint32_t* id_len, uint64_t n, int sep,
                 uint32_t* umi_off, fqd_umi_info* info)
{
    if (!e) return FQD_ERR_ARG;
    if (info) *info = fqd_umi_info{0, 0, 0, FQD_UMI_NO_RECORD, FQD_UMI_OK, 0};
    if (!info || (sep != ':' && sep != '_') || n > 0xFFFFFFFEull || (n && (!text || !id_start || !id_len || !umi_off)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_find: bad arguments (info, a separator ':' or '_', the text, and the ID lines and room for the offsets of at most 2^32-2 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(text, id_start, id_len, umi_off))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_find: the text, the ID lines' starts and lengths and umi_off are device memory");
    hipStream_t stream = fqd_internal_stream(e);
    void* scratch = nullptr;
    const int rc = fqd_internal_scratch(e, 1, sizeof(Found), &scratch);
    if (rc) return rc;
    Found* found = static_cast<Found*>(scratch);
    FQD_TRY(e, hipMemsetAsync(found, 0xFF, sizeof(Found), stream));
    const uint32_t blocks = uint32_t((n + kTile - 1) / kTile);
    hipLaunchKernelGGL(umi_find_kernel, dim3(1), dim3(kBlock), 0, stream, text, id_start, id_len, uint64_t(1), uint32_t(sep), 1, found, umi_off);
    hipLaunchKernelGGL(umi_find_kernel, dim3(blocks), dim3(kBlock), 0, stream, text, id_start, id_len, n, uint32_t(sep), 0, found, umi_off);
    FQD_TRY(e, hipGetLastError());
    Found got{};
    FQD_TRY(e, read_back(got, found, stream));
    info->umi_len = got.ulen;
    info->joiners = got.joiners;
    info->n_bases = got.ulen - uint32_t(__builtin_popcountll(got.joiners));
    if (got.bad != kNoBad) fqdclusters::bad_parts(got.bad, &info->bad_record, &info->bad_reason);
    return FQD_OK;
}

int fqd_umi_reads(fqd_engine* e, const uint8_t* text, const uint64_t* id_start, const uint32_t* umi_off, const fqd_umi_info* info,
                  const fqd_reads* mate0, uint64_t n, uint8_t* out, uint64_t out_capacity, uint64_t* out_off, uint32_t* out_len)
{
    if (!e) return FQD_ERR_ARG;
    if (!info || !mate0 || n > 0xFFFFFFFEull || (n && (!text || !id_start || !umi_off || !out_off || !out_len)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_reads: bad arguments (info, mate 1's descriptors, the text, and the ID lines' starts, the UMI offsets and room for the offsets and lengths of at most 2^32-2 records)");
    if (n == 0) return FQD_OK;
    if (info->bad_record != FQD_UMI_NO_RECORD || info->umi_len == 0 || info->umi_len > fqdumi::kMaxUmi ||
        (info->umi_len < 64 && (info->joiners >> info->umi_len)) || info->n_bases == 0 ||
        info->n_bases != info->umi_len - uint32_t(__builtin_popcountll(info->joiners)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_reads: info is not what fqd_umi_find leaves for records it does not refuse");
    const fqd_reads& m = *mate0;
    if (!is_uniform(m) && (!m.offsets || !m.lengths)) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_reads: offsets and lengths go together");
    if (!m.bases && !(is_uniform(m) && m.uniform_len == 0)) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_reads: null bases");
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(text, id_start, umi_off) || (m.bases && !on_device(m.bases)) ||
        (m.offsets && !all_on_device(m.offsets, m.lengths)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_reads: the text, the ID lines' starts, the UMI offsets, the reads and their descriptors are device memory");
    if ((out && !on_device(out)) || !all_on_device(out_off, out_len))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_reads: out, the offsets and the lengths are device memory");
    hipStream_t stream = fqd_internal_stream(e);
    fqdumi::Table table;
    const uint32_t lb = fqdumi::bases_table(info->umi_len, info->joiners, &table);
    const Mate m0{m.bases, m.offsets, m.lengths, m.uniform_len, m.uniform_stride};
    const Mate umi{nullptr, nullptr, nullptr, lb, 0};       // Lb more bytes a record

    const uint32_t tiles = uint32_t((n + kOffTile - 1) / kOffTile);
    void* scratch = nullptr;
    const int rc = fqd_internal_scratch(e, 1, (size_t(tiles) + 1) * sizeof(unsigned long long), &scratch);
    if (rc) return rc;
    unsigned long long* tile = static_cast<unsigned long long*>(scratch);
    unsigned long long* d_total = tile + tiles;
    hipLaunchKernelGGL(record_bytes_kernel<2>, dim3(tiles), dim3(kBlock), 0, stream, m0, umi, n, tile);
    hipLaunchKernelGGL(scan_tiles_kernel<unsigned long long>, dim3(1), dim3(1024), 0, stream, tile, tiles, d_total);
    FQD_TRY(e, hipGetLastError());
    // the size of the output before a byte of it is written: known here for uniform reads, else read back from the scan
    unsigned long long total = 0;
    if (is_uniform(m)) total = n * (uint64_t(m.uniform_len) + lb);
    else {
        FQD_TRY(e, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, stream));
        FQD_TRY(e, hipStreamSynchronize(stream));
    }
    if (total > out_capacity || !out)
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_umi_reads: out_capacity is smaller than the UMI bases and the sequence bytes of the input (nothing was written)");
    unsigned long long* rec_off = reinterpret_cast<unsigned long long*>(out_off);
    const uint32_t blocks = uint32_t((n + kTile - 1) / kTile);
    hipLaunchKernelGGL(record_offsets_kernel<2>, dim3(tiles), dim3(kBlock), 0, stream, m0, umi, n, static_cast<const unsigned long long*>(tile), rec_off);
    hipLaunchKernelGGL(umi_pack_kernel, dim3(blocks), dim3(kBlock), 0, stream, text, id_start, umi_off, table, lb, m0, n, out,
                       static_cast<const uint64_t*>(out_off), out_len);
    FQD_TRY(e, hipGetLastError());
    return FQD_OK;
}

} // extern "C"
