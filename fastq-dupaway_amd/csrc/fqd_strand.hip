// fqd_strand.hip — FQD_FAST_STRAND=both of the `--fast` mode (same library as fqd_engine.hip): every read (pair) turned
// into the orientation it is keyed in, packed back to back, with descriptors the engine takes as they are.  Rule and
// proofs: fqd_strand_core.hpp.
//
//   sizes    record_bytes_kernel + scan_tiles_kernel + record_offsets_kernel (fqd_record_scan.hpp, shared with
//            fqd_umi.hip): where every record's canonical bytes start.  A record's bytes (len0 + len1) do not depend on its orientation, so the offsets are known before any base
//            has been looked at: the three-step scan of fqd_output_plan (2048 records a block, one block over the
//            block sums, 2048 records a block again).
//   canon    canon_kernel: a wave takes a tile of 64 neighbouring records — their descriptors with one coalesced load a
//            lane — and works through it four records at a time, SIXTEEN LANES A RECORD, sixteen bytes a lane: 256 bytes
//            of a read per step, loaded and stored as dwordx4 by neighbouring lanes (what fqd_copy_spans does with
//            eight).  decide: lane l holds s[16l .. 16l+16) and the reverse complement of the mirrored sixteen bytes,
//            turned round in registers (a byte swap per dword, comp on four bytes at a time); the lanes that see a
//            difference are collected with one ballot and the lowest lane of a record's sixteen decides — over half
//            the read only (the lemma of the core header); pairs compare mate 1 with mate 2 the same way.  write: the
//            same sixteen lanes store the chosen orientation; the mirrored bytes come from the lines the decide step
//            has just pulled in, so a read's bytes leave HBM once.  The reversal happens inside a lane's sixteen bytes
//            and by which chunk a lane asks for: no staging through LDS is needed for it.  No lane walks a read byte by
//            byte; reads shorter than a chunk (under 32 bytes for the decide, under 16 for the copy) take one byte a lane.
#include <hip/hip_runtime.h>

#include "fqd_internal.hpp"
#include "fqd_record_scan.hpp"
#include "fqd_strand_core.hpp"

namespace {

constexpr int kBlock = fqdscan::kBlock;
constexpr uint32_t kGroup = 16;                              // lanes a record
constexpr uint32_t kWaveTile = 64;                           // records a wave
constexpr uint32_t kTile = kWaveTile * (kBlock / 64);        // records a block of canon_kernel
constexpr int kOffTile = fqdscan::kOffTile;                  // records a block of the scan's two passes

using fqdscan::Mate;                                         // the descriptors and the three-step scan: fqd_record_scan.hpp
using fqdscan::mate_off;
using fqdscan::mate_len;
using fqdscan::record_bytes_kernel;
using fqdscan::scan_tiles_kernel;
using fqdscan::record_offsets_kernel;

// What a group's lanes found in one round, read off the wave's two ballots: has a lane of the group seen a difference,
// and if so what the LOWEST such lane says.
__device__ __forceinline__ bool group_verdict(bool diff, bool less, uint32_t g, bool* flip)
{
    const unsigned long long bd = __ballot(diff), bl = __ballot(diff && less);
    const uint32_t gd = uint32_t(bd >> (kGroup * g)) & 0xFFFFu;
    if (!gd) return false;
    *flip = ((uint32_t(bl >> (kGroup * g)) >> __builtin_ctz(gd)) & 1u) != 0;
    return true;
}

// One wave per tile of kWaveTile records; see the head of the file.  rec_off = out_off0 as record_offsets_kernel left it.
template <int S>
__global__ __launch_bounds__(kBlock)
void canon_kernel(Mate m0, Mate m1, uint64_t n, uint8_t* __restrict__ out, const uint64_t* __restrict__ rec_off,
                  uint32_t* __restrict__ out_len0, uint64_t* __restrict__ out_off1, uint32_t* __restrict__ out_len1,
                  uint8_t* __restrict__ flipped, unsigned long long* __restrict__ n_flipped)
{
    const uint32_t lane = threadIdx.x & 63u, g = lane / kGroup, gl = lane % kGroup;
    const uint64_t tile0 = (uint64_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6)) * kWaveTile;
    if (tile0 >= n) return;                                  // (the whole wave)
    const uint64_t mine = tile0 + lane;
    unsigned long long off_a = 0, off_b = 0, base = 0;
    uint32_t len_a = 0, len_b = 0;
    if (mine < n) {
        off_a = mate_off(m0, mine); len_a = mate_len(m0, mine); base = rec_off[mine];
        if (S == 2) { off_b = mate_off(m1, mine); len_b = mate_len(m1, mine); }
    }
    uint32_t my_flip = 0;
    for (uint32_t j = 0; j < kWaveTile / 4u && tile0 + 4u * j < n; ++j) {
        const int r = int(4u * j + g);                       // the group's record of this step (beyond n: lengths 0)
        const uint8_t* __restrict__ a = m0.bases + __shfl(off_a, r, 64);
        const uint32_t la = __shfl(len_a, r, 64);
        uint8_t* __restrict__ dst = out + __shfl(base, r, 64);
        const uint8_t* __restrict__ b = nullptr;
        uint32_t lb = 0;
        if (S == 2) { b = m1.bases + __shfl(off_b, r, 64); lb = __shfl(len_b, r, 64); }

        // ---- decide (the lanes' looks: fqd_strand_core.hpp) ----
        bool decided = false, flip = false;
        const uint32_t m = la < lb ? la : lb;
        const uint32_t chunks = S == 1 ? fqdstrand::se_chunks(la) : fqdstrand::pe_chunks(m);
        for (uint32_t c0 = 0; __any(!decided && c0 < chunks); c0 += kGroup) {
            bool less = false;
            const bool diff = !decided && c0 < chunks && (S == 1 ? fqdstrand::se_lane_sees(a, la, c0, gl, &less) : fqdstrand::pe_lane_sees(a, b, m, c0, gl, &less));
            bool f = false;
            if (group_verdict(diff, less, g, &f) && !decided) { decided = true; flip = f; }
        }
        if (S == 2 && !decided) flip = lb < la;              // one is a prefix of the other: the shorter first
        const uint32_t got = __shfl(flip ? 1u : 0u, int((lane & 3u) * kGroup), 64);
        if ((lane >> 2) == j) my_flip = got;                 // record `lane` of the tile is group lane%4's at step lane/4

        // ---- write ----
        if (S == 1) fqdstrand::copy_lane(a, dst, la, flip, gl);
        else {
            fqdstrand::copy_lane(flip ? b : a, dst, flip ? lb : la, false, gl);
            fqdstrand::copy_lane(flip ? a : b, dst + (flip ? lb : la), flip ? la : lb, false, gl);
        }
    }
    if (mine < n) {
        flipped[mine] = uint8_t(my_flip);
        out_len0[mine] = my_flip ? (S == 2 ? len_b : len_a) : len_a;
        if (S == 2) { out_off1[mine] = base + (my_flip ? len_b : len_a); out_len1[mine] = my_flip ? len_a : len_b; }
    }
    const uint32_t turned = fqdwave::wave_sum(my_flip);
    if (lane == 0 && turned) atomicAdd(n_flipped, static_cast<unsigned long long>(turned));
}

bool is_uniform(const fqd_reads& r) { return r.offsets == nullptr && r.lengths == nullptr; }

} // namespace

extern "C" {

int fqd_canonical_reads(fqd_engine* e, const fqd_reads* seg, uint64_t n, uint8_t* out, uint64_t out_capacity,
                        uint64_t* out_off0, uint32_t* out_len0, uint64_t* out_off1, uint32_t* out_len1,
                        uint8_t* flipped, uint64_t* n_flipped)
{
    if (!e) return FQD_ERR_ARG;
    const int S = fqd_internal_segments(e);
    if (n_flipped) *n_flipped = 0;
    if (!seg || n > 0xFFFFFFFEull || (n && (!out_off0 || !out_len0 || !flipped)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_canonical_reads: bad arguments (descriptors, and room for the offsets, lengths and flags of at most 2^32-2 records)");
    if (S == 1 && (out_off1 || out_len1))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_canonical_reads: a single-end engine has no second mate (out_off1 and out_len1 are NULL)");
    if (S == 2 && n && (!out_off1 || !out_len1))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_canonical_reads: a paired engine needs out_off1 and out_len1");
    if (n == 0) return FQD_OK;
    bool uniform = true;
    for (int s = 0; s < S; ++s) {
        if (!is_uniform(seg[s])) {
            if (!seg[s].offsets || !seg[s].lengths) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_canonical_reads: offsets and lengths go together");
            uniform = false;
        }
        if (!seg[s].bases && !(is_uniform(seg[s]) && seg[s].uniform_len == 0))
            return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_canonical_reads: null bases");
    }
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    for (int s = 0; s < S; ++s)
        if ((seg[s].bases && !on_device(seg[s].bases)) || (seg[s].offsets && !all_on_device(seg[s].offsets, seg[s].lengths)))
            return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_canonical_reads: the reads and their descriptors are device memory");
    if ((out && !on_device(out)) || !all_on_device(out_off0, out_len0, flipped) ||
        (S == 2 && !all_on_device(out_off1, out_len1)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_canonical_reads: out, the offsets, the lengths and flipped are device memory");
    hipStream_t stream = fqd_internal_stream(e);
    const Mate m0{seg[0].bases, seg[0].offsets, seg[0].lengths, seg[0].uniform_len, seg[0].uniform_stride};
    const Mate m1 = S == 2 ? Mate{seg[1].bases, seg[1].offsets, seg[1].lengths, seg[1].uniform_len, seg[1].uniform_stride} : Mate{nullptr, nullptr, nullptr, 0, 0};

    const uint32_t tiles = uint32_t((n + kOffTile - 1) / kOffTile);
    void* scratch = nullptr;
    const int rc = fqd_internal_scratch(e, 1, (size_t(tiles) + 2) * sizeof(unsigned long long), &scratch);
    if (rc) return rc;
    unsigned long long* tile = static_cast<unsigned long long*>(scratch);
    unsigned long long *d_total = tile + tiles, *d_flipped = tile + tiles + 1;
    FQD_TRY(e, hipMemsetAsync(d_flipped, 0, sizeof(unsigned long long), stream));
    if (S == 1) hipLaunchKernelGGL(record_bytes_kernel<1>, dim3(tiles), dim3(kBlock), 0, stream, m0, m1, n, tile);
    else        hipLaunchKernelGGL(record_bytes_kernel<2>, dim3(tiles), dim3(kBlock), 0, stream, m0, m1, n, tile);
    hipLaunchKernelGGL(scan_tiles_kernel<unsigned long long>, dim3(1), dim3(1024), 0, stream, tile, tiles, d_total);
    FQD_TRY(e, hipGetLastError());
    // the size of the output before a byte of it is written: known here for uniform reads, else read back from the scan
    // (one 8-byte copy the call waits for, as a ragged fqd_submit does for its key words)
    unsigned long long total = 0;
    if (uniform) total = n * (uint64_t(seg[0].uniform_len) + (S == 2 ? seg[1].uniform_len : 0u));
    else {
        FQD_TRY(e, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, stream));
        FQD_TRY(e, hipStreamSynchronize(stream));
    }
    if (total > out_capacity || (total && !out))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_canonical_reads: out_capacity is smaller than the sequence bytes of the input (nothing was written)");
    unsigned long long* rec_off = reinterpret_cast<unsigned long long*>(out_off0);
    const uint32_t blocks = uint32_t((n + kTile - 1) / kTile);
    if (S == 1) {
        hipLaunchKernelGGL(record_offsets_kernel<1>, dim3(tiles), dim3(kBlock), 0, stream, m0, m1, n, static_cast<const unsigned long long*>(tile), rec_off);
        hipLaunchKernelGGL(canon_kernel<1>, dim3(blocks), dim3(kBlock), 0, stream, m0, m1, n, out, static_cast<const uint64_t*>(out_off0), out_len0,
                           out_off1, out_len1, flipped, d_flipped);
    } else {
        hipLaunchKernelGGL(record_offsets_kernel<2>, dim3(tiles), dim3(kBlock), 0, stream, m0, m1, n, static_cast<const unsigned long long*>(tile), rec_off);
        hipLaunchKernelGGL(canon_kernel<2>, dim3(blocks), dim3(kBlock), 0, stream, m0, m1, n, out, static_cast<const uint64_t*>(out_off0), out_len0,
                           out_off1, out_len1, flipped, d_flipped);
    }
    FQD_TRY(e, hipGetLastError());
    if (n_flipped) {
        unsigned long long got = 0;
        FQD_TRY(e, hipMemcpyAsync(&got, d_flipped, sizeof got, hipMemcpyDeviceToHost, stream));
        FQD_TRY(e, hipStreamSynchronize(stream));
        *n_flipped = got;
    }
    return FQD_OK;
}

} // extern "C"
