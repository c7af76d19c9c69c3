// fqd_owner.hip — FQD_FAST_KEEP / FQD_FAST_CLUSTERS of the `--fast` mode (same library as fqd_engine.hip): which record
// a duplicate repeats, and the records grouped by that record.  Rules and proofs: fqd_owner_core.hpp.
//
//   owners   fqd_owners: one record per lane walks its chain of links (fqd_submit_linked) down to the kept record of its
//            key.  A walk is a chain of dependent 4-byte gathers, of length 1 for nearly every duplicate (a link names the
//            slot's owner of the moment, which is the first occurrence unless that one was displaced later in the same
//            launch); kept records read one byte and are done.
//   group    fqd_group_owners: (owner, index) through the stable LSD radix passes of fqd_join.hip, as many 8-bit passes
//            as n - 1 has bits; then one pass that writes the order and flags the first place of every run.
//   keep     fqd_heads_to_keep: keep[perm[k]] = head[k], a byte store per place.  perm is nearly ascending where clusters
//            are small, so neighbouring lanes mostly store to neighbouring bytes.
#include <hip/hip_runtime.h>

#include "fqd_internal.hpp"
#include "fqd_owner_core.hpp"
#include "fqd_wave.hpp"

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock)
void owners_kernel(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ link, uint64_t n, uint32_t* __restrict__ owner,
                   unsigned long long* __restrict__ broken)
{
    uint32_t bad = 0;
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
        const uint32_t o = fqdowner::chain_owner(keep, link, uint32_t(i), nullptr);
        owner[i] = o;
        bad += o == fqdowner::kBrokenChain;
    }
    bad = fqdwave::wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(broken, static_cast<unsigned long long>(bad));
}

__global__ __launch_bounds__(kBlock)
void group_fill_kernel(const uint32_t* __restrict__ owner, uint64_t n, uint64_t* __restrict__ key, uint32_t* __restrict__ val)
{
    for (uint64_t i = blockIdx.x * uint64_t(kBlock) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kBlock) {
        key[i] = fqdowner::group_key(owner[i]);
        val[i] = uint32_t(i);
    }
}

__global__ __launch_bounds__(kBlock)
void group_heads_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, uint64_t n, uint32_t* __restrict__ perm,
                        uint8_t* __restrict__ head, unsigned long long* __restrict__ n_heads)
{
    uint32_t heads = 0;
    for (uint64_t k = blockIdx.x * uint64_t(kBlock) + threadIdx.x; k < n; k += uint64_t(gridDim.x) * kBlock) {
        const bool starts = fqdowner::group_starts(k, k ? key[k - 1] : 0ull, key[k]);
        perm[k] = val[k];
        head[k] = starts ? 1 : 0;
        heads += starts;
    }
    heads = fqdwave::wave_sum(heads);
    if ((threadIdx.x & 63) == 0 && heads) atomicAdd(n_heads, static_cast<unsigned long long>(heads));
}

__global__ __launch_bounds__(kBlock)
void heads_to_keep_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ head, uint64_t n, uint8_t* __restrict__ keep)
{
    for (uint64_t k = blockIdx.x * uint64_t(kBlock) + threadIdx.x; k < n; k += uint64_t(gridDim.x) * kBlock) {
        const uint32_t r = perm[k];
        if (r < n) keep[r] = head[k];                        // (an order that is no permutation of 0 .. n-1 never leaves keep[])
    }
}

struct GroupBuffers { uint64_t* keys[2]; uint32_t* vals[2]; uint32_t *counts, *tot; unsigned long long* n_heads; };

size_t carve_group(uint64_t n, char* base, GroupBuffers& b)
{
    Carver c{base};
    b.n_heads = c.take<unsigned long long>(1);
    b.keys[0] = c.take<uint64_t>(n); b.keys[1] = c.take<uint64_t>(n);
    b.vals[0] = c.take<uint32_t>(n); b.vals[1] = c.take<uint32_t>(n);
    b.counts = c.take<uint32_t>(fqd_internal_radix_counts(n)); b.tot = c.take<uint32_t>(256);
    return c.used + 256;
}

// Is p memory the device can be handed?  Asked of the runtime's bookkeeping: nothing is allocated or touched.
} // namespace

extern "C" {

int fqd_owners(fqd_engine* e, const uint8_t* keep, const uint32_t* link, uint64_t n, uint32_t* owner)
{
    if (!e) return FQD_ERR_ARG;
    if (n >= 0xFFFFFFFFull || (n && (!keep || !link || !owner)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_owners: bad arguments (keep flags, links and room for the owners of at most 2^32-2 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(keep, link, owner))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_owners: keep, link and owner are device memory");
    hipStream_t s = fqd_internal_stream(e);
    void* small = nullptr;
    const int rc = fqd_internal_scratch(e, 1, 4096, &small);
    if (rc) return rc;
    unsigned long long* broken = static_cast<unsigned long long*>(small);
    FQD_TRY(e, hipMemsetAsync(broken, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(owners_kernel, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, keep, link, n, owner, broken);
    FQD_TRY(e, hipGetLastError());
    unsigned long long bad = 0;
    FQD_TRY(e, hipMemcpyAsync(&bad, broken, sizeof bad, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (bad) return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_owners: a cleared flag's link does not name an earlier record (were all n records submitted through fqd_submit_linked?)");
    return FQD_OK;
}

int fqd_group_owners(fqd_engine* e, const uint32_t* owner, uint64_t n, uint32_t* perm, uint8_t* head, uint64_t* n_clusters)
{
    if (!e) return FQD_ERR_ARG;
    if (n >= 0x80000000ull || (n && (!owner || !perm || !head)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_group_owners: bad arguments (owners, and room for the order and the head flags of at most 2^31-1 records)");
    if (n_clusters) *n_clusters = 0;
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(owner, perm, head))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_group_owners: owner, perm and head are device memory");
    hipStream_t s = fqd_internal_stream(e);
    GroupBuffers b{};
    void* base = nullptr;
    int rc = fqd_internal_scratch(e, 0, carve_group(n, nullptr, b), &base);
    if (rc) return rc;
    (void)carve_group(n, static_cast<char*>(base), b);
    FQD_TRY(e, hipMemsetAsync(b.n_heads, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(group_fill_kernel, dim3(grid_for(n, kBlock, 4096)), dim3(kBlock), 0, s, owner, n, b.keys[0], b.vals[0]);
    int cur = 0;
    if ((rc = fqd_internal_radix_sort(e, s, b.keys, b.vals, b.counts, b.tot, n, fqdowner::group_bits(n), &cur))) return rc;
    hipLaunchKernelGGL(group_heads_kernel, dim3(grid_for(n, kBlock, 4096)), dim3(kBlock), 0, s, static_cast<const uint64_t*>(b.keys[cur]),
                       static_cast<const uint32_t*>(b.vals[cur]), n, perm, head, b.n_heads);
    FQD_TRY(e, hipGetLastError());
    unsigned long long heads = 0;
    FQD_TRY(e, hipMemcpyAsync(&heads, b.n_heads, sizeof heads, hipMemcpyDeviceToHost, s));
    FQD_TRY(e, hipStreamSynchronize(s));
    if (n_clusters) *n_clusters = heads;
    return FQD_OK;
}

int fqd_heads_to_keep(fqd_engine* e, const uint32_t* perm, const uint8_t* head, uint64_t n, uint8_t* keep)
{
    if (!e) return FQD_ERR_ARG;
    if (n >= 0x100000000ull || (n && (!perm || !head || !keep)))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_heads_to_keep: bad arguments (the order, its head flags and room for the keep flags of at most 2^32-1 records)");
    if (n == 0) return FQD_OK;
    FQD_TRY(e, hipSetDevice(fqd_internal_device(e)));
    if (!all_on_device(perm, head, keep))
        return fqd_internal_fail(e, FQD_ERR_ARG, "fqd_heads_to_keep: perm, head and keep are device memory");
    hipStream_t s = fqd_internal_stream(e);
    hipLaunchKernelGGL(heads_to_keep_kernel, dim3(grid_for(n, kBlock, 4096)), dim3(kBlock), 0, s, perm, head, n, keep);
    FQD_TRY(e, hipGetLastError());
    FQD_TRY(e, hipStreamSynchronize(s));
    return FQD_OK;
}

} // extern "C"
