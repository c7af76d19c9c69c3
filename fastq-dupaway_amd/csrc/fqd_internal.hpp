// fqd_internal.hpp — what the HIP units of the library share on the host side: the hooks into an engine that are not
// exported (declared HERE ONLY; fqd_engine.hip and fqd_join.hip define them and include this, so a definition that
// differs from its declaration does not compile), the error macro, and what every entry point's launcher re-typed: the
// grid of a strided kernel, the pieces of a scratch block (Carver), the checks of the caller's pointers (on_device,
// all_on_device, overlap), the host's clock over a call's stages (StageTimer), a wait for counters (read_back), and the
// layout of scratch slot 1 in front of a tile scan (TileScratch).  Nothing in here is exported: static, or a template.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>

#include "../../include/fqdupaway.h"

#define FQD_HIDDEN __attribute__((visibility("hidden")))
FQD_HIDDEN hipStream_t fqd_internal_stream(fqd_engine* e);
FQD_HIDDEN int fqd_internal_device(fqd_engine* e);
FQD_HIDDEN int fqd_internal_segments(fqd_engine* e);      // fqd_config.segments: 1 or 2
FQD_HIDDEN int fqd_internal_fail(fqd_engine* e, int code, const char* msg);
FQD_HIDDEN uint64_t* fqd_internal_state(fqd_engine* e);
FQD_HIDDEN int fqd_internal_scratch(fqd_engine* e, int which, size_t bytes, void** out);
// The radix passes of fqd_join.hip for other units: counts holds fqd_internal_radix_counts(N) uint32, tot 256.
FQD_HIDDEN size_t fqd_internal_radix_counts(uint64_t N);
FQD_HIDDEN int fqd_internal_radix_sort(fqd_engine* e, hipStream_t stream, uint64_t* const keys[2], uint32_t* const vals[2],
                                       uint32_t* counts, uint32_t* tot, uint64_t N, uint32_t nbits, int* cur_io);

#define FQD_TRY(e, expr)                                                                    \
    do { hipError_t err_ = (expr); if (err_ != hipSuccess) { (void)hipGetLastError();       \
        return fqd_internal_fail(e, FQD_ERR_HIP, hipGetErrorString(err_)); } } while (0)

static inline uint32_t grid_for(uint64_t n, uint32_t per_block = 256, uint32_t cap = 4096)
{
    return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1) / per_block, cap)));
}

// 256-byte aligned pieces of one scratch block: run once with a null base to size it (`used`), once more to place them.
struct Carver {
    char* p; size_t used = 0;
    template <class T> FQD_HIDDEN T* take(size_t count)
    {
        T* r = p ? reinterpret_cast<T*>(p + used) : nullptr;
        used += (count * sizeof(T) + 255) & ~size_t(255);
        return r;
    }
};

// Is p memory a kernel may read?  An optional array stays written as (!p || on_device(p)) where it is checked.
static inline bool on_device(const void* p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

template <class... P>
static inline bool all_on_device(const P*... p) { return (on_device(p) && ...); }

// Do a_bytes at a and b_bytes at b share a byte?  b may be null (an array the caller left out): no.
static inline bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
    return b && pa < pb + b_bytes && pb < pa + a_bytes;
}

// What a stage of a call cost, seen from the host: mark(k) behind a wait of the call's own writes ms[k], the time since the
// mark before it (the first: since the timer was made).
struct StageTimer {
    float* ms;
    std::chrono::steady_clock::time_point clock = std::chrono::steady_clock::now();
    void mark(int k)
    {
        const auto now = std::chrono::steady_clock::now();
        ms[k] = std::chrono::duration<float, std::milli>(now - clock).count();
        clock = now;
    }
};

// *dev comes back into host, and the stream's work in front of it is through.
template <class T>
static inline hipError_t read_back(T& host, const T* dev, hipStream_t stream)
{
    const hipError_t err = hipMemcpyAsync(&host, dev, sizeof(T), hipMemcpyDeviceToHost, stream);
    return err != hipSuccess ? err : hipStreamSynchronize(stream);
}

// *dev starts a call as zeroes, but for ones (where given): the one 64-bit word of C that starts as ~0, the identity of the
// atomicMin that a refusal comes back through.
template <class C>
static inline hipError_t zero_counters(C* dev, hipStream_t stream, unsigned long long C::* ones = nullptr)
{
    const hipError_t err = hipMemsetAsync(dev, 0, sizeof(C), stream);
    return err != hipSuccess || !ones ? err : hipMemsetAsync(&(dev->*ones), 0xFF, sizeof(unsigned long long), stream);
}

// Scratch slot 1 of a unit whose first phase is a tile scan: a sum a tile, the total behind them, and the unit's counters C
// at the next 256-byte edge.  reserve() takes the slot, zeroes the counters and — ones: the one 64-bit word of C that
// starts as ~0, the identity of an atomicMin — fills that word; it returns what an entry point returns.
template <class C>
struct TileScratch {
    uint32_t tiles = 0;
    unsigned long long *tile_sum = nullptr, *total = nullptr;
    C* counters = nullptr;
    int reserve(fqd_engine* e, uint32_t n_tiles, hipStream_t stream, unsigned long long C::* ones = nullptr)
    {
        void* base = nullptr;
        const int rc = fqd_internal_scratch(e, 1, (size_t(n_tiles) + 1) * sizeof(unsigned long long) + 256 + sizeof(C), &base);
        if (rc) return rc;
        Carver c{static_cast<char*>(base)};
        tiles = n_tiles; tile_sum = c.take<unsigned long long>(size_t(n_tiles) + 1); total = tile_sum + n_tiles; counters = c.take<C>(1);
        FQD_TRY(e, zero_counters(counters, stream, ones));
        return FQD_OK;
    }
};
