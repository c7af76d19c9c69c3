// fqd_internal.hpp — what the HIP units of the library share on the host side: the hooks into an engine that are not
// exported (declared HERE ONLY; fqd_engine.hip and fqd_join.hip define them and include this, so a definition that
// differs from its declaration does not compile), the error macro, and two helpers every unit with scratch re-typed.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
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
