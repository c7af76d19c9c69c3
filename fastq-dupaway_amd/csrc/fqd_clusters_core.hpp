// fqd_clusters_core.hpp — the words the `--fast` units hand from kernel to kernel and from kernel to host, once: a cluster's
// entry on the list of its size class, the room such a list needs, and the word a refused record comes back in.  Shared by
// the device code (csrc/fqd_clusters.hpp and the units that include it; fqd_umi.hip and fqd_sizein.hip for the refusal word)
// and a CPU harness of the tests (tests/native/clusters_check.cpp builds this header with g++ and the sanitizers).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FQD_CLUSTERS_HD __host__ __device__ __forceinline__
#else
#define FQD_CLUSTERS_HD inline
#endif

namespace fqdclusters {

// ---- a list entry: (the cluster's first place << 32 | its members) ------------------------------------------------------------
FQD_CLUSTERS_HD unsigned long long entry(uint32_t k0, uint32_t s) { return (static_cast<unsigned long long>(k0) << 32) | s; }
FQD_CLUSTERS_HD uint64_t entry_place(unsigned long long e) { return e >> 32; }
FQD_CLUSTERS_HD uint32_t entry_members(unsigned long long e) { return uint32_t(e); }

// The room of a list of clusters of MORE THAN `bound` members among n places: disjoint clusters of bound + 1 places at least,
// so floor(n / (bound + 1)) of them at most, and one entry more so that no list is empty.
FQD_CLUSTERS_HD uint64_t list_room(uint64_t n, uint64_t bound) { return n / (bound + 1) + 1; }

// ---- the refusal word: (record << 3 | reason), the lowest of them by a 64-bit atomicMin -----------------------------------------
// A reason is 1 .. 7 where a record is refused (0 is "fine" and is not sent); records stay below 2^32, so no word is kNoBad.
constexpr unsigned long long kNoBad = ~0ull;

FQD_CLUSTERS_HD unsigned long long bad_word(uint64_t record, uint32_t reason) { return (static_cast<unsigned long long>(record) << 3) | reason; }

// What the host makes of a word other than kNoBad that came back.
inline void bad_parts(unsigned long long word, uint64_t* record, uint32_t* reason) { *record = word >> 3; *reason = uint32_t(word & 7u); }

} // namespace fqdclusters
