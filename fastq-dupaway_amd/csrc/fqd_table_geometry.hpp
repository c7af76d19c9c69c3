// fqd_table_geometry.hpp — how large an engine's table is and how it is cut: slots from records, the probing segment,
// the two partition digits of the bulk insert and the width of a slot's tag.  Plain host functions that read no
// environment (csrc/fqd_engine.hip reads FQD_SEG_BITS and FQD_TABLE_PCT and hands them in); a CPU harness of the tests
// (tests/native/table_geometry_check.cpp) builds this header with g++ and prints the whole table of geometries.
//
// A table of 2^t slots is 2^(t - seg_bits) probing segments (buckets) of 2^seg_bits slots.  The bulk insert sorts a
// batch by bucket in one or two radix passes: bucket = (d1 << bits2) | d2, bits1 <= 8 (256 ways), bits2 <= 9 (512 ways),
// so at most 2^17 buckets.  A partition record carries the table position's bits below the level-1 digit, the slot tag
// and the record index in 8 bytes (fqd_kernels.hpp, BulkGeom): seg_bits + bits2 + tag bits = 32.
#pragma once
#include <algorithm>
#include <cstdint>

namespace fqdgeom {

constexpr uint32_t kDefaultSegBits = 13u;              // 64 KiB of LDS per segment: best of the 12/13/14 sweep
constexpr uint64_t kDefaultTablePct = 200u;            // slots per 100 records of a table sized for a known total
constexpr uint64_t kMinSlots = 1ull << 16;

inline uint64_t pow2_at_least(uint64_t v) { uint64_t p = 1; while (p < v) p <<= 1; return p; }
inline uint32_t log2_ceil(uint64_t slots) { uint32_t t = 0; while ((1ull << t) < slots) ++t; return t; }

// FQD_SEG_BITS as the engine takes it: 12..14.
inline uint32_t clamp_seg_bits(int wanted) { return uint32_t(std::min(14, std::max(12, wanted))); }
// FQD_TABLE_PCT as the engine takes it: 115..400.
inline uint64_t clamp_table_pct(long wanted) { return uint64_t(wanted < 115 ? 115 : (wanted > 400 ? 400 : wanted)); }

// Probing segments: 4096..16384 slots so that (slots / segment) <= 131072 buckets, or the whole
// table when it is smaller than one segment.  want: the wished width (kDefaultSegBits, or FQD_SEG_BITS clamped).
inline uint32_t seg_bits_for(uint64_t slots, uint32_t want = kDefaultSegBits)
{
    const uint32_t t = log2_ceil(slots);
    if (t <= 12) return t;
    return std::min<uint32_t>(14u, std::max<uint32_t>(want, t >= 17 ? t - 17 : 12u));
}

// How a table of 2^t slots with 2^seg_bits-slot segments is split into partition digits, and
// how wide its slot tags can be so that a partition record fits 8 bytes (fqd_kernels.hpp,
// BulkGeom): seg_bits + bits2 + tag bits = 32.
inline void table_digits(uint32_t t, uint32_t seg_bits, uint32_t& bits1, uint32_t& bits2)
{
    const uint32_t nb_bits = t > seg_bits ? t - seg_bits : 0;
    bits1 = nb_bits <= 8 ? nb_bits : std::min<uint32_t>(8u, (nb_bits + 1) / 2);   // level 1: 256 ways at most
    bits2 = nb_bits - bits1;                                                      // level 2: 512 ways at most (bulk_plan checks)
}
inline uint32_t tag_mask_for(uint64_t slots, uint32_t seg_bits)
{
    const uint32_t t = log2_ceil(slots);
    uint32_t bits1, bits2;
    table_digits(t, seg_bits, bits1, bits2);
    const uint32_t tag_bits = 32u - std::min(seg_bits, 14u) - std::min(bits2, 9u);
    return tag_bits >= 32 ? 0xFFFFFFFFu : (1u << tag_bits) - 1u;
}

// The sizing rule.  Load limit: 50 % (a table grows 4x so rehashes stay rare).  A table sized for a KNOWN total
// (capacity hint) may run denser, exact_pct slots per 100 records.
// The fewest slots a table that was sized exactly (or not) may have for records_after records:
inline uint64_t min_slots_for(uint64_t records_after, bool table_exact, uint64_t exact_pct)
{
    return table_exact ? (records_after * exact_pct + 99) / 100 : 2 * records_after;
}
// ... and the slots of the table allocated when that is not met.  exact: size for a known total.
inline uint64_t slots_for(uint64_t records_after, bool exact, uint64_t exact_pct)
{
    return std::max<uint64_t>(pow2_at_least(exact ? (records_after * exact_pct + 99) / 100 : 4 * records_after), kMinSlots);
}

} // namespace fqdgeom
