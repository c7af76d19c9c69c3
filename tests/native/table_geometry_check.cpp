// table_geometry_check.cpp — csrc/fqd_table_geometry.hpp on the CPU: prints the geometry of every table the engine can
// build, for tests/test_table_geometry.py to hold against its invariants and against tests/bulk_placement.py.
//   geom <t> <wanted seg bits> <seg_bits> <bits1> <bits2> <tag_mask>      t = 13..31, wanted = 12, 13, 14
//   size <records> <exact 0|1> <pct> <slots_for> <min_slots_for>
#include <cstdio>

#include "../../fastq-dupaway_amd/csrc/fqd_table_geometry.hpp"

int main()
{
    for (uint32_t t = 13; t <= 31; ++t)
        for (uint32_t want = 12; want <= 14; ++want) {
            const uint64_t slots = 1ull << t;
            const uint32_t seg_bits = fqdgeom::seg_bits_for(slots, want);
            uint32_t bits1 = 0, bits2 = 0;
            fqdgeom::table_digits(t, seg_bits, bits1, bits2);
            std::printf("geom %u %u %u %u %u %u\n", t, want, seg_bits, bits1, bits2, fqdgeom::tag_mask_for(slots, seg_bits));
        }
    const uint64_t records[] = {1, 2, 5461, 5462, 16383, 16384, 16385, 32768, 32769, 65536, 349526, 1u << 21, (1u << 21) + 1, 1u << 28, 100000000};
    const uint64_t pcts[] = {115, 200, 400};
    for (uint64_t r : records)
        for (int exact = 0; exact <= 1; ++exact)
            for (uint64_t pct : pcts)
                std::printf("size %llu %d %llu %llu %llu\n", static_cast<unsigned long long>(r), exact, static_cast<unsigned long long>(pct),
                            static_cast<unsigned long long>(fqdgeom::slots_for(r, exact != 0, pct)),
                            static_cast<unsigned long long>(fqdgeom::min_slots_for(r, exact != 0, pct)));
    // the clamps of the two wishes
    for (int w : {-1, 0, 11, 12, 13, 14, 15, 99}) std::printf("clamp_seg %d %u\n", w, fqdgeom::clamp_seg_bits(w));
    for (long w : {0L, 114L, 115L, 200L, 400L, 401L}) std::printf("clamp_pct %ld %llu\n", w, static_cast<unsigned long long>(fqdgeom::clamp_table_pct(w)));
    return 0;
}
