// size_order_check.cpp — the rules of FQD_FAST_SORT=size / FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE
// (fastq-dupaway_amd/csrc/fqd_size_order_core.hpp) on the CPU, the way the device runs them.  tests/test_size_order_core.py
// builds this with the sanitizers and holds it against plain Python.
//   size_order_check digit < one size per line          > tier1_digit(size), and the size and digit read back from tier1_key
//   size_order_check tier2 < "largest size" per line    > "key bits passes": tier2_key(largest, size), tier2_bits, tier2_passes
//   size_order_check drop  < "size min max" per line    > 1 where the filter takes the cluster out, 0 where it stays
//   size_order_check order < "n" then n lines           > W, then the W entries of the written order: the kept head places
//                            "perm head size keep"        compacted in place order, ONE stable pass by the low byte of tier1_key
//                                                         over all W, the first L rekeyed with tier2_key and sorted by
//                                                         tier2_passes stable 8-bit passes — fqd_size_order's steps one by one
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_size_order_core.hpp"

static int digit()
{
    unsigned long long v;
    while (std::scanf("%llu", &v) == 1) {
        const uint64_t key = fqdorder::tier1_key(uint32_t(v));
        std::printf("%u %u %u\n", fqdorder::tier1_digit(uint32_t(v)), fqdorder::key_size(key), unsigned(key & 0xFFu));
    }
    return 0;
}

static int tier2()
{
    unsigned long long largest, size;
    while (std::scanf("%llu %llu", &largest, &size) == 2)
        std::printf("%" PRIu64 " %u %u\n", fqdorder::tier2_key(uint32_t(largest), uint32_t(size)), fqdorder::tier2_bits(uint32_t(largest)),
                    fqdorder::tier2_passes(uint32_t(largest)));
    return 0;
}

static int drop()
{
    unsigned long long size, lo, hi;
    while (std::scanf("%llu %llu %llu", &size, &lo, &hi) == 3)
        std::printf("%d\n", fqdorder::dropped(uint32_t(size), uint32_t(lo), uint32_t(hi)) ? 1 : 0);
    return 0;
}

struct Pair { uint64_t key; uint32_t val; };

// One stable pass over p[0 .. n) by the eight bits of the key at `shift`: a counting sort, as the device's pass is.
static void stable_pass(std::vector<Pair>& p, size_t n, uint32_t shift)
{
    size_t start[257] = {0};
    for (size_t i = 0; i < n; ++i) ++start[((p[i].key >> shift) & 0xFFu) + 1];
    for (int d = 0; d < 256; ++d) start[d + 1] += start[d];
    std::vector<Pair> out(n);                                // exactly as long: an entry outside is the sanitizer's
    for (size_t i = 0; i < n; ++i) out[start[(p[i].key >> shift) & 0xFFu]++] = p[i];
    for (size_t i = 0; i < n; ++i) p[i] = out[i];
}

static int order()
{
    unsigned long long n = 0;
    if (std::scanf("%llu", &n) != 1) return 2;
    std::vector<uint32_t> perm(n), size(n);
    std::vector<uint8_t> head(n), keep(n);
    for (uint64_t k = 0; k < n; ++k) {
        unsigned p, h, s, f;
        if (std::scanf("%u %u %u %u", &p, &h, &s, &f) != 4) return 2;
        perm[k] = p; head[k] = uint8_t(h); size[k] = s; keep[k] = uint8_t(f);
    }
    std::vector<Pair> pairs;
    uint32_t largest = 0;
    size_t above = 0;
    for (uint64_t s = 0; s < n; ++s) {
        if (!head[s] || perm[s] >= n || !keep[perm[s]]) continue;
        const uint32_t sz = size[perm[s]];
        if (sz == 0) return 3;                               // refused before the sort
        pairs.push_back(Pair{fqdorder::tier1_key(sz), perm[s]});
        above += sz > fqdorder::kSmallMax;
        largest = sz > largest ? sz : largest;
    }
    const size_t w = pairs.size();
    stable_pass(pairs, w, 0);                                // tier 1
    for (size_t i = 0; i < above; ++i) {
        if (fqdorder::tier1_digit(fqdorder::key_size(pairs[i].key)) != 0) return 4;      // bucket 0 stands in front
        pairs[i].key = fqdorder::tier2_key(largest, fqdorder::key_size(pairs[i].key));
    }
    for (uint32_t pass = 0; pass < fqdorder::tier2_passes(largest); ++pass) stable_pass(pairs, above, 8u * pass);     // tier 2
    std::printf("%zu\n", w);
    for (size_t i = 0; i < w; ++i) std::printf("%u\n", pairs[i].val);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "digit") == 0) return digit();
    if (argc == 2 && std::strcmp(argv[1], "tier2") == 0) return tier2();
    if (argc == 2 && std::strcmp(argv[1], "drop") == 0) return drop();
    if (argc == 2 && std::strcmp(argv[1], "order") == 0) return order();
    return 2;
}
