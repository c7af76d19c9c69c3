// owner_check.cpp — the rules of FQD_FAST_KEEP / FQD_FAST_CLUSTERS (fastq-dupaway_amd/csrc/fqd_owner_core.hpp) on the CPU,
// the way the device runs them.  tests/test_owner_core.py builds this with the sanitizers and holds it against plain Python.
//   owner_check chain < "n" then n lines "keep link"   > per record "owner steps" (owner 4294967295: a broken chain)
//   owner_check group < "n" then n owners              > "bits" then per sorted place "record head": a stable sort by the
//                       low group_bits(n) bits of group_key, as the radix passes sort, and group_starts on the keys
//   owner_check bits  < one n per line                 > group_bits(n) per line
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_owner_core.hpp"

static int chain()
{
    unsigned long long n = 0;
    if (std::scanf("%llu", &n) != 1) return 2;
    std::vector<uint8_t> keep(n);                            // heap arrays of exactly n entries: a read outside is the sanitizer's
    std::vector<uint32_t> link(n);
    for (uint64_t i = 0; i < n; ++i) {
        unsigned k, l;
        if (std::scanf("%u %u", &k, &l) != 2) return 2;
        keep[i] = uint8_t(k); link[i] = l;
    }
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t steps = 0;
        const uint32_t o = fqdowner::chain_owner(keep.data(), link.data(), uint32_t(i), &steps);
        std::printf("%u %u\n", o, steps);
    }
    return 0;
}

static int group()
{
    unsigned long long n = 0;
    if (std::scanf("%llu", &n) != 1) return 2;
    std::vector<uint64_t> key(n);
    std::vector<uint32_t> val(n);
    for (uint64_t i = 0; i < n; ++i) {
        unsigned o;
        if (std::scanf("%u", &o) != 1) return 2;
        key[i] = fqdowner::group_key(o); val[i] = uint32_t(i);
    }
    const uint32_t bits = fqdowner::group_bits(n);
    const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
    std::stable_sort(val.begin(), val.end(), [&](uint32_t a, uint32_t b) { return (key[a] & mask) < (key[b] & mask); });
    std::printf("%u\n", bits);
    for (uint64_t k = 0; k < n; ++k)
        std::printf("%u %d\n", val[k], fqdowner::group_starts(k, k ? key[val[k - 1]] : 0, key[val[k]]) ? 1 : 0);
    return 0;
}

static int bits()
{
    unsigned long long n;
    while (std::scanf("%llu", &n) == 1) std::printf("%u\n", fqdowner::group_bits(n));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "chain") == 0) return chain();
    if (argc == 2 && std::strcmp(argv[1], "group") == 0) return group();
    if (argc == 2 && std::strcmp(argv[1], "bits") == 0) return bits();
    return 2;
}
