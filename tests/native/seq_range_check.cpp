// seq_range_check.cpp — the rules of the ranged `--compare-seq` run (fastq-dupaway_amd/csrc/fqd_seq_range_core.hpp) on the
// CPU, the way the device runs them: a copy of (key, bytes) sorted by key (stable), the bytes scanned in 64 bits, the cuts
// by fqdseq::next_cut from cut to cut, every pair's range by fqdseq::range_of_key.  tests/test_seq_ranged_core.py builds
// this with the sanitizers and holds it against a brute-force plan.
//   seq_range_check plan  < "n target\n" then n lines "key bytes"     > "R\n", R lines "lo hi pairs bytes", n range numbers
//   seq_range_check keys  < one sequence per line as hex ("-" = empty) > one key per line, and whether a byte is below '\n'
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_seq_range_core.hpp"

static int plan()
{
    unsigned long long n = 0, target = 0;
    if (std::scanf("%llu %llu", &n, &target) != 2) return 2;
    std::vector<uint64_t> key(n), bytes(n);
    for (uint64_t i = 0; i < n; ++i) {
        unsigned long long k, b;
        if (std::scanf("%llu %llu", &k, &b) != 2) return 2;
        key[i] = k; bytes[i] = b;
    }
    std::vector<uint64_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return key[a] < key[b]; });
    std::vector<uint64_t> skey(n), prefix(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) { skey[i] = key[order[i]]; prefix[i + 1] = prefix[i] + bytes[order[i]]; }
    auto key_at = [&](uint64_t i) { return skey.at(i); };
    auto prefix_at = [&](uint64_t i) { return prefix.at(i); };
    std::vector<uint64_t> rows;
    for (uint64_t start = 0; start < n;) {
        const uint64_t e = fqdseq::next_cut(start, n, target, key_at, prefix_at);
        if (e <= start || e > n) return 3;
        rows.insert(rows.end(), {skey[start], skey[e - 1], e - start, prefix[e] - prefix[start]});
        start = e;
    }
    const uint32_t R = uint32_t(rows.size() / 4);
    std::printf("%u\n", R);
    for (uint32_t r = 0; r < R; ++r)
        std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", rows[4 * r], rows[4 * r + 1], rows[4 * r + 2], rows[4 * r + 3]);
    auto hi = [&](uint32_t r) { return rows.at(4 * size_t(r) + 1); };
    for (uint64_t i = 0; i < n; ++i) std::printf("%u\n", fqdseq::range_of_key(key[i], R, hi));
    return 0;
}

static int keys()
{
    char line[4096];
    while (std::fgets(line, sizeof line, stdin)) {
        std::vector<uint8_t> seq;
        const size_t len = std::strcspn(line, "\r\n");
        if (!(len == 1 && line[0] == '-'))
            for (size_t k = 0; k + 1 < len; k += 2) { unsigned v = 0; std::sscanf(line + k, "%2x", &v); seq.push_back(uint8_t(v)); }
        bool low = false;
        for (size_t k = 0; k + 8 <= seq.size(); k += 8) {
            uint64_t x;
            std::memcpy(&x, seq.data() + k, 8);
            bool slow = false;
            for (size_t j = 0; j < 8; ++j) slow = slow || seq[k + j] < '\n';
            if (fqdseq::word_has_byte_below_newline(x) != slow) return 4;      // the word test is exact
            low = low || slow;
        }
        for (size_t k = seq.size() & ~size_t(7); k < seq.size(); ++k) low = low || seq[k] < '\n';
        // a heap copy of exactly the sequence's bytes: a read behind them is the sanitizer's to report
        std::printf("%" PRIu64 " %d\n", fqdseq::prefix_key(seq.data(), uint32_t(seq.size())), low ? 1 : 0);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "plan") == 0) return plan();
    if (argc == 2 && std::strcmp(argv[1], "keys") == 0) return keys();
    return 2;
}
