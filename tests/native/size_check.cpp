// size_check.cpp — the rules of FQD_FAST_SIZEOUT / FQD_FAST_LEVELS (fastq-dupaway_amd/csrc/fqd_size_core.hpp) on the CPU, the
// way the device runs them.  tests/test_size_core.py builds this with the sanitizers and holds it against plain Python.
//   size_check level < one size per line            > level(size) per line
//   size_check label < one size per line            > "label_len text" per line (write_label into exactly label_len bytes)
//   size_check word  < one line per line, in hex    > "first_word_end lanes": the scalar rule, and the sixteen lanes of
//                                                     size_labels_kernel played one after another (fqdumi::lane_look)
//   size_check scan  < "n" then n head flags        > start(k) per place, by tiles of 4 places: tile values, their exclusive
//                                                     combine, then the places — the three launches with combine()
//   size_check copy  < "label_at tail size" lines   > the destination in hex: the eight lanes of copy_labelled_kernel played
//                                                     one after another over a source of exactly label_at + tail bytes
//                                                     (byte k = (37 k + 11) mod 251) and a destination of exactly the grown
//                                                     length; every byte is also held against copy_source()
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_size_core.hpp"
#include "../../fastq-dupaway_amd/csrc/fqd_umi_core.hpp"

static int level()
{
    unsigned long long v;
    while (std::scanf("%llu", &v) == 1) std::printf("%u\n", fqdsize::level(uint32_t(v)));
    return 0;
}

static int label()
{
    unsigned long long v;
    while (std::scanf("%llu", &v) == 1) {
        const uint32_t want = fqdsize::label_len(uint32_t(v));
        std::vector<uint8_t> text(want);                     // exactly as long: a byte too many is the sanitizer's
        const uint32_t got = fqdsize::write_label(text.data(), uint32_t(v));
        if (got != want) return 3;
        std::printf("%u %.*s\n", want, int(got), reinterpret_cast<const char*>(text.data()));
    }
    return 0;
}

static int word()
{
    char hex[8192];
    while (std::scanf("%8191s", hex) == 1) {
        const size_t len = std::strlen(hex) / 2;
        std::vector<uint8_t> line(len);
        for (size_t k = 0; k < len; ++k) { unsigned b; if (std::sscanf(hex + 2 * k, "%2x", &b) != 1) return 2; line[k] = uint8_t(b); }
        const uint32_t L = uint32_t(len);
        uint32_t end = fqdumi::kNone;
        const uint32_t chunks = fqdumi::line_chunks(L);
        for (uint32_t c0 = 0; end == fqdumi::kNone && c0 < chunks; c0 += 16u) {
            uint32_t e = fqdumi::kNone;
            for (uint32_t gl = 0; gl < 16u; ++gl) {
                const uint32_t x = fqdumi::look_end(fqdumi::lane_look(line.data(), L, uint8_t(' '), c0, gl));
                e = x < e ? x : e;
            }
            end = e;
        }
        if (end == fqdumi::kNone) end = L;
        std::printf("%u %u\n", fqdsize::first_word_end(line.data(), L), end);
    }
    return 0;
}

static int scan()
{
    unsigned long long n = 0;
    if (std::scanf("%llu", &n) != 1) return 2;
    std::vector<uint8_t> head(n);
    for (uint64_t k = 0; k < n; ++k) { unsigned h; if (std::scanf("%u", &h) != 1) return 2; head[k] = uint8_t(h); }
    const uint64_t tile = 4, tiles = (n + tile - 1) / tile;
    std::vector<uint32_t> value(tiles, fqdsize::kNone), carry(tiles, fqdsize::kNone);
    for (uint64_t t = 0; t < tiles; ++t)
        for (uint64_t k = t * tile; k < n && k < (t + 1) * tile; ++k)
            value[t] = fqdsize::combine(value[t], head[k] ? uint32_t(k) : fqdsize::kNone);
    for (uint64_t t = 1; t < tiles; ++t) carry[t] = fqdsize::combine(carry[t - 1], value[t - 1]);
    for (uint64_t t = 0; t < tiles; ++t) {
        uint32_t start = carry[t];
        for (uint64_t k = t * tile; k < n && k < (t + 1) * tile; ++k) {
            start = fqdsize::combine(start, head[k] ? uint32_t(k) : fqdsize::kNone);
            std::printf("%u\n", start);
        }
    }
    return 0;
}

static int copy()
{
    unsigned label_at, tail;
    unsigned long long size;
    while (std::scanf("%u %u %llu", &label_at, &tail, &size) == 3) {
        const uint32_t rec = label_at + tail, lab = fqdsize::label_len(uint32_t(size)), len = rec + lab;
        std::vector<uint8_t> src(rec), dst(len, 0xEE);       // exactly as long: a load or store outside is the sanitizer's
        for (uint32_t k = 0; k < rec; ++k) src[k] = uint8_t((37u * k + 11u) % 251u);
        for (uint32_t l = 0; l < fqdsize::kSpanLanes; ++l)
            fqdsize::copy_labelled_lane(src.data(), dst.data(), len, label_at, uint32_t(size), l);
        uint8_t text[fqdsize::kMaxLabel];
        (void)fqdsize::write_label(text, uint32_t(size));
        for (uint32_t d = 0; d < len; ++d) {
            const fqdsize::Source from = fqdsize::copy_source(d, label_at, lab);
            if (dst[d] != (from.label ? text[from.at] : src[from.at])) return 3;
            std::printf("%02x", dst[d]);
        }
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "level") == 0) return level();
    if (argc == 2 && std::strcmp(argv[1], "label") == 0) return label();
    if (argc == 2 && std::strcmp(argv[1], "word") == 0) return word();
    if (argc == 2 && std::strcmp(argv[1], "scan") == 0) return scan();
    if (argc == 2 && std::strcmp(argv[1], "copy") == 0) return copy();
    return 2;
}
