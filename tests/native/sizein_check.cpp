// sizein_check.cpp — the rules of FQD_FAST_SIZEIN (fastq-dupaway_amd/csrc/fqd_sizein_core.hpp) on the CPU, the way the device
// runs them.  tests/test_sizein_core.py builds this with the sanitizers and holds it against plain Python.
//   sizein_check parse   < one line per line, in hex      > "weight label_at cut reason" twice: the scalar rule, and the sixteen
//                                                           lanes of size_annotations_kernel played one after another (the
//                                                           line lies in an allocation of exactly its length)
//   sizein_check combine < "h1 s1 h2 s2 h3 s3" per line   > "head sum head sum": (a∘b)∘c and a∘(b∘c); h = -1 is kNone.  A
//                                                           line of two elements "h1 s1" answers x∘id and id∘x
//   sizein_check scan    < "n tile" then n "head weight"  > "start sum" per place, by tiles of `tile` places: tile values,
//                                                           their exclusive combine, then the places — the three launches
//   sizein_check copy    < "label_at cut tail size" lines > the destination in hex: the eight lanes of copy_relabelled_kernel
//                                                           played one after another over a source of exactly label_at + cut +
//                                                           tail bytes (byte k = (37 k + 11) mod 251) and a destination of
//                                                           exactly the grown length; every byte is also held against
//                                                           relabel_source()
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_sizein_core.hpp"

using fqdsizein::Seg;

static fqdsizein::Parsed by_lanes(const uint8_t* line, uint32_t L)
{
    const uint32_t chunks = fqdumi::line_chunks(L);
    uint32_t end = fqdumi::kNone, first = fqdsizein::kNone, count = 0;
    for (uint32_t c0 = 0; end == fqdumi::kNone && c0 < chunks; c0 += 16u) {
        fqdumi::Look k[16];
        uint32_t e = fqdumi::kNone;
        for (uint32_t gl = 0; gl < 16u; ++gl) {
            k[gl] = fqdumi::lane_look(line, L, uint8_t(';'), c0, gl);
            const uint32_t x = fqdumi::look_end(k[gl]);
            e = x < e ? x : e;
        }
        uint32_t f = fqdsizein::kNone, many = 0;
        for (uint32_t gl = 0; gl < 16u; ++gl) {
            const fqdsizein::Cand c = fqdsizein::lane_candidates(line, L, k[gl], e);
            f = c.first < f ? c.first : f;
            many += c.count;
        }
        end = e;
        if (first == fqdsizein::kNone) first = f;
        count += many;
    }
    if (end == fqdumi::kNone) end = L;
    uint32_t digit_mask = 0, semi_mask = 0, other_mask = 0, digit[16];
    for (uint32_t gl = 0; gl < 16u; ++gl) {
        const uint32_t cls = fqdsizein::lane_digit(line, end, first, gl, &digit[gl]);
        digit_mask |= uint32_t(cls == fqdsizein::kDigit) << gl;
        semi_mask |= uint32_t(cls == fqdsizein::kSemi) << gl;
        other_mask |= uint32_t(cls == fqdsizein::kOther) << gl;
    }
    const uint32_t nd = fqdsizein::digits_in_front(digit_mask);
    const uint32_t behind = (semi_mask >> nd) & 1u ? uint32_t(fqdsizein::kSemi) : (other_mask >> nd) & 1u ? uint32_t(fqdsizein::kOther) : uint32_t(fqdsizein::kBehind);
    uint64_t value = 0;
    for (uint32_t gl = 0; gl < 16u; ++gl) value += fqdsizein::lane_value(digit[gl], gl, nd);
    return fqdsizein::judge(count, first, end, nd, behind, value);
}

static int parse()
{
    static char hex[16384];
    while (std::scanf("%16383s", hex) == 1) {
        const size_t len = std::strlen(hex) / 2;
        std::vector<uint8_t> line(len);                      // exactly as long: a load outside is the sanitizer's
        for (size_t k = 0; k < len; ++k) { unsigned b; if (std::sscanf(hex + 2 * k, "%2x", &b) != 1) return 2; line[k] = uint8_t(b); }
        const fqdsizein::Parsed a = fqdsizein::parse(line.data(), uint32_t(len)), b = by_lanes(line.data(), uint32_t(len));
        std::printf("%u %u %u %u %u %u %u %u\n", a.weight, a.label_at, a.cut, a.reason, b.weight, b.label_at, b.cut, b.reason);
    }
    return 0;
}

static Seg seg(long long h, unsigned long long s) { return Seg{s, h < 0 ? fqdsizein::kNone : uint32_t(h), 0u}; }
static void say(const Seg& x) { std::printf("%lld %" PRIu64, x.head == fqdsizein::kNone ? -1ll : (long long)x.head, x.sum); }

static int combine()
{
    char text[512];
    while (std::fgets(text, sizeof text, stdin)) {
        long long h[3];
        unsigned long long s[3];
        const int got = std::sscanf(text, "%lld %llu %lld %llu %lld %llu", &h[0], &s[0], &h[1], &s[1], &h[2], &s[2]);
        if (got == 2) {
            const Seg x = seg(h[0], s[0]);
            say(fqdsizein::combine(x, fqdsizein::seg_none())); std::printf(" "); say(fqdsizein::combine(fqdsizein::seg_none(), x)); std::printf("\n");
        } else if (got == 6) {
            const Seg a = seg(h[0], s[0]), b = seg(h[1], s[1]), c = seg(h[2], s[2]);
            say(fqdsizein::combine(fqdsizein::combine(a, b), c)); std::printf(" "); say(fqdsizein::combine(a, fqdsizein::combine(b, c))); std::printf("\n");
        } else return 2;
    }
    return 0;
}

static int scan()
{
    unsigned long long n = 0, tile = 0;
    if (std::scanf("%llu %llu", &n, &tile) != 2 || !tile) return 2;
    std::vector<uint8_t> head(n);
    std::vector<uint32_t> weight(n);
    for (uint64_t k = 0; k < n; ++k) { unsigned h, w; if (std::scanf("%u %u", &h, &w) != 2) return 2; head[k] = uint8_t(h); weight[k] = w; }
    const uint64_t tiles = (n + tile - 1) / tile;
    std::vector<Seg> value(tiles, fqdsizein::seg_none()), carry(tiles, fqdsizein::seg_none());
    for (uint64_t t = 0; t < tiles; ++t)
        for (uint64_t k = t * tile; k < n && k < (t + 1) * tile; ++k)
            value[t] = fqdsizein::combine(value[t], fqdsizein::seg_of(head[k] != 0, uint32_t(k), weight[k]));
    for (uint64_t t = 1; t < tiles; ++t) carry[t] = fqdsizein::combine(carry[t - 1], value[t - 1]);
    for (uint64_t t = 0; t < tiles; ++t) {
        Seg cur = carry[t];
        for (uint64_t k = t * tile; k < n && k < (t + 1) * tile; ++k) {
            cur = fqdsizein::combine(cur, fqdsizein::seg_of(head[k] != 0, uint32_t(k), weight[k]));
            say(cur); std::printf("\n");
        }
    }
    return 0;
}

static int copy()
{
    unsigned label_at, cut, tail;
    unsigned long long size;
    while (std::scanf("%u %u %u %llu", &label_at, &cut, &tail, &size) == 4) {
        const uint32_t rec = label_at + cut + tail, lab = fqdsize::label_len(uint32_t(size)), len = fqdsizein::relabelled_len(rec, cut, uint32_t(size));
        std::vector<uint8_t> src(rec), dst(len, 0xEE);       // exactly as long: a load or store outside is the sanitizer's
        for (uint32_t k = 0; k < rec; ++k) src[k] = uint8_t((37u * k + 11u) % 251u);
        for (uint32_t l = 0; l < fqdsize::kSpanLanes; ++l)
            fqdsizein::copy_relabelled_lane(src.data(), dst.data(), len, label_at, cut, uint32_t(size), l);
        uint8_t text[fqdsize::kMaxLabel];
        (void)fqdsize::write_label(text, uint32_t(size));
        for (uint32_t d = 0; d < len; ++d) {
            const fqdsize::Source from = fqdsizein::relabel_source(d, label_at, cut, lab);
            if (!from.label && from.at >= rec) return 3;
            if (dst[d] != (from.label ? text[from.at] : src[from.at])) return 3;
            std::printf("%02x", dst[d]);
        }
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "parse") == 0) return parse();
    if (argc == 2 && std::strcmp(argv[1], "combine") == 0) return combine();
    if (argc == 2 && std::strcmp(argv[1], "scan") == 0) return scan();
    if (argc == 2 && std::strcmp(argv[1], "copy") == 0) return copy();
    return 2;
}
