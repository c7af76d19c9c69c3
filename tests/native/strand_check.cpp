// CPU harness for csrc/fqd_strand_core.hpp (tests/test_strand_core.py builds it with the sanitizers).
//   strand_check canon   stdin: lines "se HEX" / "pe HEX HEX" ("-" = the empty read); stdout per line: the canonical
//                        read(s) in hex and the flipped flag, from se_canon / pe_flipped
//   strand_check lanes   the same lines and answers, from the functions the kernel's sixteen lanes a record run (se_lane_sees,
//                        pe_lane_sees, copy_lane), the lanes played one after another, round by round, into buffers of
//                        the exact size: a load or store outside a read is the sanitizer's to catch
//   strand_check lemma   every string over ACGTN up to length 7: the first place where s and rc(s) differ is at most
//                        (L-1)/2, and se_flipped (which stops at half(L)) agrees with the compare of the whole strings
//   strand_check chunks  comp4 / rc16 / first_diff16 against the bytewise functions: every byte value at every place of
//                        a dword, and random chunks over a small alphabet (so that long equal prefixes occur)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_strand_core.hpp"

using namespace fqdstrand;

static std::vector<uint8_t> unhex(const std::string& h)
{
    std::vector<uint8_t> v;
    if (h == "-") return v;
    for (size_t i = 0; i + 1 < h.size(); i += 2) v.push_back(uint8_t(std::stoul(h.substr(i, 2), nullptr, 16)));
    return v;
}

static std::string hex(const uint8_t* p, size_t n)
{
    if (n == 0) return "-";
    static const char d[] = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
    return s;
}

static int run_canon()
{
    std::string kind, x, y;
    while (std::cin >> kind) {
        if (kind == "se") {
            std::cin >> x;
            const std::vector<uint8_t> s = unhex(x);
            std::vector<uint8_t> out(s.size());                  // exact size: a write beyond it is the sanitizer's to catch
            const bool f = se_canon(s.data(), uint32_t(s.size()), out.data());
            std::cout << hex(out.data(), out.size()) << ' ' << int(f) << '\n';
        } else {
            std::cin >> x >> y;
            const std::vector<uint8_t> a = unhex(x), b = unhex(y);
            const bool f = pe_flipped(a.data(), uint32_t(a.size()), b.data(), uint32_t(b.size()));
            const std::vector<uint8_t>&first = f ? b : a, &second = f ? a : b;
            std::cout << hex(first.data(), first.size()) << ' ' << hex(second.data(), second.size()) << ' ' << int(f) << '\n';
        }
    }
    return 0;
}

// What canon_kernel does with one record: rounds of sixteen looks, the lowest lane that sees a difference decides.
static bool lanes_decide(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb, bool paired)
{
    const uint32_t m = la < lb ? la : lb, chunks = paired ? pe_chunks(m) : se_chunks(la);
    for (uint32_t c0 = 0; c0 < chunks; c0 += 16)
        for (uint32_t gl = 0; gl < 16; ++gl) {
            bool less = false;
            if (paired ? pe_lane_sees(a, b, m, c0, gl, &less) : se_lane_sees(a, la, c0, gl, &less)) return less;
        }
    return paired && lb < la;
}

static void lanes_copy(const std::vector<uint8_t>& src, uint8_t* dst, bool turn)
{
    for (uint32_t gl = 16; gl-- > 0;) copy_lane(src.data(), dst, uint32_t(src.size()), turn, gl);   // (any order of the lanes gives the same bytes)
}

static int run_lanes()
{
    std::string kind, x, y;
    while (std::cin >> kind) {
        if (kind == "se") {
            std::cin >> x;
            const std::vector<uint8_t> s = unhex(x);
            std::vector<uint8_t> out(s.size());
            const bool f = lanes_decide(s.data(), uint32_t(s.size()), nullptr, 0, false);
            lanes_copy(s, out.data(), f);
            std::cout << hex(out.data(), out.size()) << ' ' << int(f) << '\n';
        } else {
            std::cin >> x >> y;
            const std::vector<uint8_t> a = unhex(x), b = unhex(y);
            const bool f = lanes_decide(a.data(), uint32_t(a.size()), b.data(), uint32_t(b.size()), true);
            const std::vector<uint8_t>&first = f ? b : a, &second = f ? a : b;
            std::vector<uint8_t> out(a.size() + b.size());
            lanes_copy(first, out.data(), false);
            lanes_copy(second, out.data() + first.size(), false);
            std::cout << hex(out.data(), first.size()) << ' ' << hex(out.data() + first.size(), second.size()) << ' ' << int(f) << '\n';
        }
    }
    return 0;
}

static int run_lemma()
{
    static const char alphabet[] = "ACGTN";
    unsigned long long checked = 0;
    for (uint32_t L = 0; L <= 7; ++L) {
        uint32_t count = 1;
        for (uint32_t i = 0; i < L; ++i) count *= 5;
        for (uint32_t code = 0; code < count; ++code) {
            std::vector<uint8_t> s(L), r(L);
            for (uint32_t i = 0, c = code; i < L; ++i, c /= 5) s[i] = uint8_t(alphabet[c % 5]);
            for (uint32_t i = 0; i < L; ++i) r[i] = comp(s[L - 1 - i]);
            uint32_t first = L;
            for (uint32_t i = 0; i < L; ++i) if (s[i] != r[i]) { first = i; break; }
            if (first < L && first > (L - 1) / 2) { std::printf("lemma fails: length %u code %u\n", L, code); return 1; }
            const bool whole = first < L && r[first] < s[first];
            if (whole != se_flipped(s.data(), L)) { std::printf("se_flipped differs: length %u code %u\n", L, code); return 1; }
            ++checked;
        }
    }
    std::printf("%llu\n", checked);
    return 0;
}

static int run_chunks()
{
    for (uint32_t b = 0; b < 256; ++b)
        for (int at = 0; at < 4; ++at)
            for (uint32_t fill : {0x00000000u, 0x41414141u, 0x54434754u, 0xFFFFFFFFu, 0x4E4E4E4Eu}) {
                const uint32_t v = (fill & ~(0xFFu << (8 * at))) | (b << (8 * at));
                uint32_t expect = 0;
                for (int k = 0; k < 4; ++k) expect |= uint32_t(comp(uint8_t(v >> (8 * k)))) << (8 * k);
                if (comp4(v) != expect) { std::printf("comp4(%08x) = %08x, not %08x\n", v, comp4(v), expect); return 1; }
            }
    std::mt19937 rng(7);
    static const uint8_t letters[] = {'A', 'C', 'G', 'T', 'N', 'a', 0, 0xFF, 'U', '\n'};
    unsigned long long checked = 0;
    for (int round = 0; round < 200000; ++round) {
        uint8_t x[16], y[16];
        const uint32_t same = rng() % 18;                        // a common prefix of 0 .. 17 bytes
        for (int i = 0; i < 16; ++i) { x[i] = letters[rng() % (round % 2 ? 10 : 5)]; y[i] = uint32_t(i) < same ? x[i] : letters[rng() % (round % 2 ? 10 : 5)]; }
        Chunk cx, cy;
        std::memcpy(&cx, x, 16); std::memcpy(&cy, y, 16);
        uint32_t at = 16; bool less = false;
        for (int i = 15; i >= 0; --i) if (x[i] != y[i]) { at = uint32_t(i); less = y[i] < x[i]; }
        bool got_less = true;
        const uint32_t got = first_diff16(cx, cy, &got_less);
        if (got != at || got_less != less) { std::printf("first_diff16 differs in round %d\n", round); return 1; }
        const Chunk r = rc16(cx);
        uint8_t rb[16];
        std::memcpy(rb, &r, 16);
        for (int i = 0; i < 16; ++i) if (rb[i] != comp(x[15 - i])) { std::printf("rc16 differs in round %d\n", round); return 1; }
        ++checked;
    }
    std::printf("%llu\n", checked);
    return 0;
}

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "canon") return run_canon();
    if (what == "lanes") return run_lanes();
    if (what == "lemma") return run_lemma();
    if (what == "chunks") return run_chunks();
    std::fprintf(stderr, "usage: strand_check canon|lanes|lemma|chunks\n");
    return 2;
}
