// CPU harness for csrc/fqd_near_core.hpp (tests/test_near_core.py builds it with -Werror and the sanitizers): the header's
// host compile, asked over stdin and answered a line a question.  argv[1] says what:
//   bounds      no input; for D = 1 .. 3 and len = 0 .. 40 a line "D len b_0 .. b_(D+1)"
//   pigeonhole  no input; every pair of strings over three letters up to length 7, D = 1 .. 3: a pair within D differences must
//               agree on a whole segment and share that segment's seed key.  Prints "pairs P near Q" or says what failed.
//   seeds       lines "D len2 weak hex(mate 1)"; answers the D + 1 keys in hex
//   mismatch    lines "cap offset hex(a) hex(b)"; answers "lanes rule": lanes_mismatches and fqdseq::mismatches.  The bytes
//               stand at `offset` in an allocation that ends with their last byte, so a load outside them is the sanitizer's
//   near        lines "D paired hex(a1) hex(a2) hex(b1) hex(b2)" ("-" for an empty mate); answers 0 or 1
//   sweeps      "n m" and m lines "a b"; answers the sweeps and the n labels
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_near_core.hpp"

using namespace fqdnear;

namespace {

std::vector<uint8_t> unhex(const std::string& s)
{
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t k = 0; k + 1 < s.size(); k += 2) out.push_back(uint8_t(std::stoul(s.substr(k, 2), nullptr, 16)));
    return out;
}

// The bytes at `offset` in an allocation of exactly offset + size bytes.
struct Placed {
    std::unique_ptr<uint8_t[]> room; const uint8_t* p; uint32_t n;
    Placed(const std::vector<uint8_t>& bytes, size_t offset = 0) : room(new uint8_t[offset + bytes.size()]), p(room.get() + offset), n(uint32_t(bytes.size()))
    {
        if (!bytes.empty()) std::memcpy(room.get() + offset, bytes.data(), bytes.size());
    }
};

int pigeonhole()
{
    unsigned long long pairs = 0, near_pairs = 0;
    for (uint32_t len = 0; len <= 7; ++len) {
        uint32_t count = 1;
        for (uint32_t k = 0; k < len; ++k) count *= 3;
        std::vector<std::vector<uint8_t>> all(count, std::vector<uint8_t>(len));
        for (uint32_t v = 0; v < count; ++v) for (uint32_t k = 0, x = v; k < len; ++k, x /= 3) all[v][k] = "ACN"[x % 3];
        std::vector<Placed> placed;
        for (uint32_t v = 0; v < count; ++v) placed.emplace_back(all[v], v % 16);
        for (uint32_t D = 1; D <= 3; ++D)
            for (uint32_t a = 0; a < count; ++a) {
                const Placed& pa = placed[a];
                for (uint32_t b = a + 1; b < count; ++b) {
                    const Placed& pb = placed[b];
                    ++pairs;
                    if (fqdseq::mismatches(pa.p, pb.p, len, len) > D) continue;
                    ++near_pairs;
                    bool segment = false, key = false;
                    for (uint32_t j = 0; j <= D; ++j) {
                        const uint32_t from = bound(len, D, j), to = bound(len, D, j + 1);
                        segment |= std::memcmp(pa.p + from, pb.p + from, to - from) == 0;
                        key |= node_seed(pa.p, len, 0, D, j, false) == node_seed(pb.p, len, 0, D, j, false);
                    }
                    if (!segment || !key) { std::printf("failed len %u D %u a %u b %u segment %d key %d\n", len, D, a, b, int(segment), int(key)); return 0; }
                }
            }
    }
    std::printf("pairs %llu near %llu\n", pairs, near_pairs);
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "bounds") {
        for (uint32_t D = 1; D <= 3; ++D)
            for (uint32_t len = 0; len <= 40; ++len) {
                std::printf("%u %u", D, len);
                for (uint32_t j = 0; j <= D + 1; ++j) std::printf(" %u", bound(len, D, j));
                std::printf("\n");
            }
        return 0;
    }
    if (what == "pigeonhole") return pigeonhole();
    if (what == "seeds") {
        uint32_t D, len2, weak;
        std::string m1;
        while (std::cin >> D >> len2 >> weak >> m1) {
            const Placed p(unhex(m1), 3);
            for (uint32_t j = 0; j <= D; ++j) std::printf("%s%llx", j ? " " : "", static_cast<unsigned long long>(node_seed(p.p, p.n, len2, D, j, weak != 0)));
            std::printf("\n");
        }
        return 0;
    }
    if (what == "mismatch") {
        uint32_t cap, offset;
        std::string a, b;
        while (std::cin >> cap >> offset >> a >> b) {
            const Placed pa(unhex(a), offset), pb(unhex(b), (offset * 5 + 1) % 16);
            std::printf("%u %u\n", lanes_mismatches(pa.p, pb.p, pa.n, cap), fqdseq::mismatches(pa.p, pb.p, pa.n, cap));
        }
        return 0;
    }
    if (what == "near") {
        uint32_t D, paired;
        std::string a1, a2, b1, b2;
        while (std::cin >> D >> paired >> a1 >> a2 >> b1 >> b2) {
            const Placed pa1(unhex(a1), 1), pa2(unhex(a2), 2), pb1(unhex(b1), 5), pb2(unhex(b2), 7);
            std::printf("%d\n", int(near(paired != 0, {pa1.p, pa1.n}, {pa2.p, pa2.n}, {pb1.p, pb1.n}, {pb2.p, pb2.n}, D)));
        }
        return 0;
    }
    if (what == "sweeps") {
        uint32_t n;
        uint64_t m;
        if (!(std::cin >> n >> m)) return 2;
        std::vector<uint32_t> edges(2 * m), labels(n), next(n);
        for (uint64_t k = 0; k < 2 * m; ++k) std::cin >> edges[k];
        const uint32_t sweeps = components(edges.data(), m, n, labels.data(), next.data());
        std::printf("%u\n", sweeps);
        for (uint32_t v = 0; v < n; ++v) std::printf("%u\n", labels[v]);
        return 0;
    }
    std::fprintf(stderr, "near_check: what?\n");
    return 2;
}
