// CPU harness for csrc/fqd_near_umi_core.hpp (tests/test_near_umi_core.py builds it with -Werror and the sanitizers): the
// header's host compile, asked over stdin and answered a line a question.  argv[1] says what:
//   tags       lines "hex(joiners) offset hex(U)"; answers the ceil(umi_len / 8) words of T(U) in hex, then the words behind them
//              up to the eighth, which must be 0.  U stands at `offset` in an allocation that ends with its last byte, so a load
//              outside it is the sanitizer's
//   seeds      lines "D len2 weak hex(joiners) hex(U) hex(mate 1)" ("-" for an empty mate); answers the D + 1 tagged keys in hex
//   lanes      lines "hex(joiners) hex(Ua) hex(Ub)"; answers "differ lanes": tags_differ, and the lanes whose words differ, the
//              eight lanes played one after another
//   near       lines "D hex(joiners) hex(Ua) hex(Ub) hex(a1) hex(b1)"; answers 0 or 1 (single-end)
//   molecules  "n m", n lines "owner link", m lines "a b" (near edges); answers the links, the sweeps and labels[owner[i]] for
//              every record: with_links, then fqdnear::components.  A bad link is answered with "bad v" and nothing else
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_near_umi_core.hpp"

using namespace fqdnearumi;

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

uint64_t hex64(const std::string& s) { return std::stoull(s, nullptr, 16); }

} // namespace

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "tags") {
        std::string joiners, u;
        uint32_t offset;
        while (std::cin >> joiners >> offset >> u) {
            const Placed p(unhex(u), offset);
            const Tag t = load_tag(p.p, p.n, hex64(joiners));
            for (uint32_t w = 0; w < kTagWords; ++w) {
                if (t.w[w] != tag_word(p.p, p.n, hex64(joiners), w)) { std::printf("load_tag and tag_word differ\n"); return 0; }
                std::printf("%s%llx", w ? " " : "", static_cast<unsigned long long>(t.w[w]));
            }
            std::printf(" %u\n", tag_words(p.n));
        }
        return 0;
    }
    if (what == "seeds") {
        uint32_t D, len2, weak;
        std::string joiners, u, m1;
        while (std::cin >> D >> len2 >> weak >> joiners >> u >> m1) {
            const Placed pu(unhex(u), 5), p(unhex(m1), 3);
            const Tag t = load_tag(pu.p, pu.n, hex64(joiners));
            for (uint32_t j = 0; j <= D; ++j)
                std::printf("%s%llx", j ? " " : "", static_cast<unsigned long long>(tagged_seed(t, tag_words(pu.n), p.p, p.n, len2, D, j, weak != 0)));
            std::printf("\n");
        }
        return 0;
    }
    if (what == "lanes") {
        std::string joiners, a, b;
        while (std::cin >> joiners >> a >> b) {
            const Placed pa(unhex(a), 1), pb(unhex(b), 6);
            const uint64_t j = hex64(joiners);
            uint32_t lanes = 0;
            for (uint32_t gl = 0; gl < kLanes; ++gl) lanes += tag_word(pa.p, pa.n, j, gl) != tag_word(pb.p, pb.n, j, gl);
            std::printf("%d %u\n", int(tags_differ(pa.p, pb.p, pa.n, j)), lanes);
        }
        return 0;
    }
    if (what == "near") {
        uint32_t D;
        std::string joiners, ua, ub, a1, b1;
        while (std::cin >> D >> joiners >> ua >> ub >> a1 >> b1) {
            const Placed pua(unhex(ua), 2), pub(unhex(ub), 9), pa(unhex(a1), 1), pb(unhex(b1), 5);
            std::printf("%d\n", int(near(pua.p, pub.p, pua.n, hex64(joiners), false, {pa.p, pa.n}, {pa.p, 0}, {pb.p, pb.n}, {pb.p, 0}, D)));
        }
        return 0;
    }
    if (what == "molecules") {
        uint32_t n;
        uint64_t m;
        if (!(std::cin >> n >> m)) return 2;
        std::vector<uint32_t> owner(n), link(n), near_edges(2 * m), edges(2 * (uint64_t(n) + m)), labels(n), next(n);
        for (uint32_t v = 0; v < n; ++v) std::cin >> owner[v] >> link[v];
        for (uint64_t k = 0; k < 2 * m; ++k) std::cin >> near_edges[k];
        for (uint32_t v = 0; v < n; ++v)
            if (owner[v] == v && link[v] != v && !link_is_good(owner.data(), v, link[v])) { std::printf("bad %u\n", v); return 0; }
        const uint64_t all = with_links(owner.data(), link.data(), n, near_edges.data(), m, edges.data());
        const uint32_t sweeps = fqdnear::components(edges.data(), all, n, labels.data(), next.data());
        std::printf("%llu\n%u\n", static_cast<unsigned long long>(all - m), sweeps);
        for (uint32_t v = 0; v < n; ++v) std::printf("%u\n", labels[owner[v]]);
        return 0;
    }
    std::fprintf(stderr, "near_umi_check: what?\n");
    return 2;
}
