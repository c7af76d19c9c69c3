// CPU harness for csrc/fqd_prefix_core.hpp and csrc/fqd_groups_core.hpp (tests/test_prefix_core.py builds it with -Werror and
// the sanitizers): the headers' host compile, asked over stdin and answered a line a question.  argv[1] says what:
//   seeds      lines "paired L weak offset hex(first L bytes of mate 1) hex(of mate 2)" ("-" for none); answers the key in hex.
//              The L bytes stand at `offset` in an allocation that ends with their last byte, so a load outside them is the
//              sanitizer's
//   overlap    lines "offset hex(a) hex(b)" of one length n; answers "equal rounds": lanes_equal over the n bytes and the rounds
//              it played.  Both stand in allocations of exactly their bytes
//   direction  lines "paired a1 a2 b1 b2" (lengths); answers 0, 1 or 2
//   pack       lines "span node"; answers pack(span, node) in decimal
//   forest     "paired L n" and n lines "hex(mate 1) hex(mate 2)" of DISTINCT nodes, node v = line v: every pair of eligible
//              nodes through related(), best by the minimum of pack(), then trees().  Answers "jumps deepest" and n lines
//              "parent root" (a node without a parent is its own)
//   jumps      "n" and n lines up[v]; best[v] = (1 << 32 | up[v]), all ones where up[v] == v; answers as forest does
//   groups     "N" and N sorted keys in decimal; answers N lines "start end" from group_start and group_end
//   exhaust    "letters maxlen L sample seed": every set of strings of length 1 .. maxlen over the first `letters` of "ACGT" where
//              there are at most 16 such strings, `sample` random sets otherwise (sample 0: the one set of all of them); for
//              each set the parents, the trees, and what the header proves — parents grow in span, every member is a prefix
//              of its root, no root has a parent, and two roots never share a first record.  Prints "sets S nodes X children Y
//              deepest D" or says what failed
//   exhaust2   "sample seed L": `sample` random sets of PAIRS of strings of length 1 .. 3 over two letters, likewise
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_groups_core.hpp"
#include "../../fastq-dupaway_amd/csrc/fqd_prefix_core.hpp"

using namespace fqdprefix;

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
    fqdseq::View view() const { return {p, n}; }
};

struct Node { Placed m1, m2; };

// best[] of the nodes by all pairs, as verification fills it: related() decides, pack() orders.
std::vector<uint64_t> parents_of(const std::vector<Node>& nodes, bool paired, uint32_t L)
{
    std::vector<uint64_t> best(nodes.size(), kNoParent);
    for (size_t a = 0; a < nodes.size(); ++a)
        for (size_t b = a + 1; b < nodes.size(); ++b) {
            if (!eligible(paired, nodes[a].m1.n, nodes[a].m2.n, L) || !eligible(paired, nodes[b].m1.n, nodes[b].m2.n, L)) continue;
            const int dir = related(paired, nodes[a].m1.view(), nodes[a].m2.view(), nodes[b].m1.view(), nodes[b].m2.view());
            if (dir == 0) continue;
            const size_t s = dir == 1 ? a : b, l = dir == 1 ? b : a;
            best[s] = std::min(best[s], pack(nodes[l].m1.n + (paired ? nodes[l].m2.n : 0u), uint32_t(l)));
        }
    return best;
}

struct Forest { std::vector<uint32_t> parent, root; uint32_t jumps = 0, deepest = 0; };

Forest forest_of(const std::vector<uint64_t>& best)
{
    const uint32_t n = uint32_t(best.size());
    Forest f;
    std::vector<uint32_t> up(n), other(n);
    const uint32_t* roots = nullptr;
    f.jumps = trees(best.data(), n, up.data(), other.data(), &roots, &f.deepest);
    f.root.assign(roots, roots + n);
    for (uint32_t v = 0; v < n; ++v) f.parent.push_back(parent_of(best[v], v));
    return f;
}

void print(const Forest& f)
{
    std::printf("%u %u\n", f.jumps, f.deepest);
    for (size_t v = 0; v < f.parent.size(); ++v) std::printf("%u %u\n", f.parent[v], f.root[v]);
}

bool begins(const Placed& a, const Placed& b) { return a.n <= b.n && std::memcmp(a.p, b.p, a.n) == 0; }

// What the header proves, held against one set.  Returns "" or what failed.
std::string theorems(const std::vector<Node>& nodes, bool paired, uint32_t L, unsigned long long& children, uint32_t& deepest)
{
    const std::vector<uint64_t> best = parents_of(nodes, paired, L);
    const Forest f = forest_of(best);
    const uint32_t n = uint32_t(nodes.size());
    std::vector<uint32_t> first(n, 0xFFFFFFFFu);
    auto span = [&](uint32_t v) { return nodes[v].m1.n + (paired ? nodes[v].m2.n : 0u); };
    for (uint32_t v = 0; v < n; ++v) {
        const uint32_t r = f.root[v];
        first[r] = std::min(first[r], v);
        if (has_parent(best[r])) return "a root has a parent";
        if (f.parent[v] != v) {
            ++children;
            if (span(f.parent[v]) <= span(v)) return "a parent's span does not grow";
            if (!eligible(paired, nodes[v].m1.n, nodes[v].m2.n, L)) return "a node that is not eligible has a parent";
            if (r == v || !begins(nodes[v].m1, nodes[r].m1) || (paired && !begins(nodes[v].m2, nodes[r].m2))) return "a member is no prefix of its root";
        } else if (r != v) return "a node without a parent is not its own root";
    }
    std::vector<uint32_t> owners;
    for (uint32_t v = 0; v < n; ++v) if (f.root[v] == v) owners.push_back(first[v]);
    std::sort(owners.begin(), owners.end());
    if (std::adjacent_find(owners.begin(), owners.end()) != owners.end()) return "two roots in one cluster";
    if (f.jumps != (f.deepest > 1 ? 32u - uint32_t(__builtin_clz(f.deepest - 1)) : 0u)) return "the jumps are not ceil(log2(deepest))";
    deepest = std::max(deepest, f.deepest);
    return "";
}

std::vector<std::vector<uint8_t>> strings_up_to(uint32_t letters, uint32_t maxlen)
{
    std::vector<std::vector<uint8_t>> all;
    for (uint32_t len = 1; len <= maxlen; ++len) {
        uint32_t count = 1;
        for (uint32_t k = 0; k < len; ++k) count *= letters;
        for (uint32_t v = 0; v < count; ++v) {
            std::vector<uint8_t> s(len);
            for (uint32_t k = 0, x = v; k < len; ++k, x /= letters) s[k] = uint8_t("ACGT"[x % letters]);
            all.push_back(s);
        }
    }
    return all;
}

int exhaust(bool paired)
{
    uint32_t letters = 2, maxlen = 3, L = 1;
    unsigned long long sample = 0, seed = 0;
    if (paired) { if (!(std::cin >> sample >> seed >> L)) return 2; }
    else if (!(std::cin >> letters >> maxlen >> L >> sample >> seed)) return 2;
    const auto all = strings_up_to(letters, maxlen);
    std::vector<std::pair<uint32_t, uint32_t>> items;                                  // a node = one string, or a pair of them
    if (paired) { for (uint32_t a = 0; a < all.size(); ++a) for (uint32_t b = 0; b < all.size(); ++b) items.push_back({a, b}); }
    else for (uint32_t a = 0; a < all.size(); ++a) items.push_back({a, 0});
    std::mt19937_64 rng(seed);
    const bool every = !paired && all.size() <= 16;
    const unsigned long long sets = every ? 1ull << all.size() : std::max<unsigned long long>(sample, 1);
    unsigned long long total = 0, children = 0;
    uint32_t deepest = 0;
    for (unsigned long long s = 0; s < sets; ++s) {
        std::vector<Node> nodes;
        std::vector<uint32_t> order;
        for (uint32_t k = 0; k < items.size(); ++k) {
            const bool in = every ? (s >> k) & 1 : sample == 0 || rng() % 3 == 0;
            if (in) order.push_back(k);
        }
        std::shuffle(order.begin(), order.end(), rng);                                // record numbers say nothing about lengths
        for (uint32_t k : order) nodes.push_back(Node{Placed(all[items[k].first], k % 16), Placed(paired ? all[items[k].second] : std::vector<uint8_t>(), 3)});
        total += nodes.size();
        const std::string failed = theorems(nodes, paired, L, children, deepest);
        if (!failed.empty()) { std::printf("failed: %s (set %llu of %llu, L %u)\n", failed.c_str(), s, sets, L); return 0; }
    }
    std::printf("sets %llu nodes %llu children %llu deepest %u\n", sets, total, children, deepest);
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "seeds") {
        uint32_t paired, L, weak, offset;
        std::string m1, m2;
        while (std::cin >> paired >> L >> weak >> offset >> m1 >> m2) {
            const Placed p1(unhex(m1), offset), p2(unhex(m2), (offset * 7 + 3) % 16);
            std::printf("%llx\n", static_cast<unsigned long long>(node_seed(paired != 0, p1.p, paired ? p2.p : nullptr, L, weak != 0)));
        }
        return 0;
    }
    if (what == "overlap") {
        uint32_t offset;
        std::string a, b;
        while (std::cin >> offset >> a >> b) {
            const Placed pa(unhex(a), offset), pb(unhex(b), (offset * 5 + 1) % 16);
            uint32_t rounds = 0;
            const bool equal = lanes_equal(pa.p, pb.p, pa.n, &rounds);
            std::printf("%d %u\n", int(equal), rounds);
        }
        return 0;
    }
    if (what == "direction") {
        uint32_t paired, a1, a2, b1, b2;
        while (std::cin >> paired >> a1 >> a2 >> b1 >> b2) std::printf("%d\n", direction(paired != 0, a1, a2, b1, b2));
        return 0;
    }
    if (what == "pack") {
        uint32_t span, node;
        while (std::cin >> span >> node) std::printf("%llu\n", static_cast<unsigned long long>(pack(span, node)));
        return 0;
    }
    if (what == "forest") {
        uint32_t paired, L, n;
        if (!(std::cin >> paired >> L >> n)) return 2;
        std::vector<Node> nodes;
        for (uint32_t v = 0; v < n; ++v) {
            std::string m1, m2;
            std::cin >> m1 >> m2;
            nodes.push_back(Node{Placed(unhex(m1), v % 16), Placed(unhex(m2), (v * 3 + 1) % 16)});
        }
        print(forest_of(parents_of(nodes, paired != 0, L)));
        return 0;
    }
    if (what == "jumps") {
        uint32_t n;
        if (!(std::cin >> n)) return 2;
        std::vector<uint64_t> best(n);
        for (uint32_t v = 0; v < n; ++v) { uint32_t up; std::cin >> up; best[v] = up == v ? kNoParent : pack(1, up); }
        print(forest_of(best));
        return 0;
    }
    if (what == "groups") {
        uint64_t N;
        if (!(std::cin >> N)) return 2;
        std::vector<uint64_t> keys(N);
        for (uint64_t k = 0; k < N; ++k) std::cin >> keys[k];
        for (uint64_t e = 0; e < N; ++e)
            std::printf("%llu %llu\n", static_cast<unsigned long long>(fqdgroups::group_start(keys.data(), e)), static_cast<unsigned long long>(fqdgroups::group_end(keys.data(), N, e)));
        return 0;
    }
    if (what == "exhaust") return exhaust(false);
    if (what == "exhaust2") return exhaust(true);
    std::fprintf(stderr, "prefix_check: what?\n");
    return 2;
}
