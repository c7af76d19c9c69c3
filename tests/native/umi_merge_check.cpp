// CPU harness for csrc/fqd_umi_merge_core.hpp (tests/test_umi_merge_core.py builds it with the sanitizers).
//   stdin: one sequence group a line, "D ULEN JOINERS(hex) FIELD:COUNT,FIELD:COUNT,..." — the group's nodes in the order of
//   their first records, FIELD = the UMI field as it stands in the ID line (ULEN bytes, joiners at the set bits).
//   stdout per line "SWEEPS ROOT:FIRST,ROOT:FIRST,..." — per node the place of its root and the lowest place of its cluster.
//   umi_merge_check rule     merge_group over words packed by pack_word through bases_table
//   umi_merge_check lanes8   what merge_lanes_kernel<8> does with the group (at most 8 nodes): lane_in_edges, lane_sweep and
//   umi_merge_check lanes64  lane_first_of_root (<64>: at most 64 nodes), the lanes played one after another, a sweep reading
//                            the labels the sweep before left
//   umi_merge_check block    what merge_block_kernel does: block_sweep for every node into a second array, then the copy
//   Fields, words, counts and labels are buffers of the exact size: a load or store outside is the sanitizer's to catch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_umi_merge_core.hpp"

using namespace fqdmerge;

struct Group { uint32_t D, W, s; std::vector<uint64_t> P; std::vector<uint32_t> C; };

static Group parse(const std::string& line)
{
    std::istringstream in(line);
    Group g{};
    uint32_t ulen = 0;
    std::string joiners_hex, nodes;
    in >> g.D >> ulen >> joiners_hex >> nodes;
    const uint64_t joiners = std::stoull(joiners_hex, nullptr, 16);
    fqdumi::Table table;
    const uint32_t lb = fqdumi::bases_table(ulen, joiners, &table);
    g.W = words(lb);
    size_t at = 0;
    while (at < nodes.size()) {
        const size_t colon = nodes.find(':', at), comma = nodes.find(',', colon);
        const std::vector<uint8_t> field(nodes.begin() + long(at), nodes.begin() + long(colon));        // (exactly ULEN bytes)
        if (field.size() != ulen) { std::fprintf(stderr, "a field of %zu bytes, not %u\n", field.size(), ulen); std::exit(2); }
        for (uint32_t w = 0; w < g.W; ++w) g.P.push_back(pack_word(field.data(), table, lb, w));
        g.C.push_back(uint32_t(std::stoul(nodes.substr(colon + 1, comma == std::string::npos ? std::string::npos : comma - colon - 1))));
        at = comma == std::string::npos ? nodes.size() : comma + 1;
    }
    g.s = uint32_t(g.C.size());
    return g;
}

static void print(uint32_t sweeps, const std::vector<uint32_t>& root, const std::vector<uint32_t>& first)
{
    std::string out = std::to_string(sweeps) + " ";
    for (size_t v = 0; v < root.size(); ++v) out += (v ? "," : "") + std::to_string(root[v]) + ":" + std::to_string(first[v]);
    std::puts(out.c_str());
}

static void by_rule(const Group& g)
{
    std::vector<uint32_t> root(g.s), first(g.s);
    std::vector<uint64_t> labels(g.s), next(g.s);
    const uint32_t sweeps = merge_group(g.P.data(), g.C.data(), g.s, g.W, g.D, root.data(), first.data(), labels.data(), next.data());
    print(sweeps, root, first);
}

static void by_lanes(const Group& g, uint32_t G)
{
    if (g.s > G) { std::fprintf(stderr, "%u nodes for %u lanes\n", g.s, G); std::exit(2); }
    const uint32_t s_all = G == 64 ? g.s : G;
    std::vector<uint64_t> in_edges(G, 0), label(G, ~0ull);
    for (uint32_t gl = 0; gl < g.s; ++gl) { in_edges[gl] = lane_in_edges(g.P.data(), g.C.data(), g.s, g.W, g.D, gl); label[gl] = label_of(g.C[gl], gl); }
    uint32_t sweeps = 0;
    for (uint32_t t = 1; t <= G; ++t) {
        const std::vector<uint64_t> old = label;
        bool any = false;
        for (uint32_t gl = 0; gl < G; ++gl) {
            label[gl] = lane_sweep(in_edges[gl], old[gl], s_all, [&](uint32_t u) { return old.at(u); });
            any |= label[gl] != old[gl];
        }
        if (!any) break;
        sweeps = t;
    }
    std::vector<uint32_t> root(g.s), first(g.s);
    for (uint32_t gl = 0; gl < g.s; ++gl) {
        root[gl] = label_pos(label[gl]);
        first[gl] = lane_first_of_root(label[gl], s_all, [&](uint32_t u) { return label.at(u); });
    }
    print(sweeps, root, first);
}

static void by_block(const Group& g)
{
    if (g.s > kMaxGroup) { std::fprintf(stderr, "%u nodes for a block\n", g.s); std::exit(2); }
    std::vector<uint64_t> labels(g.s), next(g.s);
    for (uint32_t v = 0; v < g.s; ++v) labels[v] = label_of(g.C[v], v);
    uint32_t sweeps = 0;
    for (uint32_t t = 0; t < g.s; ++t) {
        bool changed = false;
        for (uint32_t v = 0; v < g.s; ++v) { next[v] = block_sweep(g.P.data(), g.C.data(), labels.data(), g.s, g.W, g.D, v); changed |= next[v] != labels[v]; }
        if (!changed) break;
        labels = next;
        ++sweeps;
    }
    std::vector<uint32_t> lowest(g.s, kNoPos), root(g.s), first(g.s);
    for (uint32_t v = 0; v < g.s; ++v) { root[v] = label_pos(labels[v]); if (v < lowest.at(root[v])) lowest[root[v]] = v; }
    for (uint32_t v = 0; v < g.s; ++v) first[v] = lowest[root[v]];
    print(sweeps, root, first);
}

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const Group g = parse(line);
        if (what == "rule") by_rule(g);
        else if (what == "lanes8") by_lanes(g, 8);
        else if (what == "lanes64") by_lanes(g, 64);
        else if (what == "block") by_block(g);
        else { std::fprintf(stderr, "usage: umi_merge_check rule|lanes8|lanes64|block\n"); return 2; }
    }
    return 0;
}
