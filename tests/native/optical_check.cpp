// CPU harness for csrc/fqd_optical_core.hpp (tests/test_optical_core.py builds it with the sanitizers).
//   optical_check parse      stdin: one ID line a line, as hex (so that blanks, tabs and '\r' travel); the first line is
//   optical_check lanes16    record 0.  stdout per line "REASON TILE X Y SURFACE(hex)", SURFACE with the same-surface bit.
//                            parse: the rule record by record; lanes16: what read_places_kernel does, the sixteen lanes of a
//                            record played one after another through lane_look, lane_colons, field_number and judge.
//   optical_check rule       stdin: one cluster a line, "D SURFACE0 SURFACE|TILE|X|Y;SURFACE|TILE|X|Y;..." — the members in
//   optical_check lanes8     input order, SURFACE0 = record 0's surface (the members that have it carry the bit).
//   optical_check lanes64    stdout per line "SWEEPS LABEL,LABEL,..." — per member the lowest place of its optical group.
//   optical_check block      rule: split_cluster; lanes8 / lanes64: what split_lanes_kernel does with the cluster (at most 8 /
//                            64 members): lane_neighbours, lane_min and the jump, the lanes played one after another, a step
//                            reading what the step before left; block: what split_block_kernel and the large tier do:
//                            array_min for every member into a second array, then the jump.
//   Lines, surfaces, places and labels are buffers of the exact size: a load or store outside is the sanitizer's to catch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_optical_core.hpp"

using namespace fqdoptical;

static std::vector<uint8_t> unhex(const std::string& s)
{
    std::vector<uint8_t> out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back(uint8_t(std::stoul(s.substr(i, 2), nullptr, 16)));
    return out;
}

// (nothing is promised about the place of a refused record: zeros stand for it)
static void print_place(const Place& p) { if (p.reason) std::printf("%u 0 0 0 0\n", p.reason); else std::printf("0 %u %u %u %x\n", p.tile, p.x, p.y, p.surface); }

static Place by_parse(const std::vector<uint8_t>& line0, const std::vector<uint8_t>& line)
{
    Place p = parse(line.data(), uint32_t(line.size()));
    if (p.reason == kOk && surface_is_record0s(line0.data(), uint32_t(line0.size()), line.data(), p.surface + 1u)) p.surface |= kSameSurface;
    return p;
}

static Place by_lanes16(const std::vector<uint8_t>& line0, const std::vector<uint8_t>& line_)
{
    const uint8_t* line = line_.data();
    const uint32_t L = uint32_t(line_.size()), chunks = fqdumi::line_chunks(L);
    uint32_t end = fqdumi::kNone, colons = 0, c[4] = {kNone, kNone, kNone, kNone};
    bool empty = false;
    for (uint32_t c0 = 0; end == fqdumi::kNone && c0 < chunks; c0 += kGroup) {
        fqdumi::Look k[kGroup];
        uint32_t e = fqdumi::kNone;
        for (uint32_t gl = 0; gl < kGroup; ++gl) { k[gl] = fqdumi::lane_look(line, L, uint8_t(':'), c0, gl); e = std::min(e, fqdumi::look_end(k[gl])); }
        uint32_t before = colons;
        for (uint32_t gl = 0; gl < kGroup; ++gl) {
            const uint32_t own = uint32_t(__builtin_popcount(colons_below(k[gl], e)));
            if (own) {
                const Colons got = lane_colons(line, k[gl], e, before);
                for (int f = 0; f < 4; ++f) if (c[f] == kNone) c[f] = got.at[f];
                empty |= got.empty;
            }
            before += own;
        }
        colons = before;
        end = e;
    }
    if (end == fqdumi::kNone) end = L;
    uint32_t reasons[3] = {kOk, kOk, kOk}, values[3] = {0u, 0u, 0u};
    if (colons >= 6u && !empty && c[2] + 1u < (colons >= 7u ? c[3] : end))
        for (uint32_t gl = 0; gl < 3u; ++gl) reasons[gl] = field_number(line, c, colons, end, gl, &values[gl]);
    Place p = judge(colons, c, end, empty, reasons, values);
    if (p.reason == kOk) {
        bool differs = false;
        for (uint32_t gl = 0; gl < kGroup; ++gl)
            for (uint32_t b = 1u + gl; b <= c[0]; b += kGroup) differs |= !surface_byte_same(line0.data(), uint32_t(line0.size()), line, b);
        if (!differs) p.surface |= kSameSurface;
    }
    return p;
}

struct Cluster { uint32_t D, s; std::vector<uint32_t> T, X, Y, S; std::vector<std::vector<uint8_t>> bytes; };

static Cluster read_cluster(const std::string& line)
{
    std::istringstream in(line);
    Cluster g{};
    std::string surface0, members;
    in >> g.D >> surface0 >> members;
    size_t at = 0;
    while (at < members.size()) {
        size_t semi = members.find(';', at);
        if (semi == std::string::npos) semi = members.size();
        const std::string m = members.substr(at, semi - at);
        const size_t a = m.find('|'), b = m.find('|', a + 1), c = m.find('|', b + 1);
        const std::string surface = m.substr(0, a);
        g.bytes.emplace_back(surface.begin(), surface.end());                                       // (exactly the surface's bytes)
        g.T.push_back(uint32_t(std::stoul(m.substr(a + 1, b - a - 1))));
        g.X.push_back(uint32_t(std::stoul(m.substr(b + 1, c - b - 1))));
        g.Y.push_back(uint32_t(std::stoul(m.substr(c + 1))));
        g.S.push_back(uint32_t(surface.size()) | (surface == surface0 ? kSameSurface : 0u));
        at = semi + 1;
    }
    g.s = uint32_t(g.T.size());
    return g;
}

static void print(uint32_t sweeps, const std::vector<uint32_t>& labels, uint32_t s)
{
    std::string out = std::to_string(sweeps) + " ";
    for (uint32_t v = 0; v < s; ++v) out += (v ? "," : "") + std::to_string(labels[v]);
    std::puts(out.c_str());
}

static void by_rule(const Cluster& g)
{
    std::vector<uint32_t> labels(g.s), next(g.s);
    const uint32_t sweeps = split_cluster(g.T.data(), g.X.data(), g.Y.data(), g.S.data(), g.s, g.D, labels.data(), next.data(),
                                          [&](uint32_t u) { return g.bytes.at(u).data(); });
    print(sweeps, labels, g.s);
}

static void by_lanes(const Cluster& g, uint32_t G)
{
    if (g.s > G) { std::fprintf(stderr, "%u members for %u lanes\n", g.s, G); std::exit(2); }
    const uint32_t s_all = G == 64 ? g.s : G;
    static const uint8_t nothing[1] = {0};
    auto place_of = [&](uint32_t u, uint32_t* t, uint32_t* x, uint32_t* y, uint32_t* s) {
        if (u < g.s) { *t = g.T[u]; *x = g.X[u]; *y = g.Y[u]; *s = g.S[u]; } else { *t = *x = *y = *s = 0; }      // (a lane without a member holds zeros)
    };
    auto bytes_of = [&](uint32_t u) { return u < g.s ? g.bytes[u].data() : nothing; };
    std::vector<uint64_t> neighbours(G, 0);
    std::vector<uint32_t> label(G);
    for (uint32_t gl = 0; gl < G; ++gl) {
        uint32_t t, x, y, s;
        place_of(gl, &t, &x, &y, &s);
        neighbours[gl] = lane_neighbours(gl < g.s, gl, g.s, s_all, t, x, y, s, bytes_of(gl), g.D, place_of, bytes_of);
        label[gl] = gl;
    }
    uint32_t sweeps = 0;
    for (uint32_t round = 1; round <= G; ++round) {
        const std::vector<uint32_t> old = label;
        std::vector<uint32_t> low(G);
        bool any = false;
        for (uint32_t gl = 0; gl < G; ++gl) { low[gl] = lane_min(neighbours[gl], old[gl], s_all, [&](uint32_t u) { return old.at(u); }); any |= low[gl] != old[gl]; }
        if (!any) break;
        for (uint32_t gl = 0; gl < G; ++gl) label[gl] = low.at(low[gl]);
        sweeps = round;
    }
    print(sweeps, label, g.s);
}

static void by_block(const Cluster& g)
{
    std::vector<uint32_t> labels(g.s), next(g.s);
    for (uint32_t v = 0; v < g.s; ++v) labels[v] = v;
    uint32_t sweeps = 0;
    for (uint32_t round = 0; round < g.s; ++round) {
        bool changed = false;
        for (uint32_t v = 0; v < g.s; ++v) {
            next[v] = array_min(g.T.data(), g.X.data(), g.Y.data(), g.S.data(), labels.data(), g.s, g.D, v, [&](uint32_t u) { return g.bytes.at(u).data(); });
            changed |= next[v] != labels[v];
        }
        if (!changed) break;
        for (uint32_t v = 0; v < g.s; ++v) labels[v] = next.at(next[v]);
        ++sweeps;
    }
    print(sweeps, labels, g.s);
}

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    std::string line;
    std::vector<uint8_t> line0;
    bool have0 = false;
    while (std::getline(std::cin, line)) {
        if (what == "parse" || what == "lanes16") {
            const std::vector<uint8_t> bytes = unhex(line);                                         // (an empty line: a line of no bytes)
            if (!have0) { line0 = bytes; have0 = true; }
            print_place(what == "parse" ? by_parse(line0, bytes) : by_lanes16(line0, bytes));
            continue;
        }
        if (line.empty()) continue;
        const Cluster g = read_cluster(line);
        if (what == "rule") by_rule(g);
        else if (what == "lanes8") by_lanes(g, 8);
        else if (what == "lanes64") by_lanes(g, 64);
        else if (what == "block") by_block(g);
        else { std::fprintf(stderr, "usage: optical_check parse|lanes16|rule|lanes8|lanes64|block\n"); return 2; }
    }
    return 0;
}
