// CPU harness for csrc/fqd_umi_core.hpp (tests/test_umi_core.py builds it with the sanitizers).
//   umi_check rule       stdin: lines "SEP HEXLINE HEXSEQ ALIGN" (SEP = c or u, "-" = no bytes, ALIGN = 0 .. 15); stdout per
//                        line "REASON OFF" for a line the rule refuses on its own, else "0 OFF ULEN JOINERS(hex) KEYED(hex)"
//                        with KEYED = B(U) ‖ seq: from judge, bases_table and plain loops
//   umi_check lanes      the same lines and answers, from the functions the kernels' sixteen lanes a record run (lane_look,
//                        look_end, look_sep, lane_class, verdict, gather_lane, fqdstrand::copy_lane), the lanes played one
//                        after another, round by round; the line, the sequence and the destination (ALIGN bytes behind a
//                        16-byte boundary) are buffers of the exact size: a load or store outside is the sanitizer's to catch
//   umi_check file       stdin: lines "SEP HEXLINE", the records of one run; stdout "BAD_RECORD REASON ULEN0 JOINERS0(hex) LB"
//                        (BAD_RECORD -1: none) with the lanes played as above and record 0's shape handed to the others
//   umi_check injective  every U over ACGTN+ up to length 5, by shape: all B of a shape have one length and are pairwise
//                        different, and so are B ‖ seq over a few sequences; prints the strings checked and the shapes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_strand_core.hpp"
#include "../../fastq-dupaway_amd/csrc/fqd_umi_core.hpp"

using namespace fqdumi;

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

struct Judged { uint32_t reason, off, ulen; uint64_t joiners; };

static Judged by_rule(const std::vector<uint8_t>& line, uint8_t sep, bool have0, uint32_t ulen0, uint64_t joiners0)
{
    Field f; uint64_t j = 0;
    const uint32_t reason = judge(line.data(), uint32_t(line.size()), sep, have0, ulen0, joiners0, &f, &j);
    return Judged{reason, f.off, f.len, j};
}

// What umi_find_kernel does with one record: rounds of sixteen looks while no lane has seen the word's end, the group's
// minimum and maximum, four bytes of the field a lane, the verdict.
static Judged by_lanes(const std::vector<uint8_t>& line, uint8_t sep, bool have0, uint32_t ulen0, uint64_t joiners0)
{
    const uint8_t* p = line.data();
    const uint32_t L = uint32_t(line.size()), chunks = line_chunks(L);
    uint32_t end = kNone, sep1 = 0;
    for (uint32_t c0 = 0; end == kNone && c0 < chunks; c0 += 16) {
        Look k[16];
        for (uint32_t gl = 0; gl < 16; ++gl) k[gl] = lane_look(p, L, sep, c0, gl);
        uint32_t e = kNone, s = 0;
        for (uint32_t gl = 0; gl < 16; ++gl) { const uint32_t x = look_end(k[gl]); e = x < e ? x : e; }
        for (uint32_t gl = 0; gl < 16; ++gl) { const uint32_t x = look_sep(k[gl], e); s = x > s ? x : s; }
        end = e;
        if (s) sep1 = s;
    }
    if (end == kNone) end = L;
    const bool has_sep = sep1 != 0;
    const uint32_t ulen = has_sep ? end - sep1 : 0;
    uint64_t joiners = 0;
    bool any_bad = false;
    if (has_sep && ulen <= kMaxUmi)
        for (uint32_t gl = 0; gl < 16; ++gl) {
            uint32_t j4 = 0; bool bad = false;
            lane_class(p + sep1, ulen, gl, &j4, &bad);
            for (uint32_t k = 0; k < 4; ++k) joiners |= uint64_t((j4 >> k) & 1u) << (gl + 16 * k);
            any_bad |= bad;
        }
    return Judged{verdict(has_sep, ulen, joiners, any_bad, have0, ulen0, joiners0), sep1, ulen, joiners};
}

static int run_records(bool lanes)
{
    std::string sep_name, hl, hs;
    int align = 0;
    while (std::cin >> sep_name >> hl >> hs >> align) {
        const uint8_t sep = sep_name == "c" ? ':' : '_';
        const std::vector<uint8_t> line = unhex(hl), seq = unhex(hs);
        const Judged j = lanes ? by_lanes(line, sep, false, 0, 0) : by_rule(line, sep, false, 0, 0);
        if (j.reason) { std::cout << j.reason << ' ' << j.off << '\n'; continue; }
        Table t;
        const uint32_t lb = bases_table(j.ulen, j.joiners, &t);
        const size_t total = size_t(lb) + seq.size();
        void* raw = nullptr;
        if (posix_memalign(&raw, 16, size_t(align) + total + (align + total == 0 ? 1 : 0)) != 0) return 3;   // exact size behind the alignment
        uint8_t* buf = static_cast<uint8_t*>(raw);
        std::memset(buf, 0xEE, size_t(align));
        uint8_t* dst = buf + align;
        if (lanes) {
            for (uint32_t gl = 16; gl-- > 0;) {                  // (any order of the lanes gives the same bytes)
                gather_lane(line.data() + j.off, t, lb, dst, gl);
                fqdstrand::copy_lane(seq.data(), dst + lb, uint32_t(seq.size()), false, gl);
            }
        } else {
            for (uint32_t k = 0; k < lb; ++k) dst[k] = line[j.off + t.at[k]];
            for (size_t k = 0; k < seq.size(); ++k) dst[lb + k] = seq[k];
        }
        for (int k = 0; k < align; ++k) if (buf[k] != 0xEE) { std::printf("a byte in front of the destination was written\n"); return 1; }
        std::cout << 0 << ' ' << j.off << ' ' << j.ulen << ' ' << std::hex << j.joiners << std::dec << ' ' << hex(dst, total) << '\n';
        std::free(raw);
    }
    return 0;
}

static int run_file()
{
    std::string sep_name, hl;
    long long bad = -1;
    uint32_t reason = 0, ulen0 = 0, lb = 0;
    uint64_t joiners0 = 0;
    for (long long i = 0; std::cin >> sep_name >> hl; ++i) {
        const uint8_t sep = sep_name == "c" ? ':' : '_';
        const Judged j = by_lanes(unhex(hl), sep, i != 0, ulen0, joiners0);
        if (i == 0 && !j.reason) { ulen0 = j.ulen; joiners0 = j.joiners; Table t; lb = bases_table(ulen0, joiners0, &t); }
        if (j.reason && bad < 0) { bad = i; reason = j.reason; }
    }
    std::cout << bad << ' ' << reason << ' ' << ulen0 << ' ' << std::hex << joiners0 << std::dec << ' ' << lb << '\n';
    return 0;
}

static int run_injective()
{
    static const char alphabet[] = "ACGTN+";
    static const char* seqs[] = {"", "A", "C", "AA", "AC", "CA", "CC"};
    unsigned long long checked = 0;
    std::map<std::pair<uint32_t, uint64_t>, std::set<std::string>> by_shape;
    for (uint32_t L = 1; L <= 5; ++L) {
        uint32_t count = 1;
        for (uint32_t i = 0; i < L; ++i) count *= 6;
        for (uint32_t code = 0; code < count; ++code) {
            std::vector<uint8_t> line{'@', ':'};
            for (uint32_t i = 0, c = code; i < L; ++i, c /= 6) line.push_back(uint8_t(alphabet[c % 6]));
            line.push_back('\n');
            const Judged j = by_rule(line, ':', false, 0, 0);
            if (j.reason == kNoBase) continue;
            if (j.reason || j.off != 2 || j.ulen != L) { std::printf("unexpected verdict: length %u code %u\n", L, code); return 1; }
            Table t;
            const uint32_t lb = bases_table(j.ulen, j.joiners, &t);
            if (lb != L - uint32_t(__builtin_popcountll(j.joiners))) { std::printf("Lb is not the shape's: length %u code %u\n", L, code); return 1; }
            std::string b;
            for (uint32_t k = 0; k < lb; ++k) b += char(line[j.off + t.at[k]]);
            if (!by_shape[{j.ulen, j.joiners}].insert(b).second) { std::printf("two U of one shape with one B: length %u code %u\n", L, code); return 1; }
            ++checked;
        }
    }
    for (const auto& kv : by_shape) {
        std::set<std::string> keys;
        for (const std::string& b : kv.second)
            for (const char* s : seqs) if (!keys.insert(b + s).second) { std::printf("two keys of one shape collide\n"); return 1; }
        if (keys.size() != kv.second.size() * 7) return 1;
    }
    std::printf("%llu %zu\n", checked, by_shape.size());
    return 0;
}

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "rule") return run_records(false);
    if (what == "lanes") return run_records(true);
    if (what == "file") return run_file();
    if (what == "injective") return run_injective();
    std::fprintf(stderr, "usage: umi_check rule|lanes|file|injective\n");
    return 2;
}
