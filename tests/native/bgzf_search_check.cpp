// Both modes of the device BGZF coder (fastq-dupaway_amd/csrc/fqd_bgzf_core.hpp, fqd_bgzf_search_core.hpp) run
// thread by thread on the CPU, phase by phase as the kernels of fqd_bgzf.hip and fqd_bgzf_search.hip run them
// between barriers: input file -> BGZF file.  Test infrastructure only (tests/test_bgzf_search_core.py inflates
// the result with Python's gzip; tests/test_gpu_bgzf_search.py holds the kernels to the same bytes).
//   bgzf_search_check <in> <out.gz> <lines_per_record> <effort>     prints: members stored_members bytes_out
// effort 0 = the fast mode (what bgzf_core_check writes), 1 = the search mode.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_bgzf_search_core.hpp"

using namespace fqd::bgzf;

struct HostOr { void operator()(uint32_t* p, uint32_t v) const { *p |= v; } };

struct Lines {
    std::vector<uint16_t> ls = std::vector<uint16_t>(kMaxLines + 2);
    uint32_t line_at[kThreads];
    uint32_t n_lines = 0;
    bool on;
};

static void index_lines(const uint8_t* data, uint32_t L, Lines& x)
{
    uint32_t total = 0;
    for (uint32_t t = 0; t < kThreads; ++t) {
        uint32_t lo, hi; chunk_of(t, L, lo, hi);
        x.line_at[t] = total;
        const Scan sc = scan_chunk(Linear{data}, lo, hi);
        total += uint32_t(__builtin_popcountll(sc.nl.lo) + __builtin_popcountll(sc.nl.hi));
    }
    x.n_lines = total;
    x.on = total <= kMaxLines;
    x.ls[0] = 0;
    if (!x.on) return;
    for (uint32_t t = 0; t < kThreads; ++t) {
        uint32_t lo, hi; chunk_of(t, L, lo, hi);
        const Scan sc = scan_chunk(Linear{data}, lo, hi);
        uint32_t k = x.line_at[t] + 1;
        for (uint64_t m = sc.nl.lo; m; m &= m - 1) x.ls[k++] = uint16_t(lo + uint32_t(__builtin_ctzll(m)) + 1);
        for (uint64_t m = sc.nl.hi; m; m &= m - 1) x.ls[k++] = uint16_t(lo + 64 + uint32_t(__builtin_ctzll(m)) + 1);
    }
}

struct HostMax { uint32_t operator()(uint32_t* p, uint32_t v) const { const uint32_t old = *p; if (v > old) *p = v; return old; } };

// The search of one member, round by round: every thread looks its position up, a barrier, inserts it, a barrier, looks it up again.
static void search_member(const uint8_t* data, uint32_t L, std::vector<uint32_t>& table, std::vector<uint32_t>& found)
{
    std::fill(table.begin(), table.end(), 0u);
    for (uint32_t r = 0; r * kThreads < L; ++r) {
        const uint32_t base = r * kThreads;
        for (uint32_t t = 0; t < kThreads; ++t) if (base + t < L) found[base + t] = search_lookup(Linear{data}, table.data(), base + t, L, 0u, 0u);
        for (uint32_t t = 0; t < kThreads; ++t) if (base + t < L) search_insert(Linear{data}, table.data(), base + t, L, HostMax{});
        for (uint32_t t = 0; t < kThreads; ++t) if (base + t < L) found[base + t] = search_lookup(Linear{data}, table.data(), base + t, L, base, found[base + t]);
    }
}

struct Counter {
    uint64_t* hist;
    void literal(uint32_t b) { ++hist[b]; }
    void match(uint32_t len, uint32_t dist) { ++hist[length_symbol(len).sym]; ++hist[kLitLen + dist_symbol(dist).sym]; }
};

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> in((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const uint32_t K = uint32_t(std::atoi(argv[3]));
    const uint32_t effort = uint32_t(std::atoi(argv[4]));
    if (effort > kEffortSearch) return 2;
    std::vector<uint32_t> table(kBuckets * kWays), found(kMember);
    const uint64_t n = in.size(), members = (n + kMember - 1) / kMember;
    in.resize(n + 64);
    std::vector<uint64_t> hist(kLitLen + kDist, 0);
    Lines x;
    static Codes codes;
    // the search mode is counted as the fast mode parses (pass 0), then kSearchCounts times its own parse under the codes before
    for (uint32_t pass = effort ? 0u : 1u; pass < 1u + kSearchCounts; ++pass) {
        const bool searching = effort && pass >= 1u;
        std::fill(hist.begin(), hist.end(), 0);
        for (uint64_t m = 0; m < members; m += sample_every(members)) {
            const uint8_t* data = in.data() + m * kMember;
            const uint32_t L = uint32_t(std::min<uint64_t>(kMember, n - m * kMember));
            index_lines(data, L, x);
            if (searching) search_member(data, L, table, found);
            for (uint32_t t = 0; t < kThreads; ++t) {
                uint32_t lo, hi; chunk_of(t, L, lo, hi);
                Counter c{hist.data()};
                const Scan sc = scan_chunk(Linear{data}, lo, hi);
                const Columns col = column_masks(Linear{data}, lo, hi, x.ls.data(), x.line_at[t], x.n_lines, L, x.on, K);
                if (searching) parse_chunk_search(Linear{data}, lo, hi, sc, col, found.data() + lo, WorthCodes{codes.lit, codes.dist}, c);
                else parse_chunk(Linear{data}, lo, hi, sc, col, c);
            }
        }
        build_codes(hist.data(), members, codes, effort != kEffortFast);
    }
    std::FILE* out = std::fopen(argv[2], "wb");
    uint64_t bytes_out = 0, stored_members = 0;
    std::vector<uint32_t> slot(kSlot / 4);
    for (uint64_t m = 0; m < members; ++m) {
        const uint8_t* data = in.data() + m * kMember;
        const uint32_t L = uint32_t(std::min<uint64_t>(kMember, n - m * kMember));
        std::fill(slot.begin(), slot.end(), 0u);
        index_lines(data, L, x);
        if (effort) search_member(data, L, table, found);
        uint32_t bits[kThreads], before[kThreads], body = 0;
        for (uint32_t t = 0; t < kThreads; ++t) {
            uint32_t lo, hi; chunk_of(t, L, lo, hi);
            BitCounter price{codes.lit, codes.dist};
            const Scan sc = scan_chunk(Linear{data}, lo, hi);
            const Columns col = column_masks(Linear{data}, lo, hi, x.ls.data(), x.line_at[t], x.n_lines, L, x.on, K);
            if (effort) parse_chunk_search(Linear{data}, lo, hi, sc, col, found.data() + lo, WorthCodes{codes.lit, codes.dist}, price);
            else parse_chunk(Linear{data}, lo, hi, sc, col, price);
            bits[t] = price.bits; before[t] = body; body += bits[t];
        }
        const uint32_t total_bits = codes.header_bits + body + (codes.lit[256] >> 16);
        uint32_t clen = (total_bits + 7) / 8;
        const bool stored = clen >= L + 5;
        if (stored) { clen = L + 5; ++stored_members; }
        HostOr orw;
        uint32_t crc[kThreads];
        for (uint32_t t = 0; t < kThreads; ++t) {
            uint32_t lo, hi; chunk_of(t, L, lo, hi);
            if (!stored) {
                BitWriter<HostOr> w(slot.data(), kHeadBytes * 8 + (t == 0 ? 0 : codes.header_bits + before[t]), orw);
                if (t == 0)
                    for (uint32_t at = 0; at < codes.header_bits; at += 32)
                        w.put(codes.header_bits - at >= 32 ? codes.header[at >> 5] : codes.header[at >> 5] & ((1u << (codes.header_bits - at)) - 1u),
                              codes.header_bits - at >= 32 ? 32 : codes.header_bits - at);
                Emitter<HostOr> emit{codes.lit, codes.dist, w};
                const Scan sc = scan_chunk(Linear{data}, lo, hi);
                const Columns col = column_masks(Linear{data}, lo, hi, x.ls.data(), x.line_at[t], x.n_lines, L, x.on, K);
                if (effort) parse_chunk_search(Linear{data}, lo, hi, sc, col, found.data() + lo, WorthCodes{codes.lit, codes.dist}, emit);
                else parse_chunk(Linear{data}, lo, hi, sc, col, emit);
                if (t == kThreads - 1) w.put(codes.lit[256] & 0xFFFFu, codes.lit[256] >> 16);
                w.finish();
            } else {
                if (t == 0) { BitWriter<HostOr> w(slot.data(), kHeadBytes * 8, orw); w.put(1, 8); w.put(L, 16); w.put(~L & 0xFFFFu, 16); w.finish(); }
                BitWriter<HostOr> w(slot.data(), (kHeadBytes + 5 + lo) * 8, orw);
                for (uint32_t p = lo; p < hi; ++p) w.put(data[p], 8);
                w.finish();
            }
            crc[t] = crc_chunk(codes.crc_table, Linear{data}, lo, hi);
        }
        for (uint32_t k = 0; k < kLevels; ++k)
            for (uint32_t t = 0; t < kThreads; t += 2u << k) crc[t] = crc_advance(codes.crc_shift[k], crc[t]) ^ crc[t + (1u << k)];
        const uint32_t total = kHeadBytes + clen + kTailBytes;
        BitWriter<HostOr> h(slot.data(), 0, orw);
        h.put(31u | (139u << 8) | (8u << 16) | (4u << 24), 32); h.put(0, 32); h.put(0u | (255u << 8) | (6u << 16), 32);
        h.put(uint32_t('B') | (uint32_t('C') << 8) | (2u << 16), 32); h.put(total - 1, 16); h.finish();
        BitWriter<HostOr> tl(slot.data(), (kHeadBytes + clen) * 8, orw);
        tl.put(crc[0] ^ 0xFFFFFFFFu, 32); tl.put(L, 32); tl.finish();
        std::fwrite(slot.data(), 1, total, out);
        bytes_out += total;
    }
    static const unsigned char eof[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::fwrite(eof, 1, sizeof eof, out);
    std::fclose(out);
    std::printf("%llu %llu %llu\n", (unsigned long long)members, (unsigned long long)stored_members, (unsigned long long)(bytes_out + sizeof eof));
    return 0;
}
