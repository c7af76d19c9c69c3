// seq_pick_check.cpp — the rules of FQD_SEQ_KEEP=best (fastq-dupaway_amd/csrc/fqd_seq_pick_core.hpp) on the CPU, the way
// the device runs them.  tests/test_seq_pick_core.py builds this with the sanitizers and holds it against plain Python.
//   seq_pick_check score < one record per line as hex ("-" = empty)  > "byte-rule by-words" per line: the rule byte by
//                          byte, and the walk of the scores kernel (eight lanes, 8 bytes each, from the end backwards)
//   seq_pick_check word  < one 64-bit word per line as hex           > "word_score after_newline found"
//   seq_pick_check sat   < "a b" per line (decimal, up to 2^64-1)    > "saturate_score(a) add_scores(sat a, sat b)"
//   seq_pick_check scan  < "n" then n lines "score head"             > per segment "start best", after the scan cut into
//                          three blocks at every pair of places gave what the scan in one piece gives (exit 5 if not)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_seq_pick_core.hpp"

using fqdseq::Pick;

static std::vector<uint8_t> from_hex(const char* line)
{
    std::vector<uint8_t> out;
    const size_t len = std::strcspn(line, "\r\n");
    if (len == 1 && line[0] == '-') return out;
    for (size_t k = 0; k + 1 < len; k += 2) { unsigned v = 0; std::sscanf(line + k, "%2x", &v); out.push_back(uint8_t(v)); }
    return out;
}

// What word_at of the kernel gives: eight bytes at rec + a, '\n' below the record's start.  Never reads outside rec.
static uint64_t word_at(const std::vector<uint8_t>& rec, int64_t a)
{
    uint64_t x = 0;
    for (int j = 0; j < 8; ++j) x |= uint64_t(a + j >= 0 ? rec.at(size_t(a + j)) : uint8_t('\n')) << (8 * j);
    return x;
}

static uint32_t score_by_words(const std::vector<uint8_t>& rec)
{
    int64_t pos = int64_t(rec.size());
    if (pos == 0) return 0;
    if (rec[size_t(pos - 1)] == '\n') --pos;
    uint64_t sum = 0;
    for (;;) {
        uint32_t whole[8], behind[8];
        int first = -1;
        for (int sub = 0; sub < 8; ++sub) {
            const uint64_t x = word_at(rec, pos - 8 * int64_t(sub + 1));
            bool has = false;
            whole[sub] = fqdseq::word_score(x);
            behind[sub] = fqdseq::word_score_after_newline(x, &has);
            if (has && first < 0) first = sub;
        }
        if (first < 0) { for (int sub = 0; sub < 8; ++sub) sum += whole[sub]; pos -= 64; continue; }
        for (int sub = 0; sub < first; ++sub) sum += whole[sub];
        sum += behind[first];
        return fqdseq::saturate_score(sum);
    }
}

static int score()
{
    static char line[1 << 16];
    while (std::fgets(line, sizeof line, stdin)) {
        const std::vector<uint8_t> rec = from_hex(line);   // a heap copy of exactly the record: a read outside is the sanitizer's
        std::printf("%u %u\n", fqdseq::last_line_score(rec.data(), rec.size()), score_by_words(rec));
    }
    return 0;
}

static int word()
{
    unsigned long long x;
    while (std::scanf("%llx", &x) == 1) {
        bool has = false;
        const uint32_t behind = fqdseq::word_score_after_newline(x, &has);
        std::printf("%u %u %d\n", fqdseq::word_score(x), behind, has ? 1 : 0);
    }
    return 0;
}

static int sat()
{
    unsigned long long a, b;
    while (std::scanf("%llu %llu", &a, &b) == 2)
        std::printf("%u %u\n", fqdseq::saturate_score(a), fqdseq::add_scores(fqdseq::saturate_score(a), fqdseq::saturate_score(b)));
    return 0;
}

static bool same(Pick a, Pick b) { return a.best == b.best && a.start == b.start; }

static int scan()
{
    unsigned long long n = 0;
    if (std::scanf("%llu", &n) != 1) return 2;
    std::vector<Pick> el(n);
    std::vector<int> head(n);
    for (uint64_t k = 0; k < n; ++k) {
        unsigned long long s; int h;
        if (std::scanf("%llu %d", &s, &h) != 2) return 2;
        head[k] = h;
        el[k] = fqdseq::pick_of(uint32_t(s), uint32_t(k), k == 0 || h != 0);
    }
    std::vector<Pick> whole(n);
    Pick cur = fqdseq::pick_identity();
    for (uint64_t k = 0; k < n; ++k) { cur = fqdseq::combine(cur, el[k]); whole[k] = cur; }
    auto fold = [&](uint64_t lo, uint64_t hi) { Pick a = fqdseq::pick_identity(); for (uint64_t k = lo; k < hi; ++k) a = fqdseq::combine(a, el[k]); return a; };
    for (uint64_t i = 0; i <= n; ++i)
        for (uint64_t j = i; j <= n; ++j) {
            const Pick a = fold(0, i), b = fold(i, j), c = fold(j, n);
            if (!same(fqdseq::combine(fqdseq::combine(a, b), c), fqdseq::combine(a, fqdseq::combine(b, c)))) return 5;
            if (n && !same(fqdseq::combine(fqdseq::combine(a, b), c), whole[n - 1])) return 5;
            const Pick before[3] = {fqdseq::pick_identity(), a, fqdseq::combine(a, b)};
            const uint64_t lo[3] = {0, i, j}, hi[3] = {i, j, n};
            for (int blk = 0; blk < 3; ++blk) {
                Pick run = before[blk];
                for (uint64_t k = lo[blk]; k < hi[blk]; ++k) { run = fqdseq::combine(run, el[k]); if (!same(run, whole[k])) return 5; }
            }
        }
    for (uint64_t k = 0; k < n; ++k)
        if (k + 1 == n || head[k + 1]) std::printf("%u %u\n", whole[k].start, fqdseq::picked_place(whole[k].best));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "score") == 0) return score();
    if (argc == 2 && std::strcmp(argv[1], "word") == 0) return word();
    if (argc == 2 && std::strcmp(argv[1], "sat") == 0) return sat();
    if (argc == 2 && std::strcmp(argv[1], "scan") == 0) return scan();
    return 2;
}
