// CPU harness for csrc/fqd_consensus_core.hpp (tests/test_consensus_core.py builds it with -Werror and the sanitizers): the
// header's host compile, asked over stdin and answered a line a question.  argv[1] says what:
//   columns   no input; every column of 1 .. 4 members over the letters ACGTN and the quality bytes "!#5I~ ", member 0 the
//             written one, the first member's symbol changing slowest (tests/consensus_cases.py: small_columns); a line
//             "letter quality changed" each, from 32-bit states; a 64-bit state must give the same or the line says so
//   column    lines "hex(own) hex(bases) hex(quals)"; answers "letter quality changed"
//   splits    lines "hex(bases) hex(quals)" of up to 8 members: the members dealt to 2 and to 3 parts in every way, the parts'
//             states combined in every order and grouping, 32-bit parts into 32-bit and into 64-bit sums; every result must
//             be the state of the members added one by one.  Answers "ok <combines checked>" or says what failed.
//   fit       lines "start size seq_off seq_len"; answers lines_fit as 0 or 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../fastq-dupaway_amd/csrc/fqd_consensus_core.hpp"

using namespace fqdconsensus;

namespace {

std::vector<uint8_t> unhex(const std::string& s)
{
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t k = 0; k + 1 < s.size(); k += 2) out.push_back(uint8_t(std::stoul(s.substr(k, 2), nullptr, 16)));
    return out;
}

template <class Sum>
State<Sum> state_of(const uint8_t* bases, const uint8_t* quals, size_t m)
{
    State<Sum> st;
    clear(st);
    for (size_t i = 0; i < m; ++i) add(st, bases[i], quals[i]);
    return st;
}

template <class A, class B>
bool same(const State<A>& a, const State<B>& b)
{
    for (uint32_t x = 0; x < kLetters; ++x) if (uint64_t(a.s[x]) != uint64_t(b.s[x])) return false;
    return a.mask == b.mask;
}

void print(const Verdict& v) { std::printf("%c %u %d\n", byte_of(v.letter), unsigned(v.quality), int(v.changed)); }

int columns()
{
    const char letters[] = "ACGTN", quals[] = "!#5I~ ";
    uint8_t b[4], q[4];
    for (uint32_t m = 1; m <= 4; ++m) {
        uint32_t count = 1;
        for (uint32_t k = 0; k < m; ++k) count *= 30;
        for (uint32_t v = 0; v < count; ++v) {
            uint32_t x = v;
            for (uint32_t k = m; k-- > 0; x /= 30) { b[k] = uint8_t(letters[x % 30 / 6]); q[k] = uint8_t(quals[x % 30 % 6]); }
            const Verdict a = decide(state_of<uint32_t>(b, q, m), b[0]), c = decide(state_of<uint64_t>(b, q, m), b[0]);
            if (a.letter != c.letter || a.quality != c.quality || a.changed != c.changed) { std::printf("the 64-bit state decides otherwise at %u of %u members\n", v, m); return 1; }
            print(a);
        }
    }
    return 0;
}

// Every way to deal m members to `parts` parts (empty parts among them), every order and grouping of the combine.
unsigned long long splits_of(const std::vector<uint8_t>& bases, const std::vector<uint8_t>& quals, uint32_t parts, bool* ok)
{
    const size_t m = bases.size();
    const State32 whole = state_of<uint32_t>(bases.data(), quals.data(), m);
    uint64_t ways = 1;
    for (size_t i = 0; i < m; ++i) ways *= parts;
    unsigned long long checked = 0;
    for (uint64_t w = 0; w < ways; ++w) {
        State32 part[3];
        for (uint32_t p = 0; p < 3; ++p) clear(part[p]);
        uint64_t x = w;
        for (size_t i = 0; i < m; ++i, x /= parts) add(part[x % parts], bases[i], quals[i]);
        uint32_t order[3] = {0, 1, 2};
        std::sort(order, order + parts);
        do {
            // left to right, into 32 bits and into 64 bits (an atomic add to memory is a combine with one part)
            State32 a;
            State64 wide;
            clear(a); clear(wide);
            for (uint32_t k = 0; k < parts; ++k) { combine(a, part[order[k]]); combine(wide, part[order[k]]); }
            // the last two first
            State32 tail = part[order[parts - 1]], b = part[order[0]];
            if (parts == 3) { State32 t = part[order[1]]; combine(t, tail); tail = t; }
            combine(b, tail);
            checked += 3;
            if (!same(a, whole) || !same(wide, whole) || !same(b, whole)) { *ok = false; return checked; }
        } while (std::next_permutation(order, order + parts));
    }
    return checked;
}

} // namespace

int main(int argc, char** argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "columns") return columns();
    std::string line;
    unsigned long long checked = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (what == "column") {
            std::string own, bases, quals;
            in >> own >> bases >> quals;
            const std::vector<uint8_t> o = unhex(own), b = unhex(bases), q = unhex(quals);
            print(decide(state_of<uint32_t>(b.data(), q.data(), b.size()), o.at(0)));
        } else if (what == "splits") {
            std::string bases, quals;
            in >> bases >> quals;
            const std::vector<uint8_t> b = unhex(bases), q = unhex(quals);
            if (b.size() != q.size() || b.size() > 8) { std::printf("bad line\n"); return 1; }
            bool ok = true;
            checked += splits_of(b, q, 2, &ok);
            if (ok) checked += splits_of(b, q, 3, &ok);
            if (!ok) { std::printf("a split of %s %s gives another state\n", bases.c_str(), quals.c_str()); return 1; }
        } else if (what == "fit") {
            unsigned long long start, size, seq_off, seq_len;
            in >> start >> size >> seq_off >> seq_len;
            std::printf("%d\n", int(lines_fit(start, uint32_t(size), seq_off, uint32_t(seq_len))));
        } else {
            std::printf("unknown question\n");
            return 2;
        }
    }
    if (what == "splits") std::printf("ok %llu\n", checked);
    return 0;
}
