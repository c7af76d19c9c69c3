"""CPU checks of the sequence-based modes: the plain-Python restatement (tests/seq_reference.py) reproduces the
reference's own fixtures byte for byte, and the head rules of csrc/fqd_seq_core.hpp — the ones the device runs in
parallel — agree with the reference's sequential scan on thousands of random and adversarial sorted lists (a native
harness built with ASan/UBSan into the test's temporary directory)."""
import shutil
import subprocess
from pathlib import Path

import pytest

import seq_reference as ref

FIX = Path(__file__).resolve().parent / "golden" / "reference_seq_fixtures"
CORE = Path(__file__).resolve().parent.parent / "fastq-dupaway_amd" / "csrc" / "fqd_seq_core.hpp"


@pytest.mark.parametrize("name,mode,distance", [
    ("single_tight.fa", "tight", 2), ("single_loose.fa", "loose", 2), ("single_hamming.fa", "tail-hamming", 1)])
def test_restatement_reproduces_single_fixtures(name, mode, distance):
    outs, _, _, _ = ref.dedup([(FIX / "inputs" / name).read_bytes()], fasta=True, mode=ref.MODES[mode], distance=distance)
    assert outs[0] == (FIX / "expected" / name).read_bytes()


def test_restatement_reproduces_paired_fixture():
    ins = [(FIX / "inputs" / f"paired_tight_r{k}.fa").read_bytes() for k in (1, 2)]
    outs, _, _, _ = ref.dedup(ins, fasta=True, mode=ref.TIGHT)
    for k, out in zip((1, 2), outs):
        assert out == (FIX / "expected" / f"paired_tight_r{k}.fa").read_bytes()


def test_restatement_loose_empty_read_matches_everything():
    data = b">a\n\n>b\nACGT\n>c\nAC\n"
    outs, clusters, total, dups = ref.dedup([data], fasta=True, mode=ref.LOOSE)
    assert outs[0] == b">a\n\n" and (total, dups) == (3, 2)
    assert clusters[0] == b">a\n-->c\n-->b\n"


HARNESS = r"""
#include "fqd_seq_core.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>
using fqdseq::View;
struct Rec { std::string a, b; };
static View v(const std::string& s) { return View{reinterpret_cast<const uint8_t*>(s.data()), uint32_t(s.size())}; }
static bool less(const Rec& x, const Rec& y) {
    const std::string xa = x.a + '\n', ya = y.a + '\n';
    if (xa != ya) return xa < ya;
    return x.b + '\n' < y.b + '\n';
}
static std::string rnd(std::mt19937_64& g, int len, const char* alpha) {
    std::string s; const int k = int(std::string(alpha).size());
    for (int i = 0; i < len; ++i) s += alpha[g() % k];
    return s;
}
int main() {
    std::mt19937_64 g(12345);
    long checked = 0;
    for (int trial = 0; trial < 4000; ++trial) {
        const int style = trial % 5, n = 1 + int(g() % 200);
        const bool paired = trial % 2;
        const uint32_t d = uint32_t(g() % 4);
        std::vector<Rec> r;
        std::string base = rnd(g, 1 + int(g() % 40), "ACGT");
        for (int i = 0; i < n; ++i) {
            Rec x;
            if (style == 0) { x.a = rnd(g, int(g() % 12), "ACGTNacgt"); x.b = rnd(g, int(g() % 12), "ACGT"); }
            else if (style == 1) { x.a = base.substr(0, g() % (base.size() + 1)); x.b = base.substr(0, g() % (base.size() + 1)); }  // prefix chains, empty reads
            else if (style == 2) { x.a = base; for (int k = 0; k < 2; ++k) if (g() % 2) x.a[g() % x.a.size()] = "ACGT"[g() % 4]; x.b = base; if (g() % 4 == 0) x.b[g() % x.b.size()] = 'N'; }  // hamming chains
            else if (style == 3) { const size_t c1 = g() % (base.size() + 1), c2 = g() % (base.size() + 1); x.a = base.substr(0, c1); x.b = base.substr(0, (g() % 2) ? c2 : base.size() - c1); }  // opposite-sided overlaps
            else { x.a = rnd(g, int(g() % 3), "AC"); x.b = rnd(g, int(g() % 3), "AC"); }
            if (!paired) x.b.clear();
            r.push_back(x);
        }
        std::stable_sort(r.begin(), r.end(), less);
        auto at = [&](uint64_t k, View& a, View& b) { a = v(r[k].a); b = v(r[k].b); };
        for (int mode = 0; mode < 3; ++mode) {
            std::vector<uint8_t> seq(n), par(n, 0), cut(n);
            fqdseq::sequential_heads(mode, d, paired, n, at, seq.data());
            if (mode != fqdseq::kHamming) {
                for (int k = 0; k < n; ++k) par[k] = k == 0 || !fqdseq::matches(mode, d, paired, v(r[k-1].a), v(r[k-1].b), v(r[k].a), v(r[k].b));
            } else {
                for (int k = 0; k < n; ++k) cut[k] = k == 0 || fqdseq::hamming_certain_head(d, paired, v(r[k-1].a), v(r[k-1].b), v(r[k].a), v(r[k].b));
                for (int s = 0; s < n;) {                      // each segment scanned on its own from its first record
                    int e = s + 1; while (e < n && !cut[e]) ++e;
                    auto at_seg = [&](uint64_t k, View& a, View& b) { at(s + k, a, b); };
                    fqdseq::sequential_heads(mode, d, paired, uint64_t(e - s), at_seg, par.data() + s);
                    s = e;
                }
                for (int k = 0; k < n; ++k) if (cut[k] && !seq[k]) { std::printf("cut %d is no head (trial %d)\n", k, trial); return 1; }
            }
            for (int k = 0; k < n; ++k)
                if (seq[k] != par[k]) { std::printf("mode %d trial %d: record %d sequential %d parallel %d\n", mode, trial, k, seq[k], par[k]); return 1; }
            checked += n;
        }
    }
    std::printf("ok %ld\n", checked);
    return 0;
}
"""


def test_native_head_rules_match_sequential_scan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "seq_core_check.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "seq_core_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(CORE.parent), "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")
