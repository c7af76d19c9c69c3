"""The rule of FQD_FAST_STRAND=both (fastq-dupaway_amd/csrc/fqd_strand_core.hpp) on the CPU, in a harness built with the
sanitizers (tests/native/strand_check.cpp): the header's host compile against the plain-Python statement
(tests/strand_reference.py) on the edge list of tests/strand_cases.py, the half-read lemma for every ACGTN string up to
length 7, the sixteen-byte helpers the kernel is made of, and (`lanes`) the very functions the kernel's sixteen lanes a
record run, played lane after lane into buffers of the exact size.  The device code: tests/test_gpu_strand.py; the run:
tests/test_fast_strand_cli.py."""
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

import strand_reference as ref
from strand_cases import paired_cases, random_read, single_end_cases

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "strand_check.cpp"
EXE = HERE / "native" / "strand_check"


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(EXE), str(SRC)], check=True, capture_output=True)
    return str(EXE)


def ask(harness, what, text=""):
    r = subprocess.run([harness, what], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    return r.stdout.splitlines()


def hexed(b):
    return b.hex() if b else "-"


def more_single_end_reads():
    """Every length up to 70 and round the 256-byte round of sixteen chunks: random reads, reads that are their own reverse
    complement (with and without an N at the centre), and those with one byte changed somewhere."""
    rng = random.Random(31)
    out = []
    for L in list(range(70)) + [511, 512, 513, 514, 1023, 1024, 1025, 2000]:
        for _ in range(4):
            out.append((f"random {L}", random_read(rng, L, "ACGT")))
            h = random_read(rng, L // 2, "AC")
            out += [(f"own rc {2 * (L // 2)}", h + ref.rc(h)), (f"own rc {2 * (L // 2) + 1}", h + b"N" + ref.rc(h))]
            t = bytearray(h + ref.rc(h))
            if len(t) > 2:
                t[rng.randrange(len(t))] = ord("G")
                out.append((f"own rc with one byte changed {len(t)}", bytes(t)))
    return out


def more_pairs():
    """Mates of lengths round 16 and 256 that agree up to a random place (the whole shorter mate included)."""
    rng = random.Random(32)
    lengths = [0, 1, 15, 16, 17, 31, 32, 33, 150, 255, 256, 257, 300, 600]
    out = []
    for _ in range(1500):
        la, lb = rng.choice(lengths), rng.choice(lengths)
        a, b = random_read(rng, la, "AC"), bytearray(random_read(rng, lb, "AC"))
        k = rng.randrange(min(la, lb) + 1)
        b[:k] = a[:k]
        out.append((f"lengths {la} and {lb}, equal up to {k}", a, bytes(b)))
    return out


@pytest.mark.parametrize("what", ["canon", "lanes"])
def test_single_end_edge_list(harness, what):
    cases = single_end_cases() + more_single_end_reads()
    got = ask(harness, what, "".join(f"se {hexed(s)}\n" for _, s in cases))
    assert len(got) == len(cases)
    for (name, s), line in zip(cases, got):
        c, f = ref.canon_se(s)
        assert line == f"{hexed(c)} {int(f)}", name
    assert {f for _, s in cases for f in [ref.canon_se(s)[1]]} == {True, False}


@pytest.mark.parametrize("what", ["canon", "lanes"])
def test_paired_edge_list(harness, what):
    cases = paired_cases() + more_pairs()
    got = ask(harness, what, "".join(f"pe {hexed(a)} {hexed(b)}\n" for _, a, b in cases))
    assert len(got) == len(cases)
    for (name, a, b), line in zip(cases, got):
        (x, y), f = ref.canon_pe(a, b)
        assert line == f"{hexed(x)} {hexed(y)} {int(f)}", name


def test_bytes_outside_the_alphabet_pass_through_at_their_mirrored_place(harness):
    s = bytes([0, 255, ord("a"), ord("U"), ord("\n"), ord("T"), ord("R")])
    (line,) = ask(harness, "canon", f"se {hexed(s)}\n")
    c, f = ref.canon_se(s)
    assert line == f"{hexed(c)} {int(f)}"
    assert sorted(ref.rc(s).translate(ref.COMP)) == sorted(s)       # nothing but A/C/G/T changes


def test_half_read_lemma_exhaustively(harness):
    (line,) = ask(harness, "lemma")
    assert int(line) == sum(5 ** L for L in range(8))


def test_sixteen_byte_helpers(harness):
    (line,) = ask(harness, "chunks")
    assert int(line) == 200000


def test_canonical_form_is_a_function_of_the_set():
    # of the statement itself, so that the other tests lean on something checked
    for _, s in single_end_cases():
        assert ref.canon_se(s)[0] == ref.canon_se(ref.rc(s))[0]
        assert ref.rc(ref.rc(s)) == s
    for _, a, b in paired_cases():
        assert ref.canon_pe(a, b)[0] == ref.canon_pe(b, a)[0]


def test_numpy_forms_agree_with_the_plain_ones():
    rng = np.random.default_rng(3)
    a = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=(500, 9))
    b = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=(500, 9))
    b[100:150] = a[100:150]                                      # (equal mates among the pairs)
    rows, f = ref.canon_se_rows(a)
    for i in range(len(a)):
        c, flip = ref.canon_se(a[i].tobytes())
        assert rows[i].tobytes() == c and bool(f[i]) == flip
    (x, y), f = ref.canon_pe_rows(a, b)
    for i in range(len(a)):
        (cx, cy), flip = ref.canon_pe(a[i].tobytes(), b[i].tobytes())
        assert (x[i].tobytes(), y[i].tobytes(), bool(f[i])) == (cx, cy, flip)
    recs = [r.tobytes() for r in np.concatenate([a[:200], ref.rc_rows(a[:100]), a[50:120]])]
    rows, _ = ref.canon_se_rows(np.frombuffer(b"".join(recs), np.uint8).reshape(-1, 9))
    assert np.array_equal(ref.first_occurrence_rows(rows), ref.expected_keep(recs))
