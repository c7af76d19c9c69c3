"""The rules of FQD_SEQ_KEEP=best (fastq-dupaway_amd/csrc/fqd_seq_pick_core.hpp) on the CPU, in a harness built with the
sanitizers (tests/native/seq_pick_check.cpp), against plain Python (tests/seq_keep_reference.py): the byte rule and the
masked word arithmetic, the last line found from the record's end the way the scores kernel walks it, saturation, and
the combine of the segmented scan (associativity, the tie rule, the scan cut into three blocks at every pair of places).
The device code that runs the same functions: tests/test_gpu_seq_pick.py; the run: tests/test_seq_keep_cli.py."""
import random
import subprocess
from pathlib import Path

import pytest

import seq_keep_reference as keep

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "seq_pick_check.cpp"
EXE = HERE / "native" / "seq_pick_check"


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(EXE), str(SRC)], check=True, capture_output=True)
    return str(EXE)


def ask(harness, what, text):
    r = subprocess.run([harness, what], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def byte_score(b):
    return b - 33 if b >= 33 else 0


def test_word_score_every_byte_value_at_every_place(harness):
    rng = random.Random(1)
    words = [bytes([b if j == p else 0 for j in range(8)]) for b in range(256) for p in range(8)]
    words += [bytes([b] * 8) for b in range(256)]
    words += [bytes(rng.randrange(256) for _ in range(8)) for _ in range(2000)]
    words += [bytes(rng.choice([10, 13, 32, 33, 34, 126, 255]) for _ in range(8)) for _ in range(2000)]
    got = ask(harness, "word", "".join(f"{int.from_bytes(w, 'little'):x}\n" for w in words))
    assert len(got) == len(words)
    for w, (whole, behind, found) in zip(words, got):
        assert whole == sum(byte_score(b) for b in w)
        assert found == int(10 in w)
        assert behind == sum(byte_score(b) for b in w[w.rfind(b"\n") + 1:])


def records():
    rng = random.Random(2)
    out = [b"", b"\n", b"\n\n", b"@a\nACGT\n+\n\n", b"@a\nACGT\n+\nIIII\n", b"@a\r\nACGT\r\n+\r\nIIII\r\n", b"IIII", b"IIII\n", b"\nIIII",
           b"@a\nAC\n+a\n" + bytes(range(11, 256)) + b"\n", b"@a\nAC\n+\n" + bytes(range(0, 10)) + b"\n", b"\r\n", b"~" * 300 + b"\n"]
    for q in (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300):
        for idl in range(9):                                 # the last line ends at every place of a word
            qual = bytes(rng.choice([33, 34, 73, 126, 200, 255, 13, 32]) for _ in range(q))
            out.append(b"@" + b"x" * idl + b"\n" + b"ACGT"[:q % 5] + b"\n+\n" + qual + b"\n")
            out.append(qual + b"\n")                         # a record of one line: the search ends at the record's start
            out.append(qual)
    return out


def test_last_line_score_by_bytes_and_by_words(harness):
    recs = records()
    got = ask(harness, "score", "".join((r.hex() if r else "-") + "\n" for r in recs))
    assert len(got) == len(recs)
    for r, (by_bytes, by_words) in zip(recs, got):
        assert by_bytes == keep.score(r), r
        assert by_words == keep.score(r), r


def test_saturation(harness):
    top = 2 ** 32
    sums = [(0, 0), (top - 2, 1), (top - 1, 0), (top - 1, 1), (top, 0), (top + 5, 7), (top - 1, top - 1), (2 ** 64 - 1, 2 ** 64 - 1),
            (top // 2, top // 2 - 1), (top // 2, top // 2), (222 * 19_346_000, 222 * 1000), (12, 30)]
    got = ask(harness, "sat", "".join(f"{a} {b}\n" for a, b in sums))
    for (a, b), (sa, sab) in zip(sums, got):
        assert sa == min(a, keep.SAT)
        assert sab == min(min(a, keep.SAT) + min(b, keep.SAT), keep.SAT)


def scan_cases():
    rng = random.Random(3)
    yield [(5, 1)]
    yield [(5, 0)]                                           # place 0 starts a segment whatever its flag says
    yield [(7, 1), (7, 0), (7, 0)]                           # a tie: the earliest
    yield [(1, 1), (9, 0), (9, 0), (3, 1), (3, 0)]
    yield [(0, 1)] * 6
    yield [(keep.SAT, 1), (keep.SAT, 0), (keep.SAT - 1, 0), (keep.SAT, 1), (0, 0), (keep.SAT, 0)]
    for _ in range(40):
        n = rng.choice([2, 3, 8, 21, 40])
        yield [(rng.choice([0, 1, 2, 2, 3, keep.SAT, rng.randrange(2 ** 32)]), int(rng.random() < rng.choice([0.1, 0.5, 0.9]))) for _ in range(n)]


@pytest.mark.parametrize("case", list(range(46)))
def test_combine_cut_at_every_place(harness, case):
    rows = list(scan_cases())[case]
    got = ask(harness, "scan", f"{len(rows)}\n" + "".join(f"{s} {h}\n" for s, h in rows))   # exit 5: a cut changed the scan
    n = len(rows)
    head = [1 if k == 0 else h for k, (_, h) in enumerate(rows)]
    starts = [k for k in range(n) if head[k]]
    assert [g[0] for g in got] == starts
    order, _ = keep.pick(list(range(n)), head, [s for s, _ in rows])
    assert [g[1] for g in got] == [order[k] for k in starts]  # over the identity order the record at a head's place is the best one's place
