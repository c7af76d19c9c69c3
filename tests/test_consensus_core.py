"""The rule of FQD_FAST_CONSENSUS (fastq-dupaway_amd/csrc/fqd_consensus_core.hpp) on the CPU, in a stand-alone harness built with
the sanitizers (tests/native/consensus_check.cpp): the header's host compile — a column's winner, quality and changed flag by
exhaustion over small columns, every kind of tie, both clamps, the combine over every split of a column's members, and the
record geometry that the call refuses — against the sequential statement (tests/consensus_reference.py).  The device code:
tests/test_gpu_consensus.py; the run: tests/test_fast_consensus_cli.py."""
import random
import subprocess
from pathlib import Path

import pytest

import consensus_reference as ref
from consensus_cases import LETTERS, QUALS, named_columns, small_columns

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "consensus_check.cpp"
EXE = HERE / "native" / "consensus_check"


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(EXE), str(SRC)], check=True, capture_output=True)
    return str(EXE)


def ask(harness, what, text=""):
    r = subprocess.run([harness, what], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


def said(win, quality, changed):
    return f"{chr(LETTERS[win])} {quality} {int(changed)}"


def test_every_small_column(harness):
    # 30 + 30^2 + 30^3 + 30^4 columns: up to 4 members, 5 letters, 5 quality bytes and one below 33; member 0 is the written one
    got = ask(harness, "columns")
    assert len(got) == 30 + 30 ** 2 + 30 ** 3 + 30 ** 4
    k = 0
    for bases, quals in small_columns():
        want = said(*ref.column(bases, quals, bases[0]))
        assert got[k] == want, (k, bases, quals, got[k], want)
        k += 1
    assert k == len(got)


def test_what_the_small_columns_hold():
    # the exhaustion reaches every tie, N as a winner, a changed letter, and both clamps
    seen = {"tie kept by the own letter": 0, "tie taken by the order": 0, "N wins": 0, "changed": 0, "clamped at 0": 0, "clamped at 93": 0}
    for bases, quals in small_columns(3):
        S = [0] * 5
        for b, q in zip(bases, quals):
            S[ref.letter(b)] += ref.weight(b, q)
        present = {ref.letter(b) for b in bases}
        top = max(S[x] for x in present)
        tied = [x for x in present if S[x] == top]
        win, q, changed = ref.column(bases, quals, bases[0])
        seen["tie kept by the own letter"] += len(tied) > 1 and not changed
        seen["tie taken by the order"] += len(tied) > 1 and changed and win == min(tied)
        seen["N wins"] += win == ref.N
        seen["changed"] += changed
        seen["clamped at 0"] += 2 * S[win] - sum(S) < 0
        seen["clamped at 93"] += 2 * S[win] - sum(S) > 93
        assert 33 <= q <= 126 and win in present
        assert win != ref.N or all(S[x] == 0 for x in present)     # N wins only where nothing else has weight
    assert all(seen.values()), seen


def test_ties_and_clamps_by_name(harness):
    cases = named_columns()
    for name, own, bases, quals, want in cases:                  # the statement first, so that a wrong expectation is not the harness's fault
        win, q, changed = ref.column(bases, quals, own[0])
        assert (bytes([LETTERS[win]]), bytes([q]), changed) == want, name
    got = ask(harness, "column", "".join(f"{own.hex()} {bases.hex()} {quals.hex()}\n" for _, own, bases, quals, _ in cases))
    assert got == [f"{want[0].decode()} {want[1][0]} {int(want[2])}" for *_, want in cases]


def test_any_bytes(harness):
    # every byte value as a base and as a quality byte; the own byte any byte as well
    rng = random.Random(11)
    cases = []
    for _ in range(4000):
        m = rng.randrange(1, 12)
        bases = bytes(rng.choice([rng.randrange(256), rng.choice(b"ACGTN")]) for _ in range(m))
        quals = bytes(rng.randrange(256) for _ in range(m))
        cases.append((bases[rng.randrange(m)], bases, quals))
    got = ask(harness, "column", "".join(f"{own:02x} {bases.hex()} {quals.hex()}\n" for own, bases, quals in cases))
    assert got == [said(*ref.column(bases, quals, own)) for own, bases, quals in cases]


def test_every_split_gives_the_unsplit_state(harness):
    # up to 8 members into 2 and into 3 parts in every way, combined in every order and grouping, into 32 and into 64 bits
    rng = random.Random(12)
    cases = [(b"", b""), (b"A", b"~"), (b"ACGTNACG", b"~~~~~~~~"), (b"NNNNNNNN", b"!#5I~ !#"), (b"AAAAAAAA", b"\xff" * 8)]
    for m in range(2, 9):
        for _ in range(3):
            cases.append((bytes(rng.choice(LETTERS) for _ in range(m)), bytes(rng.choice(QUALS) for _ in range(m))))
    got = ask(harness, "splits", "".join(f"{b.hex() or '-'} {q.hex() or '-'}\n" for b, q in cases))
    assert len(got) == 1 and got[0].startswith("ok "), got
    assert int(got[0].split()[1]) == 3 * sum(2 * 2 ** len(b) + 6 * 3 ** len(b) for b, _ in cases)


def test_lines_that_fit(harness):
    cases = [(0, 12, 3, 3), (100, 12, 103, 3),                   # "@r\nACG\n+\nIII\n"
             (0, 6, 3, 0),                                       # "@r\n\n+\n\n": empty lines
             (0, 7, 3, 3),                                       # ">r\nACG\n": the quality line would be the sequence line
             (0, 8, 3, 3), (0, 9, 3, 3), (0, 10, 3, 3),          # the quality line inside or right behind the sequence line
             (0, 11, 3, 3),                                      # one byte between the two lines is enough
             (0, 3, 3, 3), (0, 2, 0, 3), (0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 1, 0),
             (10, 12, 9, 3), (10, 12, 5, 0),                     # the sequence line in front of the record
             (0, 0xFFFFFFFF, 3, 0xFFFFFFFF), (0, 0xFFFFFFFF, 3, 0xFFFFFFFE), (0, 0xFFFFFFFF, 0, 0x7FFFFFFF), (2 ** 40, 0xFFFFFFFF, 2 ** 40 + 3, 0x7FFFFFF0),
             (2 ** 62, 12, 2 ** 62 + 3, 3)]
    got = ask(harness, "fit", "".join(" ".join(map(str, c)) + "\n" for c in cases))
    assert got == [str(int(ref.lines_fit(*c))) for c in cases]
    assert got[:3] == ["1", "1", "1"] and got[3:8] == ["0", "0", "0", "0", "1"]
