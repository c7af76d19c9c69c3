"""The rule of FQD_FAST_UMI (fastq-dupaway_amd/csrc/fqd_umi_core.hpp) on the CPU, in a harness built with the sanitizers
(tests/native/umi_check.cpp): the header's host compile against the plain-Python statement (tests/umi_reference.py) on the
edge list of tests/umi_cases.py and on random ID lines; (`lanes`) the very functions the kernels' sixteen lanes a record
run — the find over one or more rounds, the classing of the field, the table gather and the copy at every destination
alignment mod 16 — played lane after lane into buffers of the exact size; whole files, where a record's shape is held
against record 0's; and the injectivity of the key, exhaustively for shapes up to length 5 over ACGTN+.  The device code:
tests/test_gpu_umi.py; the run: tests/test_fast_umi_cli.py."""
import random
import subprocess
from pathlib import Path

import pytest

import umi_reference as ref
from umi_cases import COLON, random_lines, random_umi, refused_cases, shape_files, taken_cases

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "umi_check.cpp"
EXE = HERE / "native" / "umi_check"


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


def sep_name(sep):
    return "c" if sep == COLON else "u"


def expected_answer(line, sep, seq):
    off, u = ref.umi_of(line, sep)
    if isinstance(u, int):
        return f"{u} {off}"
    ulen, joiners = ref.shape(u)
    return f"0 {off} {ulen} {joiners:x} {hexed(ref.bases(u) + seq)}"


def check_records(harness, what, records):
    """records: [(name, line, sep, seq, align)]."""
    got = ask(harness, what, "".join(f"{sep_name(sep)} {hexed(line)} {hexed(seq)} {align}\n" for _, line, sep, seq, align in records))
    assert len(got) == len(records)
    for (name, line, sep, seq, align), answer in zip(records, got):
        assert answer == expected_answer(line, sep, seq), (name, line, align)


@pytest.mark.parametrize("what", ["rule", "lanes"])
def test_edge_list(harness, what):
    rng = random.Random(51)
    taken, refused = taken_cases(), refused_cases()
    records = [(name, line, sep, random_umi(rng, rng.choice([0, 1, 15, 16, 17, 40]), "ACGT"), k % 16) for k, (name, line, sep) in enumerate(taken)]
    records += [(name, line, sep, b"ACGT", 0) for name, line, sep, _ in refused]
    check_records(harness, what, records)
    for name, line, sep in taken:
        assert not isinstance(ref.umi_of(line, sep)[1], int), name
    for name, line, sep, reason in refused:
        assert ref.umi_of(line, sep)[1] == reason, name
    assert {r for _, _, _, r in refused} == {ref.NO_SEPARATOR, ref.EMPTY, ref.TOO_LONG, ref.BAD_BYTE, ref.NO_BASE}


@pytest.mark.parametrize("what", ["rule", "lanes"])
def test_random_id_lines(harness, what):
    rng = random.Random(52)
    lines = random_lines(53, 6000)
    records = [(f"random {k}", line, sep, random_umi(rng, rng.choice([0, 3, 16, 33]), "ACGT"), rng.randrange(16)) for k, (line, sep) in enumerate(lines)]
    verdicts = [ref.umi_of(line, sep)[1] for line, sep in lines]
    assert {v for v in verdicts if isinstance(v, int)} == {ref.NO_SEPARATOR, ref.EMPTY, ref.TOO_LONG, ref.BAD_BYTE, ref.NO_BASE}
    assert sum(not isinstance(v, int) for v in verdicts) > 300
    check_records(harness, what, records)


def test_gather_and_copy_at_every_alignment_and_length(harness):
    # every destination alignment mod 16 against every Lb mod 16 and the sequence lengths round a chunk and a round
    rng = random.Random(54)
    records = []
    for umi_len in (1, 2, 7, 15, 16, 17, 31, 33, 63, 64):
        for joiner in (False, True):
            u = bytearray(random_umi(rng, umi_len))
            if joiner and umi_len > 2:
                u[rng.randrange(1, umi_len - 1)] = ord("+")
            line = b"@R:" + bytes(u) + b" c\n"
            for L in (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257):
                for align in range(16):
                    records.append((f"U of {umi_len}, sequence of {L}, at {align}", line, COLON, random_umi(rng, L, "ACGT"), align))
    check_records(harness, "lanes", records)


def test_files_are_held_against_record_zero(harness):
    seen = set()
    for name, lines, sep in shape_files():
        (answer,) = ask(harness, "file", "".join(f"{sep_name(sep)} {hexed(x)}\n" for x in lines))
        _, info = ref.find(lines, sep)
        bad = -1 if info["bad_record"] == ref.NO_RECORD else info["bad_record"]
        assert answer == f"{bad} {info['bad_reason']} {info['umi_len']} {info['joiners']:x} {info['n_bases']}", name
        seen.add((bad, info["bad_reason"]))
    assert {(-1, ref.OK), (1, ref.SHAPE_DIFFERS), (69, ref.SHAPE_DIFFERS), (13, ref.SHAPE_DIFFERS), (0, ref.NO_SEPARATOR), (20, ref.BAD_BYTE)} <= seen


def test_the_key_is_injective_for_every_shape_up_to_length_five(harness):
    (line,) = ask(harness, "injective")
    strings = sum(6 ** L - 1 for L in range(1, 6))             # all but the joiners-only string of every length
    shapes = sum(2 ** L - 1 for L in range(1, 6))
    assert line == f"{strings} {shapes}"


def test_the_statement_itself():
    # of the yardstick, so that the other tests lean on something checked by hand
    assert ref.umi_of(b"@A00:1:FC:1:1101:1000:2000:ACGTACGT 1:N:0:ATCACG\n", b":") == (27, b"ACGTACGT")
    assert ref.umi_of(b"@A00:1:FC:1:1101:1000:2000:ACGT+TGCA 1:N:0:ATCACG\n", b":") == (27, b"ACGT+TGCA")
    assert ref.umi_of(b"@READ_ACGTACGT\n", b"_") == (6, b"ACGTACGT")
    assert ref.umi_of(b"@READ_ACGTACGT\n", b":") == (0, ref.NO_SEPARATOR)
    assert ref.umi_of(b"@READ 1:N:0:ACGT\n", b":") == (0, ref.NO_SEPARATOR)
    assert ref.umi_of(b"@A: x\n", b":") == (3, ref.EMPTY)
    assert ref.shape(b"ACGT+TGCA") == (9, 1 << 4) and ref.bases(b"ACGT+TGCA") == b"ACGTTGCA"
    assert ref.bases(b"AC+GTA") == ref.bases(b"ACG+TA") and ref.shape(b"AC+GTA") != ref.shape(b"ACG+TA")
    offs, info = ref.find([b"@r:AC+GTA\n", b"@r:ACG+TA\n"], b":")
    assert (info["bad_record"], info["bad_reason"], info["n_bases"], info["umi_len"], info["joiners"]) == (1, ref.SHAPE_DIFFERS, 5, 6, 4)
    assert list(offs) == [3, 3]
    assert list(ref.expected_keep([ref.key_of(b"@r:ACGT\n", b":", b"AAA"), ref.key_of(b"@q:ACGA\n", b":", b"AAA"),
                                   ref.key_of(b"@s:ACGT x\n", b":", b"AAA")])) == [1, 1, 0]
