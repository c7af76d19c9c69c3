"""The rules of FQD_FAST_SIZEOUT / FQD_FAST_LEVELS (fastq-dupaway_amd/csrc/fqd_size_core.hpp) on the CPU, in a harness built
with the sanitizers (tests/native/size_check.cpp), against the plain-Python statement (tests/size_reference.py): the level
of a size at both sides of every level edge, the label's text and length, where the first word of an ID line ends — the
scalar rule and the sixteen lanes of the device search — the max-scan that finds every place's run start across tiles without
a head, and the labelled copy lane by lane.  The device code that runs the same functions: tests/test_gpu_sizes.py; the run:
tests/test_fast_sizes_cli.py."""
import random
import subprocess
from pathlib import Path

import pytest

import size_reference as ref

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "size_check.cpp"
EXE = HERE / "native" / "size_check"


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(EXE), str(SRC)], check=True, capture_output=True)
    return str(EXE)


def ask(harness, what, text):
    r = subprocess.run([harness, what], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return r.stdout.splitlines()


def test_the_statement_itself():
    assert [ref.level(s) for s in (1, 9, 10, 49, 50, 99, 100, 499, 500, 999, 1000, 4999, 5000, 9999, 10000, 2 ** 31 - 1)] == \
        [0, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15]
    assert ref.labelled(b"@r1 1:N:0:ATCACG\nACGT\n+\nIIII\n", 3) == b"@r1;size=3 1:N:0:ATCACG\nACGT\n+\nIIII\n"
    assert ref.labelled(b"@r1\nACGT\n+\nIIII\n", 3) == b"@r1;size=3\nACGT\n+\nIIII\n"
    assert ref.labelled(b">x;size=7\tc\nAC\n", 1) == b">x;size=7;size=1\tc\nAC\n"       # what is there already is not looked at
    assert ref.sizes_from([0, 2, 1, 3], [1, 0, 1, 0]) == [2, 2, 0, 0]             # runs {0, 2} and {1, 3}
    assert ref.sizes_from([3, 0, 1, 2], [1, 1, 0, 0]) == [3, 0, 0, 1]
    text = ref.duplevels_text([1, 1, 3, 12, 10000]).decode().splitlines()
    assert len(text) == 19 and text[0] == "#level\tclusters\trecords" and text[1] == "1\t2\t2" and text[3] == "3\t1\t3"
    assert text[10] == "10-49\t1\t12" and text[16] == "10000+\t1\t10000" and text[17] == "#total\t5\t10017" and text[18] == "#largest\t10000"


def test_level_at_both_sides_of_every_edge(harness):
    sizes = sorted({s for lo in ref.LOWER for s in (lo - 1, lo, lo + 1) if s >= 1} | {2 ** 31 - 1, 2 ** 31 - 2, 123456})
    got = ask(harness, "level", "".join(f"{s}\n" for s in sizes))
    assert [int(g) for g in got] == [ref.level(s) for s in sizes]
    assert ref.level(2 ** 31 - 1) == 15


def test_label_text_and_length(harness):
    sizes = [1, 9]
    for d in range(2, 11):
        sizes += [10 ** (d - 1), 10 ** d - 1 if d < 10 else 4294967295]
    sizes += [4294967295, 2 ** 31 - 1, 1234567]
    got = ask(harness, "label", "".join(f"{s}\n" for s in sizes))
    for s, g in zip(sizes, got):
        n, text = g.split()
        assert text.encode() == ref.label(s) and int(n) == len(ref.label(s)) == 6 + len(str(s))
    assert len(got) == len(sizes)


def word_lines():
    rng = random.Random(21)
    yield b"@"                                               # '@' alone
    yield b"@\n"
    for end in b" \t\r\n":
        yield b"@r1" + bytes([end]) + b"1:N:0:ATCACG\n"
        yield b">" + bytes([end]) + b"x\n"                       # an empty first word
    yield b"@no_end_at_all"
    yield b"@" + b"x" * 40                                    # none, longer than a chunk
    for at in (14, 15, 16, 17, 18, 31, 32, 33, 255, 256, 257, 258, 300, 511, 512, 513):      # the end at and around the chunk and round edges
        for end in b" \t\r\n":
            yield b"@" + bytes(rng.choice(b"abcXYZ:;=_0189") for _ in range(at - 1)) + bytes([end]) + b"tail with spaces\n"
        yield b"@" + b"w" * (at - 1) + b"\n"                    # the line's own '\n' is the end
    for L in range(1, 80):                                    # every length, an end somewhere or nowhere
        body = bytearray(rng.choice(b"abc:=;") for _ in range(L - 1))
        if L > 2 and rng.random() < 0.7:
            body[rng.randrange(L - 1)] = rng.choice(b" \t\r\n")
        yield b"@" + bytes(body)
    yield b" @x y\n"                                          # position 0 is never a word end, whatever stands there


def test_first_word_end_scalar_and_lanes(harness):
    lines = list(word_lines())
    got = ask(harness, "word", "".join(line.hex() + "\n" for line in lines))
    assert len(got) == len(lines)
    for line, g in zip(lines, got):
        scalar, lanes = map(int, g.split())
        assert scalar == lanes == ref.first_word_end(line), line


def head_sets():
    rng = random.Random(22)
    yield [1]
    yield [1] * 9
    yield [1] + [0] * 30                                      # one run over many tiles without a head
    yield [1, 0, 0, 1] + [0] * 13 + [1, 0, 0, 0, 1]           # runs that begin on a tile's last place and on its first
    for n in (2, 3, 4, 5, 7, 8, 9, 63, 64, 65):
        yield [1] + [int(rng.random() < 0.3) for _ in range(n - 1)]
        yield [1] + [int(rng.random() < 0.05) for _ in range(n - 1)]


def test_the_scan_gives_every_place_its_run_start(harness):
    for head in head_sets():
        got = ask(harness, "scan", f"{len(head)}\n" + "".join(f"{h}\n" for h in head))
        expect, start = [], None
        for k, h in enumerate(head):
            start = k if h else start
            expect.append(start)
        assert [int(g) for g in got] == expect


def test_the_labelled_copy_lane_by_lane(harness):
    cases = [(at, tail, size) for at in list(range(0, 41)) + [127, 128, 129, 300] for tail in list(range(0, 41)) + [127, 128, 129, 300]
             for size in ((7,) if (at + tail) % 3 else (7, 4294967295))]
    cases += [(33, 300, 10 ** d) for d in range(10)] + [(1, 1, 1), (0, 0, 12)]
    got = ask(harness, "copy", "".join(f"{a} {t} {s}\n" for a, t, s in cases))
    assert len(got) == len(cases)
    for (at, tail, size), g in zip(cases, got):
        src = bytes((37 * k + 11) % 251 for k in range(at + tail))
        assert bytes.fromhex(g) == src[:at] + ref.label(size) + src[at:], (at, tail, size)
