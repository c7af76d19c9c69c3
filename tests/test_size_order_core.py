"""The rules of FQD_FAST_SORT=size / FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE (fastq-dupaway_amd/csrc/fqd_size_order_core.hpp) on the
CPU, in a harness built with the sanitizers (tests/native/size_order_check.cpp), against the plain-Python statement
(tests/size_order_reference.py): tier 1's digit at both sides of 255, tier 2's key and pass count at both sides of every
pass edge, the filter at both sides of both bounds, and a scalar two-tier sort made of the header's functions against the
statement's stable sort on inputs with many ties.  The device code that runs the same functions:
tests/test_gpu_size_order.py; the run: tests/test_fast_sort_cli.py."""
import random
import subprocess
from pathlib import Path

import pytest

import size_order_reference as ref
import size_reference as sizes

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "size_order_check.cpp"
EXE = HERE / "native" / "size_order_check"
TOP = 2 ** 31 - 1


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
    # records 0 .. 5; clusters {0, 3} {1} {2, 4, 5}: perm groups them, the sizes stand at the first members
    perm, head = [0, 3, 1, 2, 4, 5], [1, 0, 1, 1, 0, 0]
    size = sizes.sizes_from(perm, head)
    assert size == [2, 1, 3, 0, 0, 0]
    keep = [1, 1, 1, 0, 0, 0]
    assert ref.written_order(perm, head, size, keep) == [2, 0, 1]
    assert ref.filtered(size, keep, 2, 0) == ([1, 0, 1, 0, 0, 0], 1, 1)
    assert ref.filtered(size, keep, 1, 2) == ([1, 1, 0, 0, 0, 0], 1, 3)
    assert ref.filtered(size, keep, 1, None) == (keep, 0, 0)
    assert ref.written_order(perm, head, size, [1, 0, 1, 0, 0, 0]) == [2, 0]
    assert ref.written_order([0, 1, 2], [1, 1, 1], [1, 1, 1], [1, 1, 1]) == [0, 1, 2]      # ties: the place order
    assert ref.written_order([2, 0, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1]) == [2, 0, 1]
    assert ref.not_written_line(3, 7, False, 2, None) == "3 clusters holding 7 reads were not written (FQD_FAST_MINSIZE=2, FQD_FAST_MAXSIZE=none).\n"
    assert ref.not_written_line(1, 1, True, 1, 5) == "1 clusters holding 1 read pairs were not written (FQD_FAST_MINSIZE=1, FQD_FAST_MAXSIZE=5).\n"
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate([b"AC", b"GG", b"AC", b"TT", b"GG", b"GG"]))
    out, gone, records, written = ref.dedup_ordered([fq], by_size=True, sizeout=True)
    assert out[0] == b"@r1;size=3\nGG\n+\nII\n@r0;size=2\nAC\n+\nII\n@r3;size=1\nTT\n+\nII\n" and (gone, records, written) == (0, 0, [3, 2, 1])
    out, gone, records, written = ref.dedup_ordered([fq], lo=2, hi=2)
    assert out[0] == b"@r0\nAC\n+\nII\n" and (gone, records, written) == (2, 4, [2])


def test_the_tier1_digit(harness):
    asked = [1, 2, 254, 255, 256, 257, 65535, 65536, TOP]
    got = ask(harness, "digit", "".join(f"{s}\n" for s in asked))
    assert len(got) == len(asked)
    for s, g in zip(asked, got):
        digit, size_back, low = map(int, g.split())
        assert digit == low == (256 - s if s <= 255 else 0) and size_back == s
    digits = [int(g.split()[0]) for g in got]
    assert digits[:6] == [255, 254, 2, 1, 0, 0]               # ascending digit is descending size; everything above 255 is bucket 0


def bits(v):
    return v.bit_length()


def test_the_tier2_key_and_pass_count(harness):
    asked = []
    for largest in (256, 257, 65791, 65792, TOP):
        for size in sorted({256, min(257, largest), (256 + largest) // 2, largest - 1 if largest > 256 else 256, largest}):
            asked.append((largest, size))
    got = ask(harness, "tier2", "".join(f"{a} {b}\n" for a, b in asked))
    assert len(got) == len(asked)
    for (largest, size), g in zip(asked, got):
        key, nbits, passes = map(int, g.split())
        assert key == largest - size and nbits == bits(largest - 256) and passes == (bits(largest - 256) + 7) // 8
        assert key < 2 ** nbits or (nbits == 0 and key == 0)   # the passes cover every bit of every key
    by_largest = {largest: int(g.split()[2]) for (largest, _), g in zip(asked, got)}
    assert by_largest == {256: 0, 257: 1, 65791: 2, 65792: 3, TOP: 4}
    # no bucket 0 at all: no pass
    assert [int(g.split()[2]) for g in ask(harness, "tier2", "1 1\n255 255\n")] == [0, 0]


def test_the_filter_at_both_sides_of_both_bounds(harness):
    asked = [(s, lo, hi) for lo, hi in ((1, 0), (2, 0), (1, 1), (2, 2), (3, 7), (7, 7), (256, 0), (1, 255), (TOP, 0), (TOP, TOP), (1, TOP))
             for s in sorted({1, max(1, lo - 1), lo, min(TOP, lo + 1), max(1, hi - 1), max(1, hi), min(TOP, hi + 1), TOP})]
    got = ask(harness, "drop", "".join(f"{s} {lo} {hi}\n" for s, lo, hi in asked))
    assert len(got) == len(asked)
    for (s, lo, hi), g in zip(asked, got):
        out, clusters, records = ref.filtered([s], [1], lo, hi)
        assert int(g) == clusters == 1 - out[0] and records == s * clusters, (s, lo, hi)
    assert [int(g) for g in ask(harness, "drop", "1 2 0\n2 2 0\n2 1 1\n1 1 1\n")] == [1, 0, 1, 0]


def grouping(rng, runs):
    """(perm, head, size) of clusters with the given member counts, in that order, under a shuffled perm."""
    n = sum(runs)
    perm = list(range(n))
    rng.shuffle(perm)
    head = [0] * n
    at = 0
    for r in runs:
        head[at] = 1
        at += r
    return perm, head, sizes.sizes_from(perm, head)


def sort_cases():
    rng = random.Random(31)
    yield grouping(rng, [1]) + ([1],)
    for pool in ([1], [1, 2, 3], [254, 255, 256, 257], [1, 2, 255, 256, 300, 300, 1000], [256, 256, 256, 511, 512, 513], [1, 1, 2, 70000], [300]):
        for count in ((1, 7) if max(pool) > 1000 else (1, 7, 60)):
            runs = [rng.choice(pool) for _ in range(count)]
            perm, head, size = grouping(rng, runs)
            for p in (1.0, 0.5):
                keep = [int(s > 0 and rng.random() < p) for s in size]
                yield perm, head, size, keep
    perm, head, size = grouping(rng, [3, 2, 1])
    yield perm, head, size, [0] * len(perm)                   # nothing is kept


def test_a_scalar_two_tier_sort_is_the_stable_sort(harness):
    n_ties = 0
    for perm, head, size, keep in sort_cases():
        n = len(perm)
        got = ask(harness, "order", f"{n}\n" + "".join(f"{perm[k]} {head[k]} {size[k]} {keep[k]}\n" for k in range(n)))
        expect = ref.written_order(perm, head, size, keep)
        assert int(got[0]) == len(expect) and [int(g) for g in got[1:]] == expect
        kept_sizes = [size[r] for r in expect]
        assert kept_sizes == sorted(kept_sizes, reverse=True)
        n_ties += len(kept_sizes) - len(set(kept_sizes))
    assert n_ties > 500                                       # many ties, below and above 255
