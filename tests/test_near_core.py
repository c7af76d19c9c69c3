"""The rule of FQD_FAST_HAMMING (fastq-dupaway_amd/csrc/fqd_near_core.hpp) on the CPU, in a stand-alone harness built with the
sanitizers (tests/native/near_check.cpp): the header's host compile — segment bounds, the pigeonhole property by exhaustion,
the seed hash, the mismatch counter as eight lanes of sixteen bytes play it, and the fixed point and number of the label
sweeps — against the sequential statement (tests/near_reference.py) on the edge lists of tests/near_cases.py and on random
graphs.  The device code: tests/test_gpu_near.py; the run: tests/test_fast_hamming_cli.py."""
import random
import subprocess
from pathlib import Path

import pytest

import near_reference as ref
from near_cases import difference_pairs, graph_cases, lengths_for, random_graph, template

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "near_check.cpp"
EXE = HERE / "native" / "near_check"


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(EXE), str(SRC)], check=True, capture_output=True)
    return str(EXE)


def ask(harness, what, text=""):
    r = subprocess.run([harness, what], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


def hexed(b):
    return b.hex() if b else "-"


def test_segment_bounds(harness):
    want = [" ".join(map(str, [D, length] + [ref.bound(length, D, j) for j in range(D + 2)])) for D in (1, 2, 3) for length in range(41)]
    assert ask(harness, "bounds") == want
    for D in (1, 2, 3):
        for length in range(41):
            b = [ref.bound(length, D, j) for j in range(D + 2)]
            assert b[0] == 0 and b[-1] == length and b == sorted(b)                     # disjoint, and they cover the read
            assert max(y - x for x, y in zip(b, b[1:])) - min(y - x for x, y in zip(b, b[1:])) <= 1


def test_pigeonhole_by_exhaustion(harness):
    # every pair of strings over three letters up to length 7 (lengths below D + 1, with their empty segments, among them)
    got = ask(harness, "pigeonhole")
    assert len(got) == 1 and got[0].startswith("pairs "), got
    pairs, near = int(got[0].split()[1]), int(got[0].split()[3])
    assert pairs == 3 * sum(3 ** k * (3 ** k - 1) // 2 for k in range(8)) and 0 < near < pairs


def test_seed_keys(harness):
    rng = random.Random(7)
    cases = []
    for D in (1, 2, 3):
        for length in list(range(0, 72)) + [150, 151, 255, 256, 257]:
            cases.append((D, rng.choice([0, 0, 9, 150]), rng.randrange(2), template(rng, length)))
    got = ask(harness, "seeds", "".join(f"{D} {len2} {weak} {hexed(m1)}\n" for D, len2, weak, m1 in cases))
    assert len(got) == len(cases)
    for (D, len2, weak, m1), line in zip(cases, got):
        node = (m1, b"x" * len2) if len2 else (m1,)
        assert [int(x, 16) for x in line.split()] == ref.node_seeds(node, D, bool(weak)), (D, len2, weak, len(m1))
    # what goes into a key: the shape, the segment's number and the segment's bytes
    a = template(rng, 40)
    assert ref.node_seeds((a, b"A"), 2) != ref.node_seeds((a, b"AC"), 2)
    assert len(set(ref.node_seeds((b"",), 3))) == 4                                      # empty segments, one key for each j
    assert ref.node_seeds((a,), 1)[0] != ref.node_seeds((a + b"A",), 1)[0]


def test_mismatch_counter_at_every_length_and_position(harness):
    rng = random.Random(8)
    cases = []
    for length in range(71):
        a = template(rng, length)
        cases.append((3, length % 16, a, a, 0))
        for at in range(length):                                # one differing byte at every position, any alignment
            b = bytearray(a)
            b[at] ^= rng.choice([1, 0x20, 0x80, 0xFF])
            cases.append((rng.randrange(4), (length + at) % 16, a, bytes(b), 1))
        for count in (2, 3, 4, 5, length):                      # round the caps, and everything differs
            if count <= length:
                b = bytearray(a)
                for at in rng.sample(range(length), count):
                    b[at] ^= 0x55
                cases.append((rng.randrange(4), count % 16, a, bytes(b), count))
    for length in (150, 151, 255, 256, 257):                    # several rounds of eight lanes
        a = template(rng, length)
        for where in ([0], [length - 1], [127, 128], [0, 128, length - 1], list(range(0, length, 16)), list(range(length - 4, length))):
            b = bytearray(a)
            for at in where:
                b[at] ^= 2
            cases.append((3, length % 16, a, bytes(b), len(where)))
    got = ask(harness, "mismatch", "".join(f"{cap} {off} {hexed(a)} {hexed(b)}\n" for cap, off, a, b, _ in cases))
    assert len(got) == len(cases)
    for (cap, _, a, b, count), line in zip(cases, got):
        lanes, rule = map(int, line.split())
        assert count == ref.mismatches(a, b)
        # exact up to the cap; above it, above the cap
        assert (lanes == count if count <= cap else lanes > cap) and (rule == count if count <= cap else rule > cap), (len(a), cap, count, lanes, rule)


def test_near_on_the_difference_cases(harness):
    rng = random.Random(9)
    cases = []
    for D in (1, 2, 3):
        for paired in (False, True):
            for length in lengths_for(D):
                for name, a, b, want in difference_pairs(rng, length, D, paired):
                    assert ref.near(a, b, D) == want, (D, paired, length, name)
                    cases.append((D, paired, a, b, want))
    cases.append((1, False, (b"ACG",), (b"ACGA",), False))                               # same bytes, another length
    cases.append((3, True, (b"ACG", b"T"), (b"AC", b"GT"), False))                       # one concatenation, two shapes
    text = "".join(f"{D} {int(p)} {hexed(a[0])} {hexed(a[1]) if p else '-'} {hexed(b[0])} {hexed(b[1]) if p else '-'}\n" for D, p, a, b, _ in cases)
    got = ask(harness, "near", text)
    assert [int(x) for x in got] == [int(want) for *_, want in cases]


def check_graph(harness, name, places, edges):
    labels, sweeps = ref.sweeps(places, edges)
    assert labels == ref.components(places, edges), name         # the fixed point is the lowest place of every component
    got = ask(harness, "sweeps", f"{places} {len(edges)}\n" + "".join(f"{a} {b}\n" for a, b in edges))
    assert int(got[0]) == sweeps and [int(x) for x in got[1:]] == labels, name
    shuffled = list(edges) + list(edges[:3])
    random.Random(len(edges)).shuffle(shuffled)                   # neither the order nor the multiplicity of the edges reaches the result
    assert ref.sweeps(places, shuffled) == (labels, sweeps), name
    return sweeps


def test_sweeps_on_the_edge_lists(harness):
    for name, places, edges in graph_cases():
        sweeps = check_graph(harness, name, places, edges)
        assert sweeps <= max(places - 1, 0), name
        if name.startswith("chain of 40"):
            assert 0 < sweeps < 39, (name, sweeps)               # pointer jumping: fewer sweeps than links


def test_sweeps_on_random_graphs(harness):
    rng = random.Random(10)
    for places, edges in [(1, 0), (2, 1), (10, 4), (10, 30), (100, 60), (100, 100), (1000, 700), (1000, 1100), (3000, 2500)]:
        for _ in range(3):
            check_graph(harness, f"{places} places, {edges} edges", places, random_graph(rng, places, edges))
