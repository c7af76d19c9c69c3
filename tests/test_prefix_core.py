"""The rule of FQD_FAST_PREFIX (fastq-dupaway_amd/csrc/fqd_prefix_core.hpp) on the CPU, in a stand-alone harness built with the
sanitizers (tests/native/prefix_check.cpp): the header's host compile — the seed key at every L and start alignment, the overlap
compare as eight lanes of sixteen bytes play it, the direction rule, the packing order of `best`, the parents, the pointer jumps'
fixed point and count, the group ends of fqd_groups_core.hpp — against the sequential statement (tests/prefix_reference.py), and
what the header proves by exhaustion.  The device code: tests/test_gpu_prefix.py; the run: tests/test_fast_prefix_cli.py.

"All sets of strings up to length 6 over two letters" are 2^126 sets, so the exhaustion is bounded like this: EVERY set of the 14
strings of length 1 .. 3 over two letters (16384 sets, at L = 1, 2 and 3); of the 126 strings of length 1 .. 6 the one set of all
of them and 300 random sets at every L in 1 .. 6; for pairs 300 random sets of the 196 pairs of strings of length 1 .. 3."""
import random
import subprocess
from pathlib import Path

import pytest

import prefix_reference as ref
from prefix_cases import chain, pair_directions, random_records, template

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "prefix_check.cpp"
EXE = HERE / "native" / "prefix_check"


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


def test_the_seed_key_at_every_overlap_and_alignment(harness):
    rng = random.Random(1)
    cases = []
    for L in list(range(1, 41)) + [150, 151, 255, 256, 257, 65535]:
        for offset in range(16):
            paired = (L + offset) % 2
            cases.append((paired, L, int(offset == 7), offset, template(rng, L), template(rng, L) if paired else b""))
    got = ask(harness, "seeds", "".join(f"{p} {L} {weak} {off} {hexed(m1)} {hexed(m2)}\n" for p, L, weak, off, m1, m2 in cases))
    assert len(got) == len(cases)
    for (paired, L, weak, _, m1, m2), line in zip(cases, got):
        node = (m1 + b"TAIL", m2 + b"G") if paired else (m1 + b"TAIL",)       # what stands behind the L bytes is not in the key
        assert int(line, 16) == ref.node_seed(node, L, bool(weak)), (paired, L, weak)
    # what goes into a key: paired?, L, and the first L bytes of each mate
    a, b = template(rng, 40), template(rng, 40)
    assert ref.node_seed((a,), 20) == ref.node_seed((a[:20] + b,), 20) != ref.node_seed((a,), 21)
    assert ref.node_seed((a, b), 20) == ref.node_seed((a[:20], b[:20] + a), 20) != ref.node_seed((a,), 20)
    assert ref.node_seed((a, b), 20) != ref.node_seed((b, a), 20) and ref.node_seed((a, b), 20) != ref.node_seed((a, a), 20)


def test_the_overlap_compare_at_every_length_and_position(harness):
    rng = random.Random(2)
    cases = []
    for length in list(range(71)) + [127, 128, 129, 143, 144, 145, 255, 256, 257]:
        a = template(rng, length)
        cases.append((length % 16, a, a, None))
        for at in range(length):                                # a differing byte at every position, any alignment
            b = bytearray(a)
            b[at] ^= rng.choice([1, 0x20, 0x80, 0xFF])
            cases.append(((length + at) % 16, a, bytes(b), at))
        if length >= 2:                                         # the first difference decides the rounds
            b = bytearray(a)
            b[0] ^= 4
            b[length - 1] ^= 4
            cases.append((3, a, bytes(b), 0))
    got = ask(harness, "overlap", "".join(f"{off} {hexed(a)} {hexed(b)}\n" for off, a, b, _ in cases))
    assert len(got) == len(cases)
    for (_, a, b, at), line in zip(cases, got):
        equal, rounds = map(int, line.split())
        chunks = -(-len(a) // 16)
        want_rounds = -(-chunks // 8) if at is None else at // 16 // 8 + 1      # no round behind the first with a difference
        assert (equal, rounds) == (int(at is None), want_rounds), (len(a), at, equal, rounds)


def test_the_direction_rule(harness):
    cases = [(0, a, 0, b, 0) for a in range(5) for b in range(5)] + [(1, a1, a2, b1, b2) for a1 in range(4) for a2 in range(4) for b1 in range(4) for b2 in range(4)]
    got = [int(x) for x in ask(harness, "direction", "".join(" ".join(map(str, c)) + "\n" for c in cases))]
    for (paired, a1, a2, b1, b2), d in zip(cases, got):
        a, b = ((a1, a2), (b1, b2)) if paired else ((a1,), (b1,))
        same_sided_a = all(x <= y for x, y in zip(a, b)) and a != b
        same_sided_b = all(x >= y for x, y in zip(a, b)) and a != b
        assert d == (1 if same_sided_a else 2 if same_sided_b else 0), (paired, a, b)
    named = {"same-sided": (1, 5, 7, 9, 9, 1), "same-sided, turned": (1, 9, 9, 5, 7, 2), "opposite-sided": (1, 5, 9, 9, 7, 0), "mate 1 equal, mate 2 longer": (1, 5, 7, 5, 9, 1),
             "mate 2 equal, mate 1 shorter": (1, 5, 7, 4, 7, 2), "one shape": (1, 5, 7, 5, 7, 0)}
    answers = ask(harness, "direction", "".join(" ".join(map(str, c)) + "\n" for *c, _ in named.values()))
    assert [int(x) for x in answers] == [want for *_, want in named.values()], list(named)


def test_the_packing_order_of_best(harness):
    rng = random.Random(3)
    pairs = [(s, v) for s in (0, 1, 2, 300, 65535 * 2, 2 ** 32 - 2) for v in (0, 1, 7, 2 ** 31 - 2)] + [(rng.randrange(2 ** 32 - 1), rng.randrange(2 ** 31)) for _ in range(200)]
    got = [int(x) for x in ask(harness, "pack", "".join(f"{s} {v}\n" for s, v in pairs))]
    assert got == [ref.pack(s, v) for s, v in pairs]
    assert sorted(range(len(pairs)), key=lambda k: got[k]) == sorted(range(len(pairs)), key=lambda k: pairs[k])      # least span first, then the lowest record
    assert max(got) < ref.NO_PARENT                                          # all ones stay "no parent"


def forest_text(records, L):
    paired = len(records[0]) > 1
    return f"{int(paired)} {L} {len(records)}\n" + "".join(f"{hexed(r[0])} {hexed(r[1]) if paired else '-'}\n" for r in records)


def check_forest(harness, nodes, L):
    """Distinct nodes through the header's all-pairs parents and its trees, against the statement."""
    assert len(set(nodes)) == len(nodes)
    _, ids, parent = ref.parents(nodes, L, ref.all_pairs)
    assert ids == list(range(len(nodes)))
    got = ask(harness, "forest", forest_text(nodes, L))
    jumps, deepest = map(int, got[0].split())
    rows = [tuple(map(int, line.split())) for line in got[1:]]
    assert rows == [(parent[v], ref.root_of(parent, v)) for v in ids]
    want_deepest = max((ref.depth_of(parent, v) for v in ids), default=0)
    assert (jumps, deepest) == (ref.jumps_for(want_deepest), want_deepest)
    return deepest


def test_parents_and_trees_against_the_statement(harness):
    rng = random.Random(4)
    for L in (1, 5, 20):
        for paired in (False, True):
            nodes = list(dict.fromkeys(random_records(rng, L, nodes=150, templates=6, paired=paired, length=40)))
            assert check_forest(harness, nodes, L) >= 2
    records, _ = pair_directions(rng, 8)
    check_forest(harness, records, 8)
    for depth in range(1, 65):
        nodes = chain(rng, 4, depth)
        rng.shuffle(nodes)
        assert check_forest(harness, nodes, 4) == depth


def test_pointer_jumps_on_random_forests_and_chains(harness):
    rng = random.Random(5)
    def run(up):
        got = ask(harness, "jumps", f"{len(up)}\n" + "".join(f"{u}\n" for u in up))
        jumps, deepest = map(int, got[0].split())
        roots, count = ref.jump(up)
        assert [int(line.split()[1]) for line in got[1:]] == roots and jumps == count
        parent = dict(enumerate(up))
        assert roots == [ref.root_of(parent, v) for v in range(len(up))]
        assert deepest == max((ref.depth_of(parent, v) for v in range(len(up))), default=0) and jumps == ref.jumps_for(deepest)
        return jumps
    run([])
    run([0])
    for depth in range(1, 65):
        order = list(range(depth + 1))
        rng.shuffle(order)                                      # order[k] hangs under order[k + 1]
        up = [0] * (depth + 1)
        for k, v in enumerate(order):
            up[v] = order[k + 1] if k < depth else v
        assert run(up) == ref.jumps_for(depth)
    for n in (2, 10, 100, 1000, 3000):
        for _ in range(3):
            rank = list(range(n))
            rng.shuffle(rank)                                   # a node hangs under one of higher rank, or under nobody
            up = []
            for v in range(n):
                above = [u for u in rng.sample(range(n), min(n, 4)) if rank[u] > rank[v]]
                up.append(above[0] if above and rng.random() < 0.8 else v)
            run(up)


def test_group_ends_in_a_sorted_key_array(harness):
    rng = random.Random(6)
    for sizes in ([1], [5], [1, 1, 1], [2, 1, 3], [7, 8, 9, 63, 64, 65], [1000, 1, 2049, 3], [rng.randrange(1, 40) for _ in range(200)]):
        keys = sorted({rng.getrandbits(64) for _ in sizes} | {0, 2 ** 64 - 1})[:len(sizes)]
        flat = [k for k, s in zip(keys, sizes) for _ in range(s)]
        want, at = [], 0
        for s in sizes:
            want += [f"{at} {at + s}"] * s
            at += s
        assert ask(harness, "groups", f"{len(flat)}\n" + "\n".join(map(str, flat)) + "\n") == want


def test_the_theorems_by_exhaustion(harness):
    for L in (1, 2, 3):                                         # every set of the 14 strings of length 1 .. 3 over two letters
        got = ask(harness, "exhaust", f"2 3 {L} 0 0\n")
        assert len(got) == 1 and got[0].startswith("sets 16384 nodes 114688 children "), got
        assert (int(got[0].split()[5]) > 0) == (L < 3) and int(got[0].split()[7]) == 3 - L
    for L in range(1, 7):                                       # the 126 strings of length 1 .. 6: all of them, and random sets
        got = ask(harness, "exhaust", f"2 6 {L} 0 0\n")
        assert got == [f"sets 1 nodes 126 children {126 - 2 ** 6 - (2 ** L - 2)} deepest {6 - L}"], got      # all but the longest and the ineligible hang under a longer one
        got = ask(harness, "exhaust", f"2 6 {L} 300 {L}\n")
        assert len(got) == 1 and got[0].startswith("sets 300 nodes "), got
    for L in (1, 2):                                            # pairs: a bounded sample
        got = ask(harness, "exhaust2", f"300 {L} {L}\n")
        assert len(got) == 1 and got[0].startswith("sets 300 nodes ") and int(got[0].split()[5]) > 0, got


def test_the_statement_holds_its_own_theorems():
    rng = random.Random(7)
    for L in (1, 3):
        for paired in (False, True):
            records = random_records(rng, L, nodes=300, templates=8, paired=paired, length=30)
            assert ref.check_the_theorems(records, L) > 0
            assert ref.parents(records, L)[2] == ref.parents(records, L, ref.all_pairs)[2]      # the two ways to find the pairs agree
