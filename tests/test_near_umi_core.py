"""The rule of FQD_FAST_UMI_HAMMING (fastq-dupaway_amd/csrc/fqd_near_umi_core.hpp) on the CPU, in a stand-alone harness built
with the sanitizers (tests/native/near_umi_check.cpp): the header's host compile — the tag T(U) and the tagged seed key at every
UMI length round the eight-byte word with joiners at the first, last and word-boundary places, the tag compare as eight lanes
play it, and the components of near edges with links in front — against the sequential statement (tests/near_umi_reference.py)
on the edge lists of tests/near_cases.py.  The device code: tests/test_gpu_near_umi.py; the run: tests/test_fast_umi_hamming_cli.py."""
import random
import subprocess
from pathlib import Path

import pytest

import near_reference as near
import near_umi_reference as ref
from near_cases import graph_cases, random_graph, template

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "near_umi_check.cpp"
EXE = HERE / "native" / "near_umi_check"
UMI_LENGTHS = [1, 7, 8, 9, 15, 16, 17, 63, 64]


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


def joiner_sets(length):
    """Joiner places of a UMI of `length` bytes that leave a base: none, the first, the last, round every word boundary, several."""
    places = [[], [0], [length - 1], [0, length - 1]]
    for k in range(8, length, 8):
        places += [[k - 1], [k], [k - 1, k]]
    places.append(list(range(1, length, 3)))
    out = []
    for ps in places:
        ps = sorted({p for p in ps if 0 <= p < length})
        if len(ps) < length and ps not in out:
            out.append(ps)
    return out


def umi_with(rng, length, places, joiner=b"+"):
    u = bytearray(rng.choice(b"ACGTN") for _ in range(length))
    for p in places:
        u[p] = rng.choice(joiner)
    return bytes(u)


def shapes(rng):
    for length in UMI_LENGTHS:
        for places in joiner_sets(length):
            yield length, places, sum(1 << p for p in places), umi_with(rng, length, places, b"+-_")


def test_tags_at_every_length_and_joiner_place(harness):
    rng = random.Random(1)
    cases = [(joiners, (length * 3 + len(places)) % 16, u) for length, places, joiners, u in shapes(rng)]
    got = ask(harness, "tags", "".join(f"{j:x} {off} {hexed(u)}\n" for j, off, u in cases))
    assert len(got) == len(cases)
    for (j, _, u), line in zip(cases, got):
        assert ref.joiners_of(u) == j
        *words, count = line.split()
        want = ref.tag_words(u, j)
        assert int(count) == len(want) == (len(u) + 7) // 8
        assert [int(x, 16) for x in words] == want + [0] * (8 - len(want)), (len(u), hex(j))
        assert len(ref.tag(u, j)) == len(u) and all(t == (0 if c in b"+-_" else c) for t, c in zip(ref.tag(u, j), u))
    # the joiner's character is not in the tag; a base is
    assert ref.tag(b"AC+GT", 4) == ref.tag(b"AC-GT", 4) == b"AC\0GT" and ref.tag(b"AC+GT", 4) != ref.tag(b"AC+GA", 4)


def test_tagged_seed_keys(harness):
    rng = random.Random(2)
    cases = []
    for length, places, joiners, u in shapes(rng):
        for D in (1, 2, 3):
            cases.append((D, rng.choice([0, 0, 9, 150]), rng.randrange(2), joiners, u, template(rng, rng.choice([0, 1, D, D + 1, 15, 16, 17, 40, 150]))))
    got = ask(harness, "seeds", "".join(f"{D} {len2} {weak} {j:x} {hexed(u)} {hexed(m1)}\n" for D, len2, weak, j, u, m1 in cases))
    assert len(got) == len(cases)
    for (D, len2, weak, j, u, m1), line in zip(cases, got):
        record = (u, (m1, b"x" * len2) if len2 else (m1,))
        assert [int(x, 16) for x in line.split()] == ref.node_seeds(record, D, j, bool(weak)), (D, len2, weak, len(u), len(m1))
    # what goes into a key: the tag besides what fqd_near_core.hpp's key holds; not the joiner's character
    m = template(rng, 40)
    assert ref.node_seeds((b"ACGT", (m,)), 2, 0) != ref.node_seeds((b"ACGA", (m,)), 2, 0)
    assert ref.node_seeds((b"AC+GT", (m,)), 2, 4) == ref.node_seeds((b"AC_GT", (m,)), 2, 4)
    assert ref.node_seeds((b"ACGT", (m,)), 2, 0) != near.node_seeds((m,), 2)
    assert len(set(ref.node_seeds((b"ACGT", (b"",)), 3, 0))) == 4


def test_the_tag_compare_as_eight_lanes_play_it(harness):
    rng = random.Random(3)
    cases = []
    for length, places, joiners, u in shapes(rng):
        cases.append((joiners, u, u, 0))
        other = bytearray(u)
        for p in places:                                         # another joiner character at every joiner place: the same tag
            other[p] = ord("-") if u[p] != ord("-") else ord("_")
        cases.append((joiners, u, bytes(other), 0))
        bases = [p for p in range(length) if p not in places]
        for p in sorted({bases[0], bases[-1]} | {q for q in bases if q % 8 in (0, 7)}):     # one base differs: one lane says so
            v = bytearray(u)
            v[p] = ord("A") if u[p] != ord("A") else ord("C")
            cases.append((joiners, u, bytes(v), 1))
        v = bytes(ord("A") if c != ord("A") and k not in places else c if k in places else ord("C") for k, c in enumerate(u))
        cases.append((joiners, u, v, len({p // 8 for p in bases})))                            # every base differs: every word that holds one
    got = ask(harness, "lanes", "".join(f"{j:x} {hexed(a)} {hexed(b)}\n" for j, a, b, _ in cases))
    assert len(got) == len(cases)
    for (j, a, b, lanes), line in zip(cases, got):
        differ, count = map(int, line.split())
        assert (differ, count) == (int(lanes > 0), lanes), (len(a), hex(j), a, b)
        assert (ref.tag(a, j) != ref.tag(b, j)) == bool(differ)


def test_near_needs_equal_tags(harness):
    rng = random.Random(4)
    s = template(rng, 50)
    s1 = bytes([s[0] ^ 6]) + s[1:]
    cases = [(1, 0, b"ACGTACGT", b"ACGTACGT", s, s1, 1), (1, 0, b"ACGTACGT", b"ACGTACGA", s, s1, 0), (1, 0, b"ACGTACGT", b"ACGTACGA", s, s, 0),
             (3, 1 << 4, b"ACGT+ACGT", b"ACGT-ACGT", s, s1, 1), (3, 1 << 4, b"ACGT+ACGT", b"ACGT+ACGT", s, s[:-1], 0),
             (2, 0, b"A" * 64, b"A" * 63 + b"C", s, s1, 0), (2, 0, b"A" * 64, b"A" * 64, s, s1, 1)]
    got = ask(harness, "near", "".join(f"{D} {j:x} {hexed(ua)} {hexed(ub)} {hexed(a)} {hexed(b)}\n" for D, j, ua, ub, a, b, _ in cases))
    assert [int(x) for x in got] == [want for *_, want in cases]
    for D, j, ua, ub, a, b, want in cases:
        assert int(ref.tag(ua, j) == ref.tag(ub, j) and near.near((a,), (b,), D)) == want


def with_links(rng, places, share):
    """link[v] for every place: itself, or with probability `share` a lower place that is linked to itself (a cluster's first)."""
    link = list(range(places))
    for v in range(1, places):
        if rng.random() < share:
            link[v] = link[rng.randrange(v)]
    return link


def check_molecules(harness, name, places, edges, link):
    # every place is a node; two records more at the end are copies of places 0 and places - 1
    owner = list(range(places)) + ([0, places - 1] if places else [])
    links = [(link[v], v) for v in range(places) if link[v] != v]
    want = near.components(places, list(edges) + links)
    text = f"{len(owner)} {len(edges)}\n" + "".join(f"{o} {link[v] if v < places else 0}\n" for v, o in enumerate(owner)) + "".join(f"{a} {b}\n" for a, b in edges)
    got = [int(x) for x in ask(harness, "molecules", text)]
    assert got[0] == len(links), name
    assert got[2:] == [want[o] for o in owner], name
    labels, sweeps = near.sweeps(places, links + list(edges))
    assert labels == want and got[1] == sweeps, name


def test_components_with_links_on_the_edge_lists(harness):
    rng = random.Random(5)
    for name, places, edges in graph_cases():
        check_molecules(harness, name + ", no link", places, edges, list(range(places)))
        for share in (0.2, 0.7):
            check_molecules(harness, f"{name}, links {share}", places, edges, with_links(rng, places, share))
        check_molecules(harness, name + ", every place linked to place 0", places, edges, [0] * places)
    for places, edges in [(10, 4), (100, 60), (1000, 700), (3000, 2500)]:
        check_molecules(harness, f"{places} places, {edges} edges", places, random_graph(rng, places, edges), with_links(rng, places, 0.3))
    # a chain that exists only through a link: near edge (1, 2), link 1 -> 0
    check_molecules(harness, "through a link", 3, [(1, 2)], [0, 0, 2])


def test_a_bad_link_is_told(harness):
    for owner_link, bad in [([(0, 0), (1, 2), (2, 2)], 1),      # a link above its node
                            ([(0, 0), (0, 0), (2, 1)], 2),      # a link to a record that is no node
                            ([(0, 0), (1, 1), (1, 2)], None)]:  # a non-node's link is not looked at
        got = ask(harness, "molecules", f"{len(owner_link)} 0\n" + "".join(f"{o} {l}\n" for o, l in owner_link))
        assert (got == [f"bad {bad}"]) if bad is not None else got[0] == "0", (owner_link, got)
