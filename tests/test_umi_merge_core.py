"""The rule of FQD_FAST_UMI_MISMATCH (fastq-dupaway_amd/csrc/fqd_umi_merge_core.hpp) on the CPU, in a harness built with the
sanitizers (tests/native/umi_merge_check.cpp): the header's host compile — the packed words, the distance, the fixed point of
the label sweeps — against the sequential statement (tests/umi_merge_reference.py: rank order, a search per unclaimed node)
on the edge list of tests/umi_merge_cases.py and on random dense networks of 4-base UMIs; and the very functions the
kernels' lanes and threads run — eight lanes a group, a wave a group, a block a group — played one after another on buffers
of the exact size.  The device code: tests/test_gpu_umi_merge.py; the run: tests/test_fast_umi_merge_cli.py."""
import subprocess
from collections import OrderedDict
from pathlib import Path

import pytest

import umi_merge_reference as ref
import umi_reference as umi
from umi_merge_cases import bases, chain, dense_networks, edge_cases, hamming, seqkey

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "umi_merge_check.cpp"
EXE = HERE / "native" / "umi_merge_check"
MODES = ("rule", "lanes8", "lanes64", "block")
FITS = {"rule": 1 << 30, "lanes8": 8, "lanes64": 64, "block": 4096}


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(EXE), str(SRC)], check=True, capture_output=True)
    return str(EXE)


def ask(harness, what, text):
    r = subprocess.run([harness, what], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


def groups_of(records, both=False):
    """A case's records -> its sequence groups as lists of (field, count), the nodes in the order of their first records."""
    groups = OrderedDict()
    for field, seqs in records:
        nodes = groups.setdefault(seqkey(seqs, both), OrderedDict())
        nodes[bases(field)] = (field, nodes.get(bases(field), (field, 0))[1] + 1)
    return [list(nodes.values()) for nodes in groups.values()]


def expected_line(nodes, D):
    root, deepest = ref.directional([bases(f) for f, _ in nodes], [c for _, c in nodes], list(range(len(nodes))), D)
    lowest = {}
    for v, r in enumerate(root):
        lowest.setdefault(r, v)
    return f"{deepest} " + ",".join(f"{r}:{lowest[r]}" for r in root)


def check(harness, cases, modes=MODES):
    asked = {m: [] for m in modes}
    for name, D, records in cases:
        for nodes in groups_of(records):
            ulen, joiners = umi.shape(nodes[0][0])
            assert all(umi.shape(f) == (ulen, joiners) for f, _ in nodes), name
            line = f"{D} {ulen} {joiners:x} " + ",".join(f"{f.decode()}:{c}" for f, c in nodes)
            want = expected_line(nodes, D)
            for m in modes:
                if len(nodes) <= FITS[m]:
                    asked[m].append((name, line, want))
    for m, items in asked.items():
        assert items, m
        got = ask(harness, m, "".join(line + "\n" for _, line, _ in items))
        assert len(got) == len(items)
        for (name, line, want), answer in zip(items, got):
            assert answer == want, (m, name, line[:200])


def test_edge_list(harness):
    cases = edge_cases()
    check(harness, cases)
    # what the list is there for: the deepest searches are the singleton chains', one level a node
    names = {name: (D, records) for name, D, records in cases}
    for length in (2, 3, 64, 65, 300):
        for suffix in ("", ", reversed"):
            D, records = names[f"singleton chain of {length}{suffix}"]
            (nodes,) = groups_of(records)
            assert expected_line(nodes, D).startswith(f"{length - 1} ")


def test_random_dense_networks(harness):
    cases = dense_networks(72, 60)
    sizes = sorted(len(g) for _, _, records in cases for g in groups_of(records))
    assert sizes[0] == 1 and any(8 < s <= 64 for s in sizes) and sizes[-1] > 64
    merged = sum(r != v for _, D, records in cases for g in groups_of(records)
                 for v, r in enumerate(ref.directional([bases(f) for f, _ in g], [c for _, c in g], list(range(len(g))), D)[0]))
    assert merged > 500                                        # most nodes have neighbours
    check(harness, cases)


def test_a_group_at_the_limit(harness):
    # 4096 nodes, four nodes a thread of the block: a few hubs with many leaves, and a tail of singletons
    import random
    rng = random.Random(73)
    seen, nodes = set(), []
    while len(nodes) < 4096:
        u = bytes(rng.choice(b"ACGT") for _ in range(7))
        if u not in seen:
            seen.add(u)
            nodes.append((u, rng.choice([1, 1, 1, 2, 5, 40])))
    check(harness, [("at the limit", 1, [(u, (b"ACGT", None)) for u, c in nodes for _ in range(c)])], modes=("rule", "block"))


def test_the_statement_itself():
    # of the yardstick, so that the other tests lean on something checked by hand
    d = ref.directional
    assert d([b"AAAA", b"AAAC"], [1, 1], [0, 1], 1) == ([0, 0], 1)
    assert d([b"AAAA", b"AAAC"], [2, 2], [0, 1], 1) == ([0, 1], 0)            # 2 >= 2*2-1 fails both ways
    assert d([b"AAAA", b"AAAC"], [3, 2], [0, 1], 1) == ([0, 0], 1)
    assert d([b"AAAA", b"AAAC"], [2, 3], [0, 1], 1) == ([1, 1], 1)
    assert d([b"AAAA", b"AACC"], [9, 1], [0, 1], 1) == ([0, 1], 0) and d([b"AAAA", b"AACC"], [9, 1], [0, 1], 2) == ([0, 0], 1)
    assert d([b"AAAA", b"AAAC", b"AACC"], [10, 5, 3], [0, 1, 2], 1) == ([0, 0, 0], 2)
    assert d([b"AAAA", b"AAAC", b"AACC"], [10, 5, 4], [0, 1, 2], 1) == ([0, 0, 2], 1)
    assert d([b"AACC", b"AAAC", b"AAAA"], [8, 2, 8], [0, 1, 2], 1)[0] == [0, 0, 2]
    assert d([b"AACC", b"AAAC", b"AAAA"], [8, 2, 10], [0, 1, 2], 1)[0] == [0, 2, 2]
    assert d([b"ACGN", b"ACGT"], [1, 1], [0, 1], 1) == ([0, 0], 1)
    c = chain(9, 4)
    assert all(hamming(a, b) == 1 for a, b in zip(c, c[1:]))
    owner, info, owner_exact, owner_seq, size = ref.merge([b"AAAA", b"AAAC", b"AAAA", b"AAAC", b"AAAA", b"CCCC", b"AAAC"],
                                                         ["s", "s", "s", "t", "s", "s", "s"], 1, 4096)
    assert list(owner_exact) == [0, 1, 0, 3, 0, 5, 1] and list(owner_seq) == [0, 0, 0, 3, 0, 0, 0] and list(size) == [3, 2, 0, 1, 0, 1, 0]
    assert list(owner) == [0, 0, 0, 3, 0, 5, 0]
    assert info == dict(nodes=4, groups=1, merged=1, largest=3, sweeps=1, max_group=4096, over_limit_nodes=0, over_limit_first=ref.NO_RECORD)
    owner, info, *_ = ref.merge([b"AA", b"AC", b"CC", b"AA"], ["s", "s", "s", "t"], 1, 2)
    assert owner is None and (info["over_limit_first"], info["over_limit_nodes"], info["merged"], info["sweeps"]) == (0, 3, 0, 0)
    assert ref.clusters_of([0, 0, 0, 3, 0, 5, 0]) == [[0, 1, 2, 4, 6], [3], [5]]
