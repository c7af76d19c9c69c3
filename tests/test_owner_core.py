"""The rules of FQD_FAST_KEEP / FQD_FAST_CLUSTERS (fastq-dupaway_amd/csrc/fqd_owner_core.hpp) on the CPU, in a harness
built with the sanitizers (tests/native/owner_check.cpp): whatever earlier member of its key a duplicate's link names,
the chain ends at the key's first record; the grouping key orders clusters by their first member and members by input
order.  The device code that runs the same functions: tests/test_gpu_owners.py; the run: tests/test_fast_keep_cli.py."""
import random
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "owner_check.cpp"
EXE = HERE / "native" / "owner_check"
BROKEN = 2 ** 32 - 1


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(EXE), str(SRC)], check=True, capture_output=True)
    return str(EXE)


def ask(harness, what, text):
    r = subprocess.run([harness, what], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def first_index(keys):
    seen = {}
    return [seen.setdefault(k, i) for i, k in enumerate(keys)]


def random_links(rng, keys, junk=True):
    """keep flags and, for every non-first member of a key, a uniformly chosen earlier member of that key.  Entries of
    kept records are never written by the engine: they hold junk here (an index above their own, or anything)."""
    members, keep, link = {}, [], []
    for i, k in enumerate(keys):
        earlier = members.setdefault(k, [])
        keep.append(0 if earlier else 1)
        link.append(rng.choice(earlier) if earlier else (rng.randrange(2 ** 32) if junk else 0))
        earlier.append(i)
    return keep, link


def owners(harness, keep, link):
    got = ask(harness, "chain", f"{len(keep)}\n" + "".join(f"{k} {l}\n" for k, l in zip(keep, link)))
    assert len(got) == len(keep)
    return [g[0] for g in got], [g[1] for g in got]


def key_sets():
    rng = random.Random(11)
    yield "one record", [7]
    yield "all distinct", list(range(300))
    yield "all identical", [5] * 300
    yield "two keys interleaved", [i % 2 for i in range(301)]
    yield "few keys", [rng.randrange(7) for _ in range(2000)]
    yield "about a fifth duplicates", [rng.randrange(1600) for _ in range(2000)]
    yield "a heavy key among distinct ones", [0 if rng.random() < 0.5 else 10 + i for i in range(3000)]


@pytest.mark.parametrize("name,keys", list(key_sets()), ids=[k[0] for k in key_sets()])
def test_every_link_assignment_ends_at_the_first_record(harness, name, keys):
    rng = random.Random(12)
    expect = first_index(keys)
    for _ in range(8):
        keep, link = random_links(rng, keys)
        got, steps = owners(harness, keep, link)
        assert got == expect
        assert all(s == 0 for s, k in zip(steps, keep) if k)          # a kept record follows no link
        assert all(1 <= s <= i for i, (s, k) in enumerate(zip(steps, keep)) if not k)


def test_chain_of_maximal_length(harness):
    n = 5000
    keep = [1] + [0] * (n - 1)
    link = [12345] + list(range(n - 1))                      # every record names its predecessor
    got, steps = owners(harness, keep, link)
    assert got == [0] * n
    assert steps == list(range(n))


def test_a_link_that_does_not_decrease_ends_the_walk(harness):
    # memory the engine did not write: the walk reports it and never reads at or above the index it came from
    keep = [1, 0, 0, 0, 0]
    link = [0, 0, 2, 4, 2 ** 32 - 1]
    got, _ = owners(harness, keep, link)
    assert got == [0, 0, BROKEN, BROKEN, BROKEN]


def test_group_bits(harness):
    ns = [1, 2, 3, 4, 5, 255, 256, 257, 65536, 65537, 2 ** 31 - 1, 2 ** 31]
    got = ask(harness, "bits", "".join(f"{n}\n" for n in ns))
    assert [g[0] for g in got] == [max(1, (n - 1).bit_length()) for n in ns]


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000])
def test_grouping_key_order(harness, n):
    rng = random.Random(13 + n)
    for keys in ([rng.randrange(max(1, n // 3)) for _ in range(n)], list(range(n)), [0] * n,
                 [0] + [1] * (n - 2) + [0] if n > 2 else [0] * n):          # record 0 and record n-1 in one cluster
        owner = first_index(keys)
        got = ask(harness, "group", f"{n}\n" + "".join(f"{o}\n" for o in owner))
        assert got[0][0] == max(1, (n - 1).bit_length())
        perm = [g[0] for g in got[1:]]
        head = [g[1] for g in got[1:]]
        groups = {}
        for i, o in enumerate(owner):
            groups.setdefault(o, []).append(i)
        expect = [i for o in sorted(groups) for i in groups[o]]          # clusters by first member, members in input order
        assert perm == expect
        assert head == [int(k == 0 or owner[perm[k]] != owner[perm[k - 1]]) for k in range(n)]
        assert sum(head) == len(groups)
        assert all(owner[perm[k]] == perm[k] for k in range(n) if head[k])   # the owner stands first in its run
        if n - 1 in owner:                                   # an owner that needs every key bit (all distinct: record n-1)
            assert perm[-1] == n - 1
