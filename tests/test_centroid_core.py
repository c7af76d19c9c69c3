"""The rule of FQD_FAST_CENTROID=abundant (fastq-dupaway_amd/csrc/fqd_centroid_core.hpp) on the CPU, in a stand-alone harness built
with the sanitizers (tests/native/centroid_check.cpp): the header's host compile — the abundances through the helpers of the
table in LDS and of the table in scratch, the saturation, the centroid, the masked scores and the second pick, by exhaustion
over runs of up to 6 members — against the sequential statement (tests/centroid_reference.py); the slot choice and the key
packing at their edges.  The device code: tests/test_gpu_centroid.py; the run: tests/test_fast_centroid_cli.py."""
import itertools
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

import centroid_reference as ref

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "centroid_check.cpp"
EXE = HERE / "native" / "centroid_check"
WEIGHTS = (1, 2, 2 ** 31 - 1)
SCORE = (5, 0xFFFFFFFF, 0xFFFFFFFE, 0, 7, 5)                   # centroid_check.cpp: kScore


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(EXE), str(SRC)], check=True, capture_output=True)
    return str(EXE)


def ask(harness, what, text=""):
    r = subprocess.run([harness, what], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


def labellings(s):
    """Every way s members share labels: restricted growth strings in lexicographic order."""
    def grow(ids, used):
        if len(ids) == s:
            yield tuple(ids)
            return
        for v in range(used + 1):
            yield from grow(ids + [v], used + 1 if v == used else used)
    return grow([], 0)


def small_runs(upto=6):
    """(labels, weights) in the harness's order: label value (7 * id + 3) % 11, member i's weight digit i of a base-3 counter."""
    for s in range(1, upto + 1):
        for ids in labellings(s):
            labels = [(7 * v + 3) % 11 for v in ids]
            for code in range(3 ** s):
                yield labels, [WEIGHTS[code // 3 ** i % 3] for i in range(s)]


def statement(labels, weights):
    """(abundances, centroid, masked scores behind the exchange, the member the second pick takes) of one run."""
    s = len(labels)
    perm, head = np.arange(s, dtype=np.uint32), np.array([1] + [0] * (s - 1), np.uint8)
    stored, exact, _ = ref.abundances(perm, head, labels, weights)
    order, _ = ref.pick(perm, head, stored)
    masked = ref.masked_scores(order, head, labels, SCORE[:s])
    best, _ = ref.pick(order, head, masked)
    assert int(order[0]) == ref.written(perm, head, labels, weights, stored=stored)[0]
    assert int(best[0]) == ref.written(perm, head, labels, weights, SCORE[:s], stored=stored)[0]
    return stored, exact, int(order[0]), masked, int(best[0])


def test_every_small_run(harness):
    got = ask(harness, "runs")
    assert len(got) == sum(n * 3 ** s for s, n in zip(range(1, 7), (1, 2, 5, 15, 52, 203)))     # Bell numbers
    k = 0
    for labels, weights in small_runs():
        stored, _, centroid, masked, best = statement(labels, weights)
        want = f"{','.join(map(str, stored))} {centroid} {','.join(map(str, masked))} {best}"
        assert got[k] == want, (k, labels, weights, got[k], want)
        k += 1
    assert k == len(got)


def test_what_the_small_runs_hold():
    seen = {"a tie taken by the order": 0, "a tie kept by the first member": 0, "a saturated sum": 0, "a centroid that is the last member": 0,
            "the second pick takes another member": 0}
    for labels, weights in small_runs(5):
        stored, exact, centroid, _, best = statement(labels, weights)
        top = max(stored)
        tied = {l for l, a in zip(labels, stored) if a == top}
        seen["a tie taken by the order"] += len(tied) > 1 and centroid != 0 and labels[0] not in tied
        seen["a tie kept by the first member"] += len(tied) > 1 and centroid == 0
        seen["a saturated sum"] += max(exact) > ref.SATURATED
        seen["a centroid that is the last member"] += centroid == len(labels) - 1 and len(labels) > 1
        seen["the second pick takes another member"] += best != centroid
        # the proofs' statements: the centroid is the first member of its sub-cluster; the first member stays iff it is among the maxima
        assert labels.index(labels[centroid]) == centroid
        assert (centroid == 0) == (stored[0] == top)
        assert len(set(labels)) > 1 or centroid == 0
        assert labels[best] == labels[centroid]
    assert all(seen.values()), seen


def test_the_tables_on_long_runs(harness):
    rng = random.Random(5)
    for s, head_place, pool in ((2048, 0, 2048), (2048, 7, 1), (1500, 2 ** 31 - 2, 3), (9000, 2 ** 31 - 2, 4000), (5000, 12345, 5000)):
        n = 2 ** 31 - 1
        values = sorted({0, n - 1} | {rng.randrange(n) for _ in range(pool)})[:max(pool, 1)] if pool > 1 else [n - 1]
        labels = [rng.choice(values) for _ in range(s)] if pool != s else list(range(100, 100 + s))
        weights = [rng.choice(WEIGHTS + (3, 0xFFFFFFFF)) for _ in range(s)]
        got = ask(harness, "tables", "".join(f"{head_place} {l} {w}\n" for l, w in zip(labels, weights)))
        total = {}
        for l, w in zip(labels, weights):
            total[l] = total.get(l, 0) + w
        assert got == [str(min(total[l], ref.SATURATED)) for l in labels], (s, head_place, pool)


def test_slots_and_keys_at_their_edges(harness):
    n = 2 ** 31 - 1
    members = [1, 2, 31, 32, 33, 64, 65, 1023, 1024, 1025, 2047, 2048]
    pairs = list(itertools.product([0, 1, 63, n - 1, 0x7FFFFFFF, 0x9E3779B1 & 0x7FFFFFFF], members))
    got = ask(harness, "slots", "".join(f"{l} {m}\n" for l, m in pairs))
    for (l, m), line in zip(pairs, got):
        slots, slot, tier = map(int, line.split())
        assert slots >= max(64, 2 * m) and slots & (slots - 1) == 0 and slots <= 4096 and (slots == 64 or slots < 4 * m), (l, m, line)
        assert 0 <= slot < slots
        assert tier == (0 if m == 1 else 1 if m <= 8 else 2 if m <= 64 else 3)
    assert [int(x.split()[2]) for x in ask(harness, "slots", "0 2049\n0 100000\n")] == [4, 4]
    triples = list(itertools.product([0, 1, 2048, 2 ** 31 - 2], [0, 1, n - 1], [2049, 4097, 10 ** 6, n]))
    got = ask(harness, "slots", "".join(f"{h} {l} {m}\n" for h, l, m in triples))
    keys = set()
    for (h, l, m), line in zip(triples, got):
        slots, slot, key = int(line.split()[0]), int(line.split()[1]), int(line.split()[2], 16)
        assert slots == 2 * m and 0 <= slot < slots
        assert key == (h << 32 | l) and key != 2 ** 64 - 1 and key >> 63 == 0
        keys.add(key)
    assert len(keys) == 12                                       # equal labels under different head places never meet
