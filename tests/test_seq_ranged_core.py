"""The rules of the ranged `--compare-seq` run (fastq-dupaway_amd/csrc/fqd_seq_range_core.hpp) on the CPU, in a harness built
with the sanitizers (tests/native/seq_range_check.cpp): the exact plan of the ranges against a brute-force plan on fuzzed
(key, bytes) lists, the prefix key against its definition, and — without a GPU — the validation of FQD_SEQ_RANGE_KB by the
CLI.  The device code that runs the same functions: tests/test_gpu_seq_ranged.py; the run: tests/test_seq_ranged_cli.py."""
import os
import random
import subprocess
from pathlib import Path

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "seq_range_check.cpp"
EXE = HERE / "native" / "seq_range_check"
CORE = HERE.parent / "fastq-dupaway_amd" / "csrc" / "fqd_seq_range_core.hpp"


def harness():
    if not EXE.exists() or EXE.stat().st_mtime < max(SRC.stat().st_mtime, CORE.stat().st_mtime):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-o", str(EXE), str(SRC)], check=True, capture_output=True)
    return str(EXE)


def native_plan(pairs, target):
    text = f"{len(pairs)} {target}\n" + "".join(f"{k} {b}\n" for k, b in pairs)
    r = subprocess.run([harness(), "plan"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tok = r.stdout.split()
    R = int(tok[0])
    rows = [tuple(int(x) for x in tok[1 + 4 * i: 5 + 4 * i]) for i in range(R)]
    return rows, [int(x) for x in tok[1 + 4 * R:]]


def brute_plan(pairs, target):
    """Key value by key value: a range takes the next key value while the bytes stay within the target; a key value that
    alone is beyond the target stands alone.  Returns the rows and every pair's range."""
    per_key = {}
    for k, b in pairs:
        c = per_key.setdefault(k, [0, 0])
        c[0] += 1; c[1] += b
    rows, cur = [], None
    for k in sorted(per_key):
        cnt, b = per_key[k]
        if cur is not None and cur[3] + b <= target:
            cur[1] = k; cur[2] += cnt; cur[3] += b
        else:
            if cur is not None:
                rows.append(tuple(cur))
            cur = [k, k, cnt, b]
    if cur is not None:
        rows.append(tuple(cur))
    where = {}
    for r, (lo, hi, _, _) in enumerate(rows):
        for k in per_key:
            if lo <= k <= hi:
                where[k] = r
    return rows, [where[k] for k, _ in pairs]


def fuzz_lists():
    rng = random.Random(20)
    yield [(5, 100)], 1000                                   # one pair
    yield [(5, 100)], 10                                     # one pair beyond the target
    yield [(7, 10)] * 50, 100                                # one key value beyond the target: alone, whole
    yield [(k, 10) for k in range(100)], 10 ** 9             # everything fits: one range
    yield [(k, 10) for k in range(100)], 1                   # nothing fits: every key value alone
    yield [(2 ** 64 - 1, 7), (0, 9), (2 ** 63, 3), (0, 1)], 10
    for _ in range(60):
        n = rng.choice([2, 3, 17, 200, 2000])
        keys = [rng.getrandbits(64) for _ in range(rng.choice([1, 2, 5, 40, n]))]
        if rng.random() < 0.3:
            keys = [k & ~0xFFFF | rng.randrange(4) for k in keys]        # key values next to each other
        pairs = [(rng.choice(keys), rng.choice([1, 40, 330, rng.randrange(1, 5000), 2 ** 32 - 1 if rng.random() < 0.02 else 7])) for _ in range(n)]
        total = sum(b for _, b in pairs)
        yield pairs, rng.choice([1, 330, 1000, max(1, total // 4), max(1, total // 50), total, total + 1])


@pytest.mark.parametrize("case", list(range(66)))
def test_plan_against_brute_force(case):
    pairs, target = list(fuzz_lists())[case]
    rows, range_of = native_plan(pairs, target)
    exp_rows, exp_range_of = brute_plan(pairs, target)
    per_key = {}
    for k, b in pairs:
        per_key[k] = per_key.get(k, 0) + b
    keys = sorted(per_key)
    # ranges cut only at key changes: the rows' key intervals are disjoint, ascending and cover every key value once
    assert all(lo <= hi for lo, hi, _, _ in rows)
    assert all(rows[i][1] < rows[i + 1][0] for i in range(len(rows) - 1))
    assert sum(c for _, _, c, _ in rows) == len(pairs) and sum(b for _, _, _, b in rows) == sum(b for _, b in pairs)
    for r, (lo, hi, cnt, b) in enumerate(rows):
        inside = [k for k in keys if lo <= k <= hi]
        assert inside and inside[0] == lo and inside[-1] == hi
        assert b == sum(per_key[k] for k in inside) and cnt == sum(1 for k, _ in pairs if lo <= k <= hi)
        # every multi-key range is within the target; an oversized one is a single key value
        assert b <= target or len(inside) == 1
        # maximal: the next key value would not have fitted
        if r + 1 < len(rows):
            assert b + per_key[rows[r + 1][0]] > target
    # the way back to input order
    assert all(rows[range_of[i]][0] <= k <= rows[range_of[i]][1] for i, (k, _) in enumerate(pairs))
    assert rows == exp_rows and range_of == exp_range_of


def test_prefix_key_and_the_word_test():
    rng = random.Random(4)
    seqs = [b"", b"A", b"ACGT", b"ACGTACG", b"ACGTACGT", b"ACGTACGTA", b"acgtnRYK" * 3, b"AC\x00T", b"ACGTACGTACG\x09TTTTT", b"\x0a" * 9, b"\xff" * 8 + b"\x01"]
    for _ in range(300):
        L = rng.randrange(0, 40)
        seqs.append(bytes(rng.choice([rng.randrange(256), rng.choice(b"ACGTN"), rng.choice(b"ACGTN")]) for _ in range(L)))
    text = "".join((s.hex() if s else "-") + "\n" for s in seqs)
    r = subprocess.run([harness(), "keys"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(seqs)
    for s, (key, low) in zip(seqs, got):
        assert key == int.from_bytes((s + b"\n" * 8)[:8], "big")
        assert low == int(any(c < 10 for c in s))
    # monotone in the sort order of the terminated strings when no byte is below '\n' (and none is '\n')
    clean = sorted({s for s in seqs if all(c > 10 for c in s)}, key=lambda s: s + b"\n")
    ks = [int.from_bytes((s + b"\n" * 8)[:8], "big") for s in clean]
    assert ks == sorted(ks)


# ---------------------------------------------------------------- the CLI's switch, without a GPU

@pytest.fixture(scope="module")
def exe():
    if not _lib.CLI_PATH.exists():
        fqd.build_native("all")
    return str(_lib.CLI_PATH)


@pytest.mark.parametrize("value", ["x", "0", "", "-3", "12k", "1.5"])
def test_range_switch_is_validated_before_any_gpu_call(exe, tmp_path, value):
    src = tmp_path / "in.fq"; src.write_bytes(b"@a\nACGT\n+\nIIII\n")
    out = tmp_path / "o.fq"
    r = subprocess.run([exe, "-i", str(src), "-o", str(out), "--compare-seq", "tight"], capture_output=True, text=True,
                       env=dict(os.environ, FQD_SEQ_RANGE_KB=value, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1
    assert "FQD_SEQ_RANGE_KB" in r.stderr and "positive integer" in r.stderr
    assert not out.exists() and not Path(str(out) + ".clusters").exists()
