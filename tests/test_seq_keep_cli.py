"""FQD_SEQ_KEEP=best of the `--compare-seq` modes through the CLI.  CPU part: the refusals that come before any GPU call.
GPU part: outputs, `.clusters` files and the `-v` line byte for byte against the restatement (tests/seq_keep_reference.py
on top of tests/seq_reference.py; both sorts are stable, so identical sequences have one defined order): SE and PE,
every mode, plain and `.gz` in and out; flat qualities give the default run's bytes; the ranged run (tight) gives the
in-core bytes and refuses loose and tail-hamming before any output exists."""
import gzip
import os
import random
import subprocess
from collections import Counter
from pathlib import Path

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib
import seq_reference as ref
import seq_keep_reference as keep


@pytest.fixture(scope="module")
def exe():
    if not _lib.CLI_PATH.exists():
        fqd.build_native("all")
    return str(_lib.CLI_PATH)


def run(exe, *args, env=None):
    e = dict(os.environ)
    e.pop("FQD_SEQ_KEEP", None)
    e.update(env or {})
    r = subprocess.run([exe, *map(str, args)], capture_output=True, env=e)
    r.stdout = r.stdout.decode("latin-1")
    r.stderr = r.stderr.decode("latin-1")
    return r


NO_GPU = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}


# ---------------------------------------------------------------- CPU: refused before any GPU call

@pytest.mark.parametrize("value", ["bogus", "", "BEST", "best ", "1"])
def test_unknown_value_is_refused(exe, tmp_path, value):
    src = tmp_path / "in.fq"; src.write_bytes(b"@a\nACGT\n+\nIIII\n")
    out = tmp_path / "o.fq"
    r = run(exe, "-i", src, "-o", out, "--compare-seq", "tight", "--write-clusters", env={**NO_GPU, "FQD_SEQ_KEEP": value})
    assert r.returncode == 1
    assert "FQD_SEQ_KEEP" in r.stderr and "'first' or 'best'" in r.stderr
    assert not out.exists() and not Path(str(out) + ".clusters").exists()


def test_best_with_fasta_is_refused(exe, tmp_path):
    src = tmp_path / "in.fa"; src.write_bytes(b">a\nACGT\n")
    out = tmp_path / "o.fa"
    r = run(exe, "-i", src, "-o", out, "--compare-seq", "loose", "--format", "fasta", env={**NO_GPU, "FQD_SEQ_KEEP": "best"})
    assert r.returncode == 1
    assert "FQD_SEQ_KEEP" in r.stderr and "fasta" in r.stderr
    assert not out.exists()


# ---------------------------------------------------------------- GPU

def make_reads(rng, n, flat=None, pool_size=40):
    """The read model of test_seq_cli.py (ragged lengths 0-200, prefixes, a few substitutions, many exact duplicates)
    with random qualities; flat: the one byte every quality line is made of."""
    alpha = "ACGTNacgtRYKMSWBDHV"
    pool = []
    for _ in range(pool_size):
        L = rng.choice([0, 1, 5, 20, 75, 150, 200, rng.randrange(0, 201)])
        pool.append("".join(rng.choice("ACGT" if rng.random() < 0.8 else alpha) for _ in range(L)))
    recs = []
    for k in range(n):
        s = rng.choice(pool)
        t = rng.random()
        if t < 0.25 and s:
            s = s[:rng.randrange(0, len(s) + 1)]
        elif t < 0.5 and s:
            s = list(s)
            for _ in range(rng.randrange(1, 4)):
                s[rng.randrange(len(s))] = rng.choice("ACGTN")
            s = "".join(s)
        lo = rng.choice([33, 33, 50, 70])                    # whole reads of low and of high quality, and ties among short ones
        q = flat * len(s) if flat else "".join(chr(rng.randrange(lo, lo + 8)) for _ in range(len(s)))
        recs.append(f"@r{k} x\n{s}\n+\n{q}\n".encode())
    return recs


def inputs(seed, paired, flat=None, n=2000):
    rng = random.Random(seed)
    files = [make_reads(rng, n, flat)]
    if paired:
        files.append(make_reads(rng, n, flat, pool_size=10))
    return [b"".join(f) for f in files]


def cli(exe, tmp_path, data, mode, d, gz=False, env=None, tag="a", clusters=True):
    ext = ".fq.gz" if gz else ".fq"
    ins = [tmp_path / f"in{tag}{k}{ext}" for k in range(len(data))]
    outs = [tmp_path / f"out{tag}{k}{ext}" for k in range(len(data))]
    for p, x in zip(ins, data):
        p.write_bytes(gzip.compress(x) if gz else x)
    args = ["-i", ins[0], "-o", outs[0]]
    if len(data) == 2:
        args += ["-u", ins[1], "-p", outs[1]]
    args += ["--compare-seq", mode, "--distance", d, "-v"]
    if clusters:
        args += ["--write-clusters"]
    return run(exe, *args, env=env), outs


def read_out(path):
    data = path.read_bytes()
    return gzip.decompress(data) if str(path).endswith(".gz") else data


MODES = [("tight", 2), ("loose", 2), ("tail-hamming", 0), ("tail-hamming", 2)]
CASES = [(paired, mode, d, gz) for paired in (False, True) for mode, d in MODES for gz in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{'pe' if c[0] else 'se'}-{c[1]}-d{c[2]}-{'gz' if c[3] else 'plain'}" for c in CASES])
def test_best_against_restatement(exe, tmp_path, case):
    paired, mode, d, gz = case
    data = inputs(100 + CASES.index(case), paired)
    r, outs = cli(exe, tmp_path, data, mode, d, gz=gz, env={"FQD_SEQ_KEEP": "best", "FQD_HOST_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    exp_out, exp_cl, total, dups, moved = keep.dedup_best(data, mode=ref.MODES[mode], distance=d)
    assert moved > 0                                         # the case is about something
    assert r.stdout == ref.verbose_line(total, dups, paired)
    assert f"sequence: best-quality pick, {moved} of {total - dups} clusters changed\n" in r.stderr
    for k, o in enumerate(outs):
        assert read_out(o) == exp_out[k]
        assert Path(str(o) + ".clusters").read_bytes() == exp_cl[k]
    # beside the default run: as many records; tight: the same sequences
    r0, outs0 = cli(exe, tmp_path, data, mode, d, gz=gz, tag="b")
    assert r0.returncode == 0, r0.stderr
    assert r0.stdout == r.stdout
    for o, o0 in zip(outs, outs0):
        got, default = ref.parse(read_out(o), False), ref.parse(read_out(o0), False)
        assert len(got) == len(default)
        if mode == "tight":
            assert Counter(x[2] for x in got) == Counter(x[2] for x in default)
            assert [x[2] for x in got] == [x[2] for x in default]
    assert any(read_out(o) != read_out(o0) for o, o0 in zip(outs, outs0))


@pytest.mark.gpu
@pytest.mark.parametrize("paired,mode,d,flat", [(False, "loose", 2, "!"), (True, "tight", 2, "I"), (True, "tail-hamming", 2, "I"), (False, "tight", 2, "!")])
def test_flat_qualities_give_the_default_bytes(exe, tmp_path, paired, mode, d, flat):
    # every member of a cluster scores the same: equal sequences (tight) and equal lengths (tail-hamming) under one
    # quality byte; for loose, whose members differ in length, under '!', which counts 0
    data = inputs(7, paired, flat=flat)
    r1, outs1 = cli(exe, tmp_path, data, mode, d, env={"FQD_SEQ_KEEP": "best", "FQD_HOST_TIMING": "1"}, tag="a")
    r0, outs0 = cli(exe, tmp_path, data, mode, d, env={"FQD_HOST_TIMING": "1"}, tag="b")
    rf, outsf = cli(exe, tmp_path, data, mode, d, env={"FQD_SEQ_KEEP": "first"}, tag="c")
    assert r1.returncode == 0 and r0.returncode == 0 and rf.returncode == 0, r1.stderr + r0.stderr + rf.stderr
    assert "best-quality pick, 0 of " in r1.stderr
    assert "best-quality pick" not in r0.stderr
    assert r1.stdout == r0.stdout == rf.stdout
    for a, b, c in zip(outs1, outs0, outsf):
        assert a.read_bytes() == b.read_bytes() == c.read_bytes()
        assert Path(str(a) + ".clusters").read_bytes() == Path(str(b) + ".clusters").read_bytes() == Path(str(c) + ".clusters").read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_ranged_tight_equals_in_core(exe, tmp_path, paired):
    data = inputs(21 + paired, paired)
    r1, outs1 = cli(exe, tmp_path, data, "tight", 2, env={"FQD_SEQ_KEEP": "best"}, tag="a")
    r2, outs2 = cli(exe, tmp_path, data, "tight", 2, env={"FQD_SEQ_KEEP": "best", "FQD_SEQ_RANGE_KB": "1", "FQD_HOST_TIMING": "1"}, tag="b")
    assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
    assert "ranged run" in r2.stderr
    exp_out, exp_cl, total, dups, moved = keep.dedup_best(data, mode=ref.TIGHT)
    assert moved > 0
    assert f"sequence: best-quality pick, {moved} of {total - dups} clusters changed\n" in r2.stderr
    assert r1.stdout == r2.stdout == ref.verbose_line(total, dups, paired)
    for k, (a, b) in enumerate(zip(outs1, outs2)):
        assert a.read_bytes() == b.read_bytes() == exp_out[k]
        assert Path(str(a) + ".clusters").read_bytes() == Path(str(b) + ".clusters").read_bytes() == exp_cl[k]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["loose", "tail-hamming"])
def test_ranged_loose_and_hamming_are_refused(exe, tmp_path, mode):
    data = inputs(30, True, n=200)
    r, outs = cli(exe, tmp_path, data, mode, 2, env={"FQD_SEQ_KEEP": "best", "FQD_SEQ_RANGE_KB": "1"})
    assert r.returncode == 1
    assert "FQD_SEQ_KEEP" in r.stderr and "FQD_SEQ_RANGE_KB" in r.stderr
    for o in outs:
        assert not o.exists() and not Path(str(o) + ".clusters").exists()
