"""FQD_FAST_KEEP=best and FQD_FAST_CLUSTERS=1 of the `--fast` mode through the CLI.  CPU part: the refusals that the
switches' values and the command line decide, before any GPU call.  GPU part: outputs, `.clusters` files and the `-v`
line byte for byte against the restatement (tests/fast_keep_reference.py), single-end and paired-end, plain, BGZF and
ordinary gzip in, plain and `.gz` out; flat qualities and FQD_FAST_KEEP=first give the default run's bytes; the inputs
the GPU-resident run cannot take are refused before any output exists."""
import gzip
import os
import random
import subprocess
from pathlib import Path

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib
import fast_keep_reference as fast
from inflate_cases import bgzf

SWITCHES = ("FQD_FAST_KEEP", "FQD_FAST_CLUSTERS", "FQD_ORDERED_RESIDENT", "FQD_DEVICES", "FQD_GUNZIP_DEVICE", "FQD_HOST_TIMING")
NO_GPU = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
BEST = {"FQD_FAST_KEEP": "best"}
CLUSTERS = {"FQD_FAST_CLUSTERS": "1"}


@pytest.fixture(scope="module")
def exe():
    if not _lib.CLI_PATH.exists():
        fqd.build_native("all")
    return str(_lib.CLI_PATH)


def run(exe, *args, env=None):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([exe, *map(str, args)], capture_output=True, env=e, timeout=120)
    r.stdout = r.stdout.decode("latin-1")
    r.stderr = r.stderr.decode("latin-1")
    return r


def verbose_line(total, dups, paired):
    return f"{total} {'read pairs' if paired else 'reads'} processed, out of which {dups} duplicates were removed.\n"


def make_reads(rng, n, flat=None, pool_size=None, fasta=False, tag="r"):
    """Reads of ragged lengths over a pool (many exact duplicates, clusters of 1 to dozens), random qualities whose level
    differs read by read; flat: the one byte every quality line is made of."""
    pool = ["".join(rng.choice("ACGTN" if rng.random() < 0.1 else "ACGT") for _ in range(rng.choice([1, 20, 75, 150, 150, 200])))
            for _ in range(pool_size or max(2, n // 3))]
    recs = []
    for k in range(n):
        s = rng.choice(pool)
        if fasta:
            recs.append(f">{tag}{k} x\n{s}\n".encode())
            continue
        lo = rng.choice([33, 40, 60, 70])
        q = flat * len(s) if flat else "".join(chr(rng.randrange(lo, lo + 6)) for _ in range(len(s)))
        recs.append(f"@{tag}{k} x\n{s}\n+\n{q}\n".encode())
    return recs


def inputs(seed, paired, n=2000, flat=None, fasta=False):
    rng = random.Random(seed)
    files = [make_reads(rng, n, flat, fasta=fasta, tag="a")]
    if paired:
        files.append(make_reads(rng, n, flat, pool_size=6, fasta=fasta, tag="b"))
    return [b"".join(f) for f in files]


PACK = {"plain": lambda x: x, "bgzf": bgzf, "gzip": gzip.compress}


def cli(exe, tmp_path, data, kind="plain", gz_out=False, env=None, tag="a", extra=(), fasta=False):
    ext = ".fa" if fasta else ".fq"
    ins = [tmp_path / f"in{tag}{k}{ext}{'' if kind == 'plain' else '.gz'}" for k in range(len(data))]
    outs = [tmp_path / f"out{tag}{k}{ext}{'.gz' if gz_out else ''}" for k in range(len(data))]
    for p, x in zip(ins, data):
        p.write_bytes(PACK[kind](x))
    args = ["-i", ins[0], "-o", outs[0]]
    if len(data) == 2:
        args += ["-u", ins[1], "-p", outs[1]]
    args += ["--fast", "-v", *extra]
    if fasta:
        args += ["--format", "fasta"]
    return run(exe, *args, env=env), outs


def read_out(path):
    data = path.read_bytes()
    return gzip.decompress(data) if str(path).endswith(".gz") else data


def clusters_of(path):
    return Path(str(path) + ".clusters")


def nothing_written(outs):
    return all(not o.exists() and not clusters_of(o).exists() for o in outs)


# ---------------------------------------------------------------- CPU: refused before any GPU call

@pytest.mark.parametrize("value", ["bogus", "", "BEST", "best ", "1"])
def test_unknown_value_is_refused(exe, tmp_path, value):
    r, outs = cli(exe, tmp_path, inputs(1, False, n=4), env={**NO_GPU, "FQD_FAST_KEEP": value})
    assert r.returncode == 1
    assert "FQD_FAST_KEEP" in r.stderr and "'first' or 'best'" in r.stderr
    assert nothing_written(outs)


@pytest.mark.parametrize("env", [BEST, CLUSTERS, {**BEST, **CLUSTERS}], ids=["best", "clusters", "both"])
def test_unordered_is_refused(exe, tmp_path, env):
    r, outs = cli(exe, tmp_path, inputs(2, True, n=4), env={**NO_GPU, **env}, extra=["--unordered"])
    assert r.returncode == 1
    assert all(k in r.stderr for k in env) and "--unordered" in r.stderr
    assert nothing_written(outs)


@pytest.mark.parametrize("env", [BEST, CLUSTERS], ids=["best", "clusters"])
def test_several_devices_are_refused(exe, tmp_path, env):
    r, outs = cli(exe, tmp_path, inputs(3, False, n=4), env={**NO_GPU, **env, "FQD_DEVICES": "0,1"})
    assert r.returncode == 1
    assert all(k in r.stderr for k in env) and "FQD_DEVICES" in r.stderr
    assert nothing_written(outs)


def test_best_with_fasta_is_refused(exe, tmp_path):
    r, outs = cli(exe, tmp_path, inputs(4, False, n=4, fasta=True), env={**NO_GPU, **BEST}, fasta=True)
    assert r.returncode == 1
    assert "FQD_FAST_KEEP" in r.stderr and "fasta" in r.stderr
    assert nothing_written(outs)


@pytest.mark.parametrize("env", [BEST, CLUSTERS], ids=["best", "clusters"])
def test_resident_run_turned_off_is_refused(exe, tmp_path, env):
    r, outs = cli(exe, tmp_path, inputs(5, False, n=4), env={**NO_GPU, **env, "FQD_ORDERED_RESIDENT": "0"})
    assert r.returncode == 1
    assert all(k in r.stderr for k in env) and "FQD_ORDERED_RESIDENT" in r.stderr
    assert nothing_written(outs)


def test_a_compare_seq_run_does_not_look_at_the_switches(exe, tmp_path):
    # a value that `--fast` refuses: the sequence-based run gets as far as the GPU it does not have
    src = tmp_path / "in.fq"; src.write_bytes(inputs(6, False, n=4)[0])
    r = run(exe, "-i", src, "-o", tmp_path / "o.fq", "--compare-seq", "tight", env={**NO_GPU, "FQD_FAST_KEEP": "bogus", "FQD_FAST_CLUSTERS": "1"})
    assert "FQD_FAST_KEEP" not in r.stderr and "FQD_FAST_CLUSTERS" not in r.stderr


# ---------------------------------------------------------------- GPU

CASES = [(paired, kind, gz_out) for paired in (False, True) for kind, gz_out in (("plain", False), ("bgzf", True), ("gzip", True), ("plain", True))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{'pe' if c[0] else 'se'}-{c[1]}-to-{'gz' if c[2] else 'plain'}" for c in CASES])
def test_best_and_clusters_against_restatement(exe, tmp_path, case):
    paired, kind, gz_out = case
    data = inputs(100 + CASES.index(case), paired)
    exp_out, exp_cl, total, dups, moved = fast.dedup(data, best=True)
    first_out, first_cl, _, _, _ = fast.dedup(data, best=False)
    assert moved > 0 and dups > 0 and exp_out != first_out  # the case is about something
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**BEST, **CLUSTERS, "FQD_HOST_TIMING": "1"}, tag="a")
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    assert f"fast: best-quality pick, {moved} of {total - dups} clusters changed\n" in r.stderr
    for k, o in enumerate(outs):
        assert read_out(o) == exp_out[k]
        assert clusters_of(o).read_bytes() == exp_cl[k]
    # the default run: the reference's first occurrences, the same -v line, no cluster file
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, tag="b")
    assert r0.returncode == 0, r0.stderr
    assert r0.stdout == r.stdout
    for k, o in enumerate(outs0):
        assert read_out(o) == first_out[k]
        assert not clusters_of(o).exists()
    # clusters without best: the default output's bytes, the first member written
    rc, outsc = cli(exe, tmp_path, data, kind, gz_out, env={**CLUSTERS, "FQD_HOST_TIMING": "1"}, tag="c")
    assert rc.returncode == 0, rc.stderr
    assert rc.stdout == r.stdout and "best-quality pick" not in rc.stderr
    for k, (o, o0) in enumerate(zip(outsc, outs0)):
        assert o.read_bytes() == o0.read_bytes()
        assert clusters_of(o).read_bytes() == first_cl[k]
    # best without clusters
    rb, outsb = cli(exe, tmp_path, data, kind, gz_out, env=BEST, tag="d")
    assert rb.returncode == 0, rb.stderr
    for k, o in enumerate(outsb):
        assert read_out(o) == exp_out[k]
        assert not clusters_of(o).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("paired,kind,gz_out", [(False, "plain", False), (True, "bgzf", True)])
def test_flat_qualities_and_first_give_the_default_bytes(exe, tmp_path, paired, kind, gz_out):
    # every member of a cluster has the same sequence, so under one quality byte the same score: the first stays
    data = inputs(7, paired, flat="I")
    r1, outs1 = cli(exe, tmp_path, data, kind, gz_out, env={**BEST, "FQD_HOST_TIMING": "1"}, tag="a")
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, env={"FQD_HOST_TIMING": "1"}, tag="b")
    rf, outsf = cli(exe, tmp_path, data, kind, gz_out, env={"FQD_FAST_KEEP": "first"}, tag="c")
    assert r1.returncode == 0 and r0.returncode == 0 and rf.returncode == 0, r1.stderr + r0.stderr + rf.stderr
    assert "best-quality pick, 0 of " in r1.stderr
    assert "best-quality pick" not in r0.stderr
    assert r1.stdout == r0.stdout == rf.stdout
    for a, b, c in zip(outs1, outs0, outsf):
        assert a.read_bytes() == b.read_bytes() == c.read_bytes()
        assert not clusters_of(c).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_fasta_with_clusters(exe, tmp_path, paired):
    data = inputs(8, paired, n=500, fasta=True)
    exp_out, exp_cl, total, dups, _ = fast.dedup(data, fasta=True)
    r, outs = cli(exe, tmp_path, data, env=CLUSTERS, fasta=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    for k, o in enumerate(outs):
        assert o.read_bytes() == exp_out[k]
        assert clusters_of(o).read_bytes() == exp_cl[k]


@pytest.mark.gpu
def test_one_named_device_is_taken(exe, tmp_path):
    data = inputs(9, False, n=200)
    exp_out, exp_cl, total, dups, _ = fast.dedup(data, best=True)
    r, outs = cli(exe, tmp_path, data, env={**BEST, **CLUSTERS, "FQD_DEVICES": "0"})
    assert r.returncode == 0, r.stderr
    assert outs[0].read_bytes() == exp_out[0] and clusters_of(outs[0]).read_bytes() == exp_cl[0]


def irregular_inputs():
    good = inputs(10, False, n=200)[0]
    yield "malformed record", good + b"@tail\nACGT\n+\n", "well-formed"
    at = good.index(b"\n") + 1                               # the first base of the first record
    yield "byte outside ACGTN", good[:at] + b"R" + good[at + 1:], "unknown character"


@pytest.mark.gpu
@pytest.mark.parametrize("env", [BEST, CLUSTERS], ids=["best", "clusters"])
@pytest.mark.parametrize("what", [c[0] for c in irregular_inputs()])
def test_inputs_the_resident_run_cannot_take_are_refused(exe, tmp_path, what, env):
    _, text, words = next(c for c in irregular_inputs() if c[0] == what)
    r, outs = cli(exe, tmp_path, [text], env=env)
    assert r.returncode == 1
    assert all(k in r.stderr for k in env) and words in r.stderr
    assert nothing_written(outs)
    # the default run takes the same input to the streaming run and creates its output
    r0, outs0 = cli(exe, tmp_path, [text], tag="b")
    assert outs0[0].exists()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [BEST, CLUSTERS, {**BEST, **CLUSTERS}], ids=["best", "clusters", "both"])
def test_an_empty_file_gives_what_the_default_run_gives(exe, tmp_path, env):
    # no record, no cluster: the default run's result and, with clusters, an empty cluster file
    r0, outs0 = cli(exe, tmp_path, [b""], tag="b")
    r, outs = cli(exe, tmp_path, [b""], env=env)
    assert (r.returncode, r.stdout, r.stderr) == (r0.returncode, r0.stdout, r0.stderr)
    assert outs[0].exists() == outs0[0].exists()
    if outs0[0].exists():
        assert outs[0].read_bytes() == outs0[0].read_bytes()
    if r0.returncode == 0 and "FQD_FAST_CLUSTERS" in env:
        assert clusters_of(outs[0]).read_bytes() == b""
    else:
        assert not clusters_of(outs[0]).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [BEST, CLUSTERS], ids=["best", "clusters"])
def test_a_pipe_is_refused(exe, tmp_path, env):
    fifo = tmp_path / "in.fq"
    os.mkfifo(fifo)
    out = tmp_path / "o.fq"
    r = run(exe, "-i", fifo, "-o", out, "--fast", env=env)     # refused on the file's type: the pipe is never opened
    assert r.returncode == 1
    assert all(k in r.stderr for k in env) and "not a regular file" in r.stderr
    assert not out.exists() and not clusters_of(out).exists()


@pytest.mark.gpu
def test_pairs_of_unequal_count_are_refused(exe, tmp_path):
    a, b = inputs(11, True, n=200)
    r, outs = cli(exe, tmp_path, [a, b + b"@extra\nACGT\n+\nIIII\n"], env=BEST)
    assert r.returncode == 1
    assert "FQD_FAST_KEEP" in r.stderr and "different numbers of records" in r.stderr
    assert nothing_written(outs)
