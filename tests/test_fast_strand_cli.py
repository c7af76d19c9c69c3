"""FQD_FAST_STRAND=both of the `--fast` mode through the CLI.  CPU part: what the switch's value and the command line
decide, before any GPU call.  GPU part: on small FASTQ and FASTA inputs — plain, BGZF and ordinary gzip, single-end and
paired, with hand-placed strand-duplicates before and after their partner — the outputs are the ORIGINAL text of the
records tests/strand_reference.py keeps, the `-v` line matches, the cluster files list the turned members, the
best-quality copy of a mixed-strand cluster is written at its own place (tests/fast_keep_reference.py fed canonical keys);
the reference's fixtures, which hold no turned copy, give their expected files; `given` and an unset switch give the
default run's bytes; the inputs the GPU-resident run cannot take are refused before any output exists."""
import gzip
import os
import random
import subprocess
from pathlib import Path

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib
import fast_keep_reference as fast
import strand_reference as ref
from inflate_cases import bgzf

SWITCHES = ("FQD_FAST_STRAND", "FQD_FAST_KEEP", "FQD_FAST_CLUSTERS", "FQD_ORDERED_RESIDENT", "FQD_DEVICES", "FQD_GUNZIP_DEVICE", "FQD_HOST_TIMING")
NO_GPU = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
BOTH = {"FQD_FAST_STRAND": "both"}
FIXTURES = Path(__file__).resolve().parent / "golden" / "reference_fixtures"


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


def rand_seq(rng, L):
    return "".join(rng.choice("ACGTN" if rng.random() < 0.1 else "ACGT") for _ in range(L)).encode()


def fragments(seed, paired, n=600):
    """[(mate 1, mate 2 or None)] in input order.  The first records are placed by hand: a read and then its turned copy,
    a turned copy and then its original, a read that is its own reverse complement twice, an exact copy; the rest draw
    from a pool, every second draw turned."""
    rng = random.Random(seed)

    def turn(f):
        return (f[1], f[0]) if paired else (ref.rc(f[0]), None)

    def fresh(L=None):
        return (rand_seq(rng, L or rng.choice([1, 20, 75, 150, 150, 200])), rand_seq(rng, rng.choice([1, 30, 150])) if paired else None)

    p = [fresh(150), fresh(151), fresh(33), fresh(16)]
    own = (b"ACGT" * 10, b"ACGT" * 10) if paired else (b"ACGTTGCA" + b"N" + b"TGCAACGT", None)
    out = [p[0], turn(p[0]), turn(p[1]), p[2], p[1], own, turn(own), p[2], turn(p[3]), turn(p[3]), p[3]]
    pool = [fresh() for _ in range(n // 3)]
    while len(out) < n:
        f = rng.choice(pool)
        out.append(turn(f) if rng.random() < 0.5 else f)
    out.append(turn(p[0]))                                      # and one far behind its partner
    return out


def as_text(frags, fasta, flat=None, seed=0):
    """The files' bytes: one per mate."""
    rng = random.Random(seed)
    files = []
    for m in range(2 if frags[0][1] is not None else 1):
        recs = []
        for k, f in enumerate(frags):
            s = f[m].decode()
            if fasta:
                recs.append(f">{'ab'[m]}{k} x\n{s}\n")
                continue
            lo = rng.choice([33, 40, 60, 70])
            q = flat * len(s) if flat else "".join(chr(rng.randrange(lo, lo + 6)) for _ in range(len(s)))
            recs.append(f"@{'ab'[m]}{k} x\n{s}\n+\n{q}\n")
        files.append("".join(recs).encode())
    return files


def restate(inputs, fasta=False, best=False):
    """tests/fast_keep_reference.py's dedup with the clusters taken over CANONICAL keys: (outputs, cluster files, total,
    duplicates, clusters whose written member changed)."""
    files = [fast.parse(x, fasta) for x in inputs]
    n = len(files[0])
    records = [files[0][i][2] if len(files) == 1 else (files[0][i][2], files[1][i][2]) for i in range(n)]
    groups = fast.clusters_of([ref.canon_key(r) for r in records])
    scores = [min(fast.SAT, sum(fast.score(f[i][0]) for f in files)) for i in range(n)]
    written, moved, listing = set(), 0, []
    for g in groups:
        w = fast.pick(g, scores) if best else g[0]
        moved += w != g[0]
        written.add(w)
        order = list(g)
        at = order.index(w)
        order[0], order[at] = order[at], order[0]
        listing.append(order)
    if not best:
        keep = ref.expected_keep(records)
        assert written == {i for i in range(n) if keep[i]}
    outputs = [b"".join(f[i][0] for i in range(n) if i in written) for f in files]
    cluster_files = [b"".join((b"" if k == 0 else b"--") + f[i][1] for order in listing for k, i in enumerate(order)) for f in files]
    return outputs, cluster_files, n, n - len(groups), moved


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


# ---------------------------------------------------------------- CPU: decided before any GPU call

@pytest.mark.parametrize("value", ["sideways", "", "BOTH", "both ", "1"])
def test_unknown_value_is_refused(exe, tmp_path, value):
    r, outs = cli(exe, tmp_path, as_text(fragments(1, False, n=12), False), env={**NO_GPU, "FQD_FAST_STRAND": value})
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_STRAND") == 1 and "'given' or 'both'" in r.stderr
    assert nothing_written(outs)


def test_unordered_is_refused(exe, tmp_path):
    r, outs = cli(exe, tmp_path, as_text(fragments(2, True, n=12), False), env={**NO_GPU, **BOTH}, extra=["--unordered"])
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_STRAND") == 1 and "--unordered" in r.stderr
    assert nothing_written(outs)


def test_several_devices_are_refused(exe, tmp_path):
    r, outs = cli(exe, tmp_path, as_text(fragments(3, False, n=12), False), env={**NO_GPU, **BOTH, "FQD_DEVICES": "0,1"})
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_STRAND") == 1 and "FQD_DEVICES" in r.stderr
    assert nothing_written(outs)


def test_resident_run_turned_off_is_refused(exe, tmp_path):
    r, outs = cli(exe, tmp_path, as_text(fragments(4, False, n=12), False), env={**NO_GPU, **BOTH, "FQD_ORDERED_RESIDENT": "0"})
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_STRAND") == 1 and "FQD_ORDERED_RESIDENT" in r.stderr
    assert nothing_written(outs)


@pytest.mark.gpu
def test_a_compare_seq_run_does_not_look_at_the_switch(exe, tmp_path):
    # a value that `--fast` refuses: the sequence-based run goes through, and turned copies stay (it compares given bytes)
    data = as_text(fragments(5, False, n=40), False)[0]
    src = tmp_path / "in.fq"; src.write_bytes(data)
    outs = []
    for tag, env in (("a", {"FQD_FAST_STRAND": "sideways"}), ("b", BOTH), ("c", {})):
        out = tmp_path / f"o{tag}.fq"
        r = run(exe, "-i", src, "-o", out, "--compare-seq", "tight", "-v", env=env)
        assert r.returncode == 0, r.stderr
        assert "FQD_FAST_STRAND" not in r.stderr and "both strands" not in r.stderr
        outs.append((r.stdout, out.read_bytes()))
    assert outs[0] == outs[1] == outs[2]


def test_the_fixtures_hold_no_turned_copy():
    # what makes their expected files the expected files of FQD_FAST_STRAND=both as well
    for names in (["single_fast.fa"], ["paired_fast_r1.fa", "paired_fast_r2.fa"]):
        data = [(FIXTURES / "inputs" / x).read_bytes() for x in names]
        outs, _, _, _, _ = restate(data, fasta=True)
        assert outs == [(FIXTURES / "expected" / x).read_bytes() for x in names]


# ---------------------------------------------------------------- GPU

CASES = [(paired, fasta, kind, gz_out) for paired in (False, True) for fasta in (False, True)
         for kind, gz_out in (("plain", False), ("bgzf", True), ("gzip", False))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{'pe' if c[0] else 'se'}-{'fasta' if c[1] else 'fastq'}-{c[2]}-to-{'gz' if c[3] else 'plain'}" for c in CASES])
def test_outputs_clusters_and_the_verbose_line(exe, tmp_path, case):
    paired, fasta, kind, gz_out = case
    frags = fragments(100 + CASES.index(case), paired)
    data = as_text(frags, fasta, seed=CASES.index(case))
    exp_out, exp_cl, total, dups, _ = restate(data, fasta)
    plain_out, _, _, plain_dups, _ = fast.dedup(data, fasta)
    assert dups > plain_dups > 0                                # turned copies AND exact ones
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**BOTH, "FQD_HOST_TIMING": "1"}, fasta=fasta)
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    turned = sum(ref.canon_pe(*f)[1] if paired else ref.canon_se(f[0])[1] for f in frags)
    assert f"fast: both strands, {turned} of {total} records turned\n" in r.stderr
    for k, o in enumerate(outs):
        assert read_out(o) == exp_out[k]                        # original text, never a turned read
        assert not clusters_of(o).exists()
    # with the cluster files: the same outputs, the turned members listed under the record that is written
    rc_, outsc = cli(exe, tmp_path, data, kind, gz_out, env={**BOTH, "FQD_FAST_CLUSTERS": "1"}, tag="c", fasta=fasta)
    assert rc_.returncode == 0, rc_.stderr
    assert rc_.stdout == r.stdout
    for k, o in enumerate(outsc):
        assert read_out(o) == exp_out[k]
        assert clusters_of(o).read_bytes() == exp_cl[k]


@pytest.mark.gpu
@pytest.mark.parametrize("paired,fasta,kind,gz_out", [(False, False, "plain", False), (True, False, "bgzf", True), (False, True, "gzip", False)])
def test_given_and_an_unset_switch_give_the_default_bytes(exe, tmp_path, paired, fasta, kind, gz_out):
    data = as_text(fragments(50 + int(paired), paired), fasta, seed=1)
    plain_out, _, total, plain_dups, _ = fast.dedup(data, fasta)
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, tag="d", fasta=fasta)
    rg, outsg = cli(exe, tmp_path, data, kind, gz_out, env={"FQD_FAST_STRAND": "given", "FQD_HOST_TIMING": "1"}, tag="g", fasta=fasta)
    assert r0.returncode == 0 and rg.returncode == 0, r0.stderr + rg.stderr
    assert r0.stdout == rg.stdout == verbose_line(total, plain_dups, paired)
    assert "both strands" not in rg.stderr
    for k, (a, b) in enumerate(zip(outs0, outsg)):
        assert a.read_bytes() == b.read_bytes()
        assert read_out(a) == plain_out[k]


@pytest.mark.gpu
@pytest.mark.parametrize("paired,kind,gz_out", [(False, "plain", False), (True, "bgzf", True), (False, "gzip", True)])
def test_best_copy_of_a_mixed_strand_cluster(exe, tmp_path, paired, kind, gz_out):
    data = as_text(fragments(7 + int(paired), paired), False, seed=3)
    exp_out, exp_cl, total, dups, moved = restate(data, best=True)
    first_out, _, _, _, _ = restate(data)
    assert moved > 0 and exp_out != first_out
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**BOTH, "FQD_FAST_KEEP": "best", "FQD_FAST_CLUSTERS": "1", "FQD_HOST_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    assert f"fast: best-quality pick, {moved} of {total - dups} clusters changed\n" in r.stderr
    for k, o in enumerate(outs):
        assert read_out(o) == exp_out[k]
        assert clusters_of(o).read_bytes() == exp_cl[k]


@pytest.mark.gpu
@pytest.mark.parametrize("names", [["single_fast.fa"], ["paired_fast_r1.fa", "paired_fast_r2.fa"]], ids=["single_fast", "paired_fast"])
def test_reference_fixtures_give_their_expected_files(exe, tmp_path, names):
    data = [(FIXTURES / "inputs" / x).read_bytes() for x in names]
    r, outs = cli(exe, tmp_path, data, env=BOTH, fasta=True)
    assert r.returncode == 0, r.stderr
    for o, x in zip(outs, names):
        assert o.read_bytes() == (FIXTURES / "expected" / x).read_bytes()


@pytest.mark.gpu
def test_a_pipe_is_refused(exe, tmp_path):
    fifo = tmp_path / "in.fq"
    os.mkfifo(fifo)
    out = tmp_path / "o.fq"
    r = run(exe, "-i", fifo, "-o", out, "--fast", env=BOTH)    # refused on the file's type: the pipe is never opened
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_STRAND") == 1 and "not a regular file" in r.stderr
    assert not out.exists()


@pytest.mark.gpu
def test_a_bad_base_is_refused(exe, tmp_path):
    good = as_text(fragments(11, False, n=200), False)[0]
    at = good.index(b"\n") + 1                                 # the first base of the first record
    r, outs = cli(exe, tmp_path, [good[:at] + b"R" + good[at + 1:]], env=BOTH)
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_STRAND") == 1 and "unknown character" in r.stderr
    assert nothing_written(outs)
