"""FQD_FAST_UMI_MISMATCH=0|1|2 of the `--fast` mode through the CLI.  CPU part: what the switch's value, FQD_FAST_UMI and the
command line decide, before any GPU call.  GPU part: on small files of molecules x PCR copies x UMI errors — FASTQ and FASTA,
plain, BGZF and ordinary gzip, single-end and paired, colon and underscore, single and dual UMIs — the outputs, the cluster
files, the `;size=N` labels, the duplication-level table and the `-v` line are those of tests/size_reference.py fed the merged
clusters of the sequential statement (tests/umi_merge_reference.py), alone and with each of FQD_FAST_KEEP=best,
FQD_FAST_CLUSTERS, FQD_FAST_STRAND=both, FQD_FAST_SIZEOUT and FQD_FAST_LEVELS; 0 and an unset switch give the files of the
FQD_FAST_UMI-only run byte for byte; a file without UMI errors gives the same output with 1 as with 0; a sequence under more
UMIs than the limit ends the run before any output exists."""
import gzip
import os
import random
import subprocess
from pathlib import Path

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib
import fast_keep_reference as fast
import size_reference as sized
import strand_reference as strand
import umi_merge_reference as mref
import umi_reference as umi
from inflate_cases import bgzf
from umi_merge_cases import hamming

SWITCHES = ("FQD_FAST_UMI", "FQD_FAST_UMI_MISMATCH", "FQD_FAST_STRAND", "FQD_FAST_KEEP", "FQD_FAST_CLUSTERS", "FQD_FAST_SIZEOUT", "FQD_FAST_LEVELS",
            "FQD_ORDERED_RESIDENT", "FQD_DEVICES", "FQD_GUNZIP_DEVICE", "FQD_HOST_TIMING")
NO_GPU = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
MODE = {"colon": b":", "underscore": b"_"}
PACK = {"plain": lambda x: x, "bgzf": bgzf, "gzip": gzip.compress}
MAX_GROUP_AT_LEAST = 4096                                      # the issue's floor; the GPU tests read the library's value


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


def rand_seq(rng, L, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(L)).encode()


def with_error(rng, u):
    """One base of the UMI field changed (never a joiner)."""
    places = [p for p, c in enumerate(u) if c not in b"+-_"]
    p = rng.choice(places)
    return u[:p] + bytes([rng.choice([c for c in b"ACGTN" if c != u[p]])]) + u[p + 1:]


def library(seed, paired, n_molecules=120, dual=False, error=0.12, turned=False, far_apart=False):
    """[(UMI field, mate 1, mate 2 or None)] in shuffled order: molecules (a UMI on one of a few fragments, so that a fragment
    carries several UMIs) x 1 .. 9 PCR copies, a copy's UMI with one wrong base at rate `error`.  far_apart: the UMIs come
    from a pool whose members differ in three bases at least."""
    rng = random.Random(seed)
    frags = [(rand_seq(rng, rng.choice([20, 75, 150, 151])), rand_seq(rng, rng.choice([30, 150])) if paired else None) for _ in range(n_molecules // 6)]
    fresh = (lambda: rand_seq(rng, 3) + b"+" + rand_seq(rng, 3)) if dual else (lambda: rand_seq(rng, 6))
    pool = []
    while far_apart and len(pool) < 40:
        u = fresh()
        if all(hamming(u, v) >= 3 for v in pool):
            pool.append(u)
    out = []
    for _ in range(n_molecules):
        u, f = (rng.choice(pool) if far_apart else fresh()), rng.choice(frags)
        for _ in range(rng.choice([1, 1, 2, 3, 5, 9])):
            g = f
            if turned and rng.random() < 0.5:
                g = (f[1], f[0]) if paired else (strand.rc(f[0]), None)
            out.append((with_error(rng, u) if rng.random() < error else u, *g))
    rng.shuffle(out)
    return out


def id_line(k, u, mode, fasta, mate):
    lead = ">" if fasta else "@"
    if mode == "colon":
        return f"{lead}A00:7:FC_1:{k}:{u.decode()} {mate + 1}:N:0:ATCACG\n"
    return f"{lead}r{k}:x_y_{u.decode()}\tmate_{mate + 1}\n"


def as_text(mols, mode, fasta=False, seed=0):
    rng = random.Random(seed)
    files = []
    for m in range(2 if mols[0][2] is not None else 1):
        recs = []
        for k, (u, *mates) in enumerate(mols):
            s = mates[m].decode()
            if fasta:
                recs.append(f"{id_line(k, u, mode, fasta, m)}{s}\n")
                continue
            lo = rng.choice([33, 40, 60, 70])
            recs.append(f"{id_line(k, u, mode, fasta, m)}{s}\n+\n{''.join(chr(rng.randrange(lo, lo + 6)) for _ in s)}\n")
        files.append("".join(recs).encode())
    return files


def statement(inputs, mode, D, fasta=False, best=False, both=False, max_group=1 << 30):
    """(outputs with labels, `.duplevels` text, total, duplicates, plain outputs, cluster files, the merge's info)."""
    files = [fast.parse(x, fasta) for x in inputs]
    umis, keys = [], []
    for i in range(len(files[0])):
        seqs = tuple(f[i][2] for f in files)
        if both:
            c = strand.canon_key(seqs[0] if len(seqs) == 1 else seqs)
            seqs = (c,) if len(files) == 1 else tuple(c)
        _, u = umi.umi_of(files[0][i][1], MODE[mode])
        umis.append(umi.bases(u))
        keys.append(seqs)
    if D == 0:
        owner, info = list(zip(umis, keys)), None
    else:
        owner, info, *_ = mref.merge(umis, keys, D, max_group)
        owner = [int(o) for o in owner]
    return (*sized.dedup_sized(inputs, fasta, best, keys=owner), info)


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


def beside(path, ext):
    return Path(str(path) + ext)


def nothing_written(outs):
    return all(not o.exists() and not beside(o, ".clusters").exists() and not beside(o, ".duplevels").exists() for o in outs)


def switches(mode, D, **more):
    return {"FQD_FAST_UMI": mode, "FQD_FAST_UMI_MISMATCH": str(D), **more}


# ---------------------------------------------------------------- CPU: decided before any GPU call

@pytest.mark.parametrize("value", ["3", "-1", "", "one", "1 ", "01", "2.0"])
def test_unknown_value_is_refused(exe, tmp_path, value):
    r, outs = cli(exe, tmp_path, as_text(library(1, False, 6), "colon"), env={**NO_GPU, **switches("colon", value)})
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_UMI_MISMATCH") == 1 and "must be 0, 1 or 2" in r.stderr
    assert nothing_written(outs)


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("other", [None, "off"])
def test_the_switch_without_fast_umi_is_refused(exe, tmp_path, D, other):
    env = {**NO_GPU, "FQD_FAST_UMI_MISMATCH": str(D), **({"FQD_FAST_UMI": other} if other else {})}
    r, outs = cli(exe, tmp_path, as_text(library(2, False, 6), "colon"), env=env)
    assert r.returncode == 1
    assert f"FQD_FAST_UMI_MISMATCH={D}" in r.stderr and "FQD_FAST_UMI=colon" in r.stderr and "FQD_FAST_UMI=underscore" in r.stderr
    assert nothing_written(outs)


def test_unordered_is_refused(exe, tmp_path):
    r, outs = cli(exe, tmp_path, as_text(library(3, True, 6), "colon"), env={**NO_GPU, **switches("colon", 1)}, extra=["--unordered"])
    assert r.returncode == 1
    assert "FQD_FAST_UMI=colon and FQD_FAST_UMI_MISMATCH=1" in r.stderr and "--unordered" in r.stderr
    assert nothing_written(outs)


def test_several_devices_are_refused(exe, tmp_path):
    r, outs = cli(exe, tmp_path, as_text(library(4, False, 6), "colon"), env={**NO_GPU, **switches("colon", 2), "FQD_DEVICES": "0,1"})
    assert r.returncode == 1
    assert "FQD_FAST_UMI_MISMATCH=2" in r.stderr and "FQD_DEVICES" in r.stderr
    assert nothing_written(outs)


def test_the_statement_merges_what_the_exact_run_keeps_apart():
    # of the yardstick: a library with UMI errors has fewer molecules under the rule, one without has the same
    data = as_text(library(5, False), "colon")
    exact, merged1, merged2 = (statement(data, "colon", D) for D in (0, 1, 2))
    assert exact[3] < merged1[3] <= merged2[3]
    clean = as_text(library(6, True, far_apart=True, error=0), "underscore")
    assert statement(clean, "underscore", 0)[:6] == statement(clean, "underscore", 1)[:6]


# ---------------------------------------------------------------- GPU

SHAPES = [(False, False, "plain", False, "colon", 1, False), (True, False, "bgzf", True, "underscore", 2, True), (False, True, "gzip", False, "colon", 1, True),
          (True, True, "plain", False, "underscore", 1, False)]
OPTIONS = ["alone", "best", "clusters", "both", "sizeout", "levels"]
CASES = [(s, o) for s in SHAPES for o in OPTIONS if not (o == "best" and s[1])]          # (FQD_FAST_KEEP=best needs quality lines)


def case_id(c):
    s, o = c
    return f"{'pe' if s[0] else 'se'}-{'fasta' if s[1] else 'fastq'}-{s[2]}-to-{'gz' if s[3] else 'plain'}-{s[4]}-D{s[5]}-{o}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_outputs_against_the_statement(exe, tmp_path, case):
    shape, option = case
    paired, fasta, kind, gz_out, mode, D, dual = shape
    k = SHAPES.index(shape)
    both, best = option == "both", option == "best"
    data = as_text(library(100 + k, paired, dual=dual, turned=both), mode, fasta, seed=k)
    labelled, levels, total, dups, plain, cluster_files, info = statement(data, mode, D, fasta, best, both)
    assert info["merged"] > 10 and statement(data, mode, 0, fasta, best, both)[3] < dups
    more = {"best": {"FQD_FAST_KEEP": "best"}, "clusters": {"FQD_FAST_CLUSTERS": "1"}, "both": {"FQD_FAST_STRAND": "both"},
            "sizeout": {"FQD_FAST_SIZEOUT": "1"}, "levels": {"FQD_FAST_LEVELS": "1"}}.get(option, {})
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env=switches(mode, D, FQD_HOST_TIMING="1", **more), fasta=fasta)
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    assert (f"fast: UMI mismatches <= {D}, {info['merged']} of {info['nodes']} exact clusters merged into others, largest network {info['largest']}, "
            f"{info['sweeps']} sweeps\n") in r.stderr
    for j, o in enumerate(outs):
        assert read_out(o) == (labelled if option == "sizeout" else plain)[j]
        assert beside(o, ".clusters").exists() == (option == "clusters")
        if option == "clusters":
            assert beside(o, ".clusters").read_bytes() == cluster_files[j]
        assert beside(o, ".duplevels").exists() == (option == "levels" and j == 0)
    if option == "levels":
        assert beside(outs[0], ".duplevels").read_bytes() == levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired,fasta,kind,gz_out", [(False, False, "plain", False), (True, False, "bgzf", True), (False, True, "gzip", False)])
def test_zero_and_an_unset_switch_give_the_exact_run_byte_for_byte(exe, tmp_path, paired, fasta, kind, gz_out):
    data = as_text(library(50 + int(paired), paired), "colon", fasta, seed=1)
    all_on = {"FQD_FAST_UMI": "colon", "FQD_FAST_CLUSTERS": "1", "FQD_FAST_SIZEOUT": "1", "FQD_FAST_LEVELS": "1", "FQD_HOST_TIMING": "1"}
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, env=all_on, tag="d", fasta=fasta)
    rz, outsz = cli(exe, tmp_path, data, kind, gz_out, env={**all_on, "FQD_FAST_UMI_MISMATCH": "0"}, tag="z", fasta=fasta)
    r1, outs1 = cli(exe, tmp_path, data, kind, gz_out, env={**all_on, "FQD_FAST_UMI_MISMATCH": "1"}, tag="m", fasta=fasta)
    assert r0.returncode == 0 and rz.returncode == 0 and r1.returncode == 0, r0.stderr + rz.stderr + r1.stderr
    assert r0.stdout == rz.stdout != r1.stdout
    assert "mismatches" not in r0.stderr and "mismatches" not in rz.stderr and "mismatches" in r1.stderr
    for a, b, c in zip(outs0, outsz, outs1):
        for ext in ("", ".clusters"):
            assert beside(a, ext).read_bytes() == beside(b, ext).read_bytes() != beside(c, ext).read_bytes()   # the files as they lie on disk
    assert beside(outs0[0], ".duplevels").read_bytes() == beside(outsz[0], ".duplevels").read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_a_file_without_umi_errors_is_written_as_the_exact_run_writes_it(exe, tmp_path, paired):
    data = as_text(library(60 + int(paired), paired, far_apart=True, error=0), "colon", seed=2)
    env = {"FQD_FAST_UMI": "colon", "FQD_FAST_CLUSTERS": "1", "FQD_FAST_SIZEOUT": "1", "FQD_FAST_LEVELS": "1"}
    r0, outs0 = cli(exe, tmp_path, data, env={**env, "FQD_FAST_UMI_MISMATCH": "0"}, tag="z")
    r1, outs1 = cli(exe, tmp_path, data, env={**env, "FQD_FAST_UMI_MISMATCH": "1"}, tag="m")
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert r0.stdout == r1.stdout
    for a, b in zip(outs0, outs1):
        for ext in ("", ".clusters"):
            assert beside(a, ext).read_bytes() == beside(b, ext).read_bytes()
    assert beside(outs0[0], ".duplevels").read_bytes() == beside(outs1[0], ".duplevels").read_bytes()


@pytest.mark.gpu
def test_a_sequence_under_more_umis_than_the_limit_is_refused(exe, tmp_path):
    from fastq_dupaway_amd import Engine
    with Engine(segments=1) as e:
        limit = e.umi_merge(None, None, None, _lib.UmiInfo(4, 4, 0, umi.NO_RECORD, 0, 0), None, None, None, 0, 1, None).max_group
    assert limit >= MAX_GROUP_AT_LEAST
    rng = random.Random(7)
    seen = set()
    while len(seen) < limit + 1:
        seen.add(rand_seq(rng, 8))
    amplicon = rand_seq(rng, 40)
    mols = [(rand_seq(rng, 8), rand_seq(rng, 30), None) for _ in range(5)] + [(u, amplicon, None) for u in sorted(seen)]
    data = as_text(mols, "colon", fasta=True)
    r, outs = cli(exe, tmp_path, data, env=switches("colon", 1, FQD_FAST_CLUSTERS="1", FQD_FAST_LEVELS="1"), fasta=True)
    assert r.returncode == 1
    assert "FQD_FAST_UMI_MISMATCH=1" in r.stderr and "record 5 " in r.stderr and f"{limit + 1} different UMIs" in r.stderr and str(limit) in r.stderr
    assert nothing_written(outs)
    r, outs = cli(exe, tmp_path, as_text(mols[:-1], "colon", fasta=True), env=switches("colon", 1), fasta=True, tag="b")       # one UMI fewer: taken
    assert r.returncode == 0, r.stderr
    labelled, _, total, dups, plain, _, info = statement(as_text(mols[:-1], "colon", fasta=True), "colon", 1, fasta=True)
    assert r.stdout == verbose_line(total, dups, False) and read_out(outs[0]) == plain[0] and info["largest"] == limit
