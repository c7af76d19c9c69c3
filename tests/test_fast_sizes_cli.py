"""FQD_FAST_SIZEOUT=1 and FQD_FAST_LEVELS=1 of the `--fast` mode through the CLI.  CPU part: what the command line decides,
before any GPU call.  GPU part: on small FASTQ and FASTA inputs — plain, BGZF and ordinary gzip in, plain and `.gz` out,
single-end and paired — the outputs are the statement's (tests/size_reference.py): the default run's records, each with
`;size=N` behind the first word of its ID line, and they differ from the default run's; `<output 1>.duplevels` is the
statement's table; the `-v` line does not change; the cluster files are those of a run without the labels; with
FQD_FAST_KEEP=best the label is on the best copy; with FQD_FAST_STRAND=both / FQD_FAST_UMI a cluster is what those switches
make it; small windows cut the output in many places; empty inputs, a pipe, and unset / `0` switches behave as documented."""
import gzip
import os
import random
import subprocess
from pathlib import Path

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib
import fast_keep_reference as fast
import size_reference as ref
import strand_reference as strand
import umi_reference as umi_ref
import test_fast_umi_cli as inputs                            # its generator of small inputs: molecules(), as_text(), PACK

SWITCHES = ("FQD_FAST_SIZEOUT", "FQD_FAST_LEVELS", "FQD_FAST_UMI", "FQD_FAST_STRAND", "FQD_FAST_KEEP", "FQD_FAST_CLUSTERS", "FQD_ORDERED_RESIDENT",
            "FQD_DEVICES", "FQD_GUNZIP_DEVICE", "FQD_HOST_TIMING", "FQD_STREAM_WINDOW_KB")
NO_GPU = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
SIZEOUT, LEVELS = {"FQD_FAST_SIZEOUT": "1"}, {"FQD_FAST_LEVELS": "1"}


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


def cli(exe, tmp_path, data, kind="plain", gz_out=False, env=None, tag="a", extra=(), fasta=False):
    ext = ".fa" if fasta else ".fq"
    ins = [tmp_path / f"in{tag}{k}{ext}{'' if kind == 'plain' else '.gz'}" for k in range(len(data))]
    outs = [tmp_path / f"out{tag}{k}{ext}{'.gz' if gz_out else ''}" for k in range(len(data))]
    for p, x in zip(ins, data):
        p.write_bytes(inputs.PACK[kind](x))
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


def levels_of(path):
    return Path(str(path) + ".duplevels")


def clusters_of(path):
    return Path(str(path) + ".clusters")


def nothing_written(outs):
    return all(not o.exists() and not levels_of(o).exists() and not clusters_of(o).exists() for o in outs)


def verbose_line(total, dups, paired):
    return f"{total} {'read pairs' if paired else 'reads'} processed, out of which {dups} duplicates were removed.\n"


def small_input(seed, paired, fasta=False, n=600, mode="colon", turned=False):
    return inputs.as_text(inputs.molecules(seed, paired, n=n, turned=turned), mode, fasta, seed=seed)


def mostly_distinct_input(seed, paired, n=600):
    """FASTQ files of n records (pairs) of 100 .. 150 bases, about a fifth of them copies of an earlier one."""
    rng = random.Random(seed)
    frags = []
    for k in range(n):
        if k and rng.random() < 0.2:
            frags.append(rng.choice(frags))
        else:
            frags.append(tuple("".join(rng.choice("ACGT") for _ in range(rng.randrange(100, 151))) for _ in range(2 if paired else 1)))
    files = []
    for m in range(2 if paired else 1):
        recs = []
        for k, f in enumerate(frags):
            s = f[m]
            recs.append(f"@read{k}{['', ' ', chr(9)][k % 3]}{'' if k % 3 == 0 else f'{m + 1}:N:0'}\n{s}\n+\n{''.join(chr(rng.randrange(40, 74)) for _ in s)}\n")
        files.append("".join(recs).encode())
    return files


# ---------------------------------------------------------------- CPU: decided before any GPU call

@pytest.mark.parametrize("env,names", [(SIZEOUT, ["FQD_FAST_SIZEOUT=1"]), (LEVELS, ["FQD_FAST_LEVELS=1"]),
                                       ({**SIZEOUT, **LEVELS}, ["FQD_FAST_SIZEOUT=1 and FQD_FAST_LEVELS=1"])], ids=["sizeout", "levels", "both"])
def test_unordered_is_refused(exe, tmp_path, env, names):
    r, outs = cli(exe, tmp_path, small_input(1, True, n=12), env={**NO_GPU, **env}, extra=["--unordered"])
    assert r.returncode == 1
    assert all(name in r.stderr for name in names) and "--unordered" in r.stderr
    assert nothing_written(outs)


@pytest.mark.parametrize("env,name", [(SIZEOUT, "FQD_FAST_SIZEOUT=1"), (LEVELS, "FQD_FAST_LEVELS=1")], ids=["sizeout", "levels"])
def test_several_devices_are_refused(exe, tmp_path, env, name):
    r, outs = cli(exe, tmp_path, small_input(2, False, n=12), env={**NO_GPU, **env, "FQD_DEVICES": "0,1"})
    assert r.returncode == 1
    assert r.stderr.count(name) == 1 and "FQD_DEVICES" in r.stderr
    assert nothing_written(outs)


@pytest.mark.parametrize("env,name", [(SIZEOUT, "FQD_FAST_SIZEOUT=1"), (LEVELS, "FQD_FAST_LEVELS=1")], ids=["sizeout", "levels"])
def test_resident_run_turned_off_is_refused(exe, tmp_path, env, name):
    r, outs = cli(exe, tmp_path, small_input(3, False, n=12), env={**NO_GPU, **env, "FQD_ORDERED_RESIDENT": "0"})
    assert r.returncode == 1
    assert r.stderr.count(name) == 1 and "FQD_ORDERED_RESIDENT" in r.stderr
    assert nothing_written(outs)


# ---------------------------------------------------------------- GPU

CASES = [(False, False, "plain", False), (False, False, "bgzf", True), (False, True, "gzip", False),
         (True, False, "plain", True), (True, True, "bgzf", False), (True, False, "gzip", False)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{'pe' if c[0] else 'se'}-{'fasta' if c[1] else 'fastq'}-{c[2]}-to-{'gz' if c[3] else 'plain'}" for c in CASES])
def test_labels_levels_and_the_verbose_line(exe, tmp_path, case):
    paired, fasta, kind, gz_out = case
    k = CASES.index(case)
    data = small_input(200 + k, paired, fasta, mode="colon" if k % 2 else "underscore")
    exp_out, exp_levels, total, dups, plain, _ = ref.dedup_sized(data, fasta)
    assert dups > 0 and plain == fast.dedup(data, fasta)[0]
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, tag="d", fasta=fasta)
    assert r0.returncode == 0 and r0.stdout == verbose_line(total, dups, paired), r0.stderr
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**SIZEOUT, **LEVELS, "FQD_HOST_TIMING": "1"}, fasta=fasta)
    assert r.returncode == 0, r.stderr
    assert r.stdout == r0.stdout                               # the `-v` line is unchanged
    largest = int(exp_levels.decode().splitlines()[-1].split("\t")[1])
    assert f"fast: cluster sizes, {total - dups} clusters, largest {largest}\n" in r.stderr
    for j, o in enumerate(outs):
        assert read_out(outs0[j]) == plain[j]
        assert read_out(o) == exp_out[j]                        # every written record with its cluster's size ...
        assert read_out(o) != read_out(outs0[j])                # ... which the default run does not write
        assert not clusters_of(o).exists()
    assert levels_of(outs[0]).read_bytes() == exp_levels
    assert all(not levels_of(o).exists() for o in outs[1:])     # pairs: one file, beside output 1
    # the table alone: the default run's bytes and the same table
    rl, outsl = cli(exe, tmp_path, data, kind, gz_out, env=LEVELS, tag="l", fasta=fasta)
    assert rl.returncode == 0 and rl.stdout == r0.stdout, rl.stderr
    assert [read_out(o) for o in outsl] == plain
    assert levels_of(outsl[0]).read_bytes() == exp_levels
    # the labels alone: no table
    rs, outss = cli(exe, tmp_path, data, kind, gz_out, env=SIZEOUT, tag="s", fasta=fasta)
    assert rs.returncode == 0 and rs.stdout == r0.stdout, rs.stderr
    assert [read_out(o) for o in outss] == exp_out
    assert not levels_of(outss[0]).exists()


@pytest.mark.gpu
@pytest.mark.parametrize("paired,kind,gz_out", [(False, "plain", False), (True, "bgzf", True)])
def test_cluster_files_keep_the_original_id_lines(exe, tmp_path, paired, kind, gz_out):
    data = small_input(210 + int(paired), paired)
    exp_out, exp_levels, total, dups, _, exp_cl = ref.dedup_sized(data)
    rc_, outsc = cli(exe, tmp_path, data, kind, gz_out, env={"FQD_FAST_CLUSTERS": "1"}, tag="c")
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**SIZEOUT, **LEVELS, "FQD_FAST_CLUSTERS": "1"})
    assert rc_.returncode == 0 and r.returncode == 0, rc_.stderr + r.stderr
    assert r.stdout == rc_.stdout == verbose_line(total, dups, paired)
    for j, o in enumerate(outs):
        assert read_out(o) == exp_out[j]
        assert clusters_of(o).read_bytes() == clusters_of(outsc[j]).read_bytes() == exp_cl[j]
    assert levels_of(outs[0]).read_bytes() == exp_levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired,kind,gz_out", [(False, "plain", False), (True, "gzip", True)])
def test_the_label_sits_on_the_best_copy(exe, tmp_path, paired, kind, gz_out):
    data = small_input(220 + int(paired), paired)
    exp_out, exp_levels, total, dups, plain, exp_cl = ref.dedup_sized(data, best=True)
    first_out = ref.dedup_sized(data)[0]
    assert exp_out != first_out and plain == fast.dedup(data, best=True)[0]
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**SIZEOUT, **LEVELS, "FQD_FAST_KEEP": "best", "FQD_FAST_CLUSTERS": "1"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    for j, o in enumerate(outs):
        assert read_out(o) == exp_out[j]
        assert clusters_of(o).read_bytes() == exp_cl[j]
    assert levels_of(outs[0]).read_bytes() == exp_levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_both_strands_make_the_clusters(exe, tmp_path, paired):
    data = small_input(230 + int(paired), paired, turned=True)
    files = [fast.parse(x, False) for x in data]
    keys = [strand.canon_key(files[0][i][2] if not paired else (files[0][i][2], files[1][i][2])) for i in range(len(files[0]))]
    exp_out, exp_levels, total, dups, _, _ = ref.dedup_sized(data, keys=keys)
    assert dups > ref.dedup_sized(data)[3] > 0                  # both strands of one fragment among the records
    r, outs = cli(exe, tmp_path, data, env={**SIZEOUT, **LEVELS, "FQD_FAST_STRAND": "both"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    assert [read_out(o) for o in outs] == exp_out
    assert levels_of(outs[0]).read_bytes() == exp_levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_umis_make_the_clusters(exe, tmp_path, paired):
    data = small_input(240 + int(paired), paired)
    files = [fast.parse(x, False) for x in data]
    keys = [umi_ref.key_of(files[0][i][1], b":", *(f[i][2] for f in files)) for i in range(len(files[0]))]
    exp_out, exp_levels, total, dups, _, _ = ref.dedup_sized(data, keys=keys)
    assert ref.dedup_sized(data)[3] > dups > 0                  # one sequence under several UMIs, and true copies
    r, outs = cli(exe, tmp_path, data, env={**SIZEOUT, **LEVELS, "FQD_FAST_UMI": "colon"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    assert [read_out(o) for o in outs] == exp_out
    assert levels_of(outs[0]).read_bytes() == exp_levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired,gz_out", [(False, False), (True, True)])
def test_many_small_windows(exe, tmp_path, paired, gz_out):
    data = mostly_distinct_input(250 + int(paired), paired)
    exp_out, exp_levels, total, dups, _, _ = ref.dedup_sized(data)
    assert dups > 50 and len(exp_out[0]) > 20 * 5120                          # more than twenty windows of 4 KiB (5 KiB at the most)
    r, outs = cli(exe, tmp_path, data, gz_out=gz_out, env={**SIZEOUT, **LEVELS, "FQD_STREAM_WINDOW_KB": "4"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    assert [read_out(o) for o in outs] == exp_out
    assert levels_of(outs[0]).read_bytes() == exp_levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_empty_inputs(exe, tmp_path, paired):
    data = [b""] * (2 if paired else 1)
    r0, outs0 = cli(exe, tmp_path, data, tag="d")
    r, outs = cli(exe, tmp_path, data, env={**SIZEOUT, **LEVELS})
    assert (r.returncode, r.stdout, r.stderr) == (r0.returncode, r0.stdout, r0.stderr)
    for a, b in zip(outs0, outs):
        assert a.exists() == b.exists()
        if a.exists():
            assert a.read_bytes() == b.read_bytes()
    assert levels_of(outs[0]).read_bytes() == ref.duplevels_text([])
    text = levels_of(outs[0]).read_text().splitlines()
    assert len(text) == 19 and all(line.endswith("\t0\t0") for line in text[1:18]) and text[18] == "#largest\t0"
    assert not any(levels_of(o).exists() for o in outs0)


@pytest.mark.gpu
@pytest.mark.parametrize("env,name", [(SIZEOUT, "FQD_FAST_SIZEOUT=1"), (LEVELS, "FQD_FAST_LEVELS=1")], ids=["sizeout", "levels"])
def test_a_pipe_is_refused(exe, tmp_path, env, name):
    fifo = tmp_path / "in.fq"
    os.mkfifo(fifo)
    out = tmp_path / "o.fq"
    r = run(exe, "-i", fifo, "-o", out, "--fast", env=env)       # refused on the file's type: the pipe is never opened
    assert r.returncode == 1
    assert r.stderr.count(name) == 1 and "not a regular file" in r.stderr
    assert not out.exists() and not levels_of(out).exists()


@pytest.mark.gpu
def test_a_malformed_record_is_refused_before_any_output(exe, tmp_path):
    good = small_input(5, False, n=50)[0]
    r, outs = cli(exe, tmp_path, [good[:-7]], env={**SIZEOUT, **LEVELS})      # the last record is cut short
    assert r.returncode == 1
    assert "FQD_FAST_SIZEOUT=1 and FQD_FAST_LEVELS=1" in r.stderr
    assert nothing_written(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("paired,fasta,kind,gz_out", [(False, False, "plain", False), (True, False, "bgzf", True), (False, True, "gzip", False)])
def test_unset_and_zero_give_the_default_bytes(exe, tmp_path, paired, fasta, kind, gz_out):
    data = small_input(260 + int(paired), paired, fasta)
    plain_out, _, total, dups, _ = fast.dedup(data, fasta)
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, tag="d", fasta=fasta)
    rz, outsz = cli(exe, tmp_path, data, kind, gz_out, env={"FQD_FAST_SIZEOUT": "0", "FQD_FAST_LEVELS": "0", "FQD_HOST_TIMING": "1"}, tag="z", fasta=fasta)
    assert r0.returncode == 0 and rz.returncode == 0, r0.stderr + rz.stderr
    assert r0.stdout == rz.stdout == verbose_line(total, dups, paired)
    assert "cluster sizes" not in rz.stderr
    for j, (a, b) in enumerate(zip(outs0, outsz)):
        assert a.read_bytes() == b.read_bytes()
        assert read_out(a) == plain_out[j]
        assert not levels_of(b).exists()
