"""FQD_FAST_SORT=size, FQD_FAST_MINSIZE=N and FQD_FAST_MAXSIZE=N of the `--fast` mode through the CLI.  CPU part: what the
values and the command line decide, before any GPU call.  GPU part: on inputs of a few hundred records with ties and distinct
cluster sizes — single-end and paired, FASTQ and FASTA, plain, BGZF and ordinary gzip in, plain and `.gz` out, many small
windows — the outputs are the statement's (tests/size_order_reference.py): under SORT=size the default run's records in another
order, with FQD_FAST_SIZEOUT labels that descend; under a filter the clusters outside the bounds are missing and `-v` says so;
`.clusters`, `.duplevels` and the first `-v` line never change; FQD_FAST_KEEP / _STRAND / _UMI / _UMI_MISMATCH decide what a
cluster is and which member is written; unset switches and their defaults give the default run's bytes."""
import os
import random
import re
import subprocess

import pytest

import fast_keep_reference as fast
import size_order_reference as ref
import size_reference as sized
import strand_reference as strand
import umi_merge_reference as mref
import umi_reference as umi
import test_fast_sizes_cli as base                            # its helpers: exe, read_out, small_input, verbose_line, ...
import test_fast_umi_merge_cli as merge_cli                   # its generator of UMI libraries with errors
from test_fast_sizes_cli import exe                           # noqa: F401  (the fixture)

SWITCHES = base.SWITCHES + ("FQD_FAST_SORT", "FQD_FAST_MINSIZE", "FQD_FAST_MAXSIZE", "FQD_FAST_UMI_MISMATCH")
NO_GPU = base.NO_GPU
BY_SIZE = {"FQD_FAST_SORT": "size"}
SIZEOUT = base.SIZEOUT


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
        p.write_bytes(base.inputs.PACK[kind](x))
    args = ["-i", ins[0], "-o", outs[0]]
    if len(data) == 2:
        args += ["-u", ins[1], "-p", outs[1]]
    args += ["--fast", "-v", *extra]
    if fasta:
        args += ["--format", "fasta"]
    return run(exe, *args, env=env), outs


SIZES = [260, 257, 12, 7, 5, 5, 3, 3, 3, 2, 2, 2, 2] + [1] * 40      # ties and distinct sizes, two clusters above 255


def sized_input(seed, paired, fasta=False):
    """Files of sum(SIZES) records (pairs): one cluster per entry of SIZES, the members shuffled over the file; ID lines with
    and without a comment; qualities that differ from copy to copy."""
    rng = random.Random(seed)
    frags = [tuple("".join(rng.choice("ACGT") for _ in range(rng.randrange(30, 90))) for _ in range(2 if paired else 1)) for _ in SIZES]
    members = [k for k, s in enumerate(SIZES) for _ in range(s)]
    rng.shuffle(members)
    files = []
    for m in range(2 if paired else 1):
        recs = []
        for i, k in enumerate(members):
            s = frags[k][m]
            line = f"{'>' if fasta else '@'}read{i}{['', ' ', chr(9)][i % 3]}{'' if i % 3 == 0 else f'{m + 1}:N:0'}\n"
            recs.append(f"{line}{s}\n" if fasta else f"{line}{s}\n+\n{''.join(chr(rng.randrange(40, 74)) for _ in s)}\n")
        files.append("".join(recs).encode())
    return files


def has_ties_and_distinct_sizes(written):
    return len(set(written)) > 2 and len(set(written)) < len(written)


def record_multiset(data, fasta):
    return sorted(r for r, _, _ in fast.parse(data, fasta))


def label_sizes(data):
    return [int(x) for x in re.findall(rb"^[@>][^\n]*?;size=(\d+)", data, re.M)]


# ---------------------------------------------------------------- CPU: decided before any GPU call

BAD_VALUES = [({"FQD_FAST_SORT": "abundance"}, "FQD_FAST_SORT"), ({"FQD_FAST_SORT": ""}, "FQD_FAST_SORT"),
              ({"FQD_FAST_MINSIZE": "0"}, "FQD_FAST_MINSIZE"), ({"FQD_FAST_MINSIZE": "-1"}, "FQD_FAST_MINSIZE"), ({"FQD_FAST_MINSIZE": "2x"}, "FQD_FAST_MINSIZE"),
              ({"FQD_FAST_MINSIZE": "2147483648"}, "FQD_FAST_MINSIZE"), ({"FQD_FAST_MINSIZE": ""}, "FQD_FAST_MINSIZE"),
              ({"FQD_FAST_MAXSIZE": "0"}, "FQD_FAST_MAXSIZE"), ({"FQD_FAST_MAXSIZE": "+3"}, "FQD_FAST_MAXSIZE"), ({"FQD_FAST_MAXSIZE": "99999999999"}, "FQD_FAST_MAXSIZE"),
              ({"FQD_FAST_MAXSIZE": "1", "FQD_FAST_MINSIZE": "2"}, "FQD_FAST_MAXSIZE=1")]


@pytest.mark.parametrize("env,name", BAD_VALUES, ids=["-".join(f"{k[9:]}={v}" for k, v in e.items()) for e, _ in BAD_VALUES])
def test_a_bad_value_ends_the_run_before_any_gpu_call(exe, tmp_path, env, name):
    r, outs = cli(exe, tmp_path, sized_input(1, False)[:1], env={**NO_GPU, **env})
    assert r.returncode == 1
    assert name in r.stderr and "no ROCm-capable device" not in r.stderr and "hipSetDevice" not in r.stderr      # not the "no GPU" message
    assert base.nothing_written(outs)


EACH = [(BY_SIZE, "FQD_FAST_SORT=size"), ({"FQD_FAST_MINSIZE": "2"}, "FQD_FAST_MINSIZE=2"), ({"FQD_FAST_MAXSIZE": "5"}, "FQD_FAST_MAXSIZE=5")]
EACH_IDS = ["sort", "minsize", "maxsize"]


@pytest.mark.parametrize("env,name", EACH, ids=EACH_IDS)
def test_unordered_is_refused(exe, tmp_path, env, name):
    r, outs = cli(exe, tmp_path, sized_input(2, True), env={**NO_GPU, **env}, extra=["--unordered"])
    assert r.returncode == 1
    assert r.stderr.count(name) == 1 and "--unordered" in r.stderr and "no ROCm-capable device" not in r.stderr
    assert base.nothing_written(outs)


@pytest.mark.parametrize("env,name", EACH, ids=EACH_IDS)
def test_several_devices_are_refused(exe, tmp_path, env, name):
    r, outs = cli(exe, tmp_path, sized_input(3, False), env={**NO_GPU, **env, "FQD_DEVICES": "0,1"})
    assert r.returncode == 1
    assert r.stderr.count(name) == 1 and "FQD_DEVICES" in r.stderr
    assert base.nothing_written(outs)


def test_all_three_are_named_together(exe, tmp_path):
    r, outs = cli(exe, tmp_path, sized_input(4, True), env={**NO_GPU, **BY_SIZE, "FQD_FAST_MINSIZE": "2", "FQD_FAST_MAXSIZE": "9", **SIZEOUT}, extra=["--unordered"])
    assert r.returncode == 1
    assert "FQD_FAST_SIZEOUT=1 and FQD_FAST_SORT=size and FQD_FAST_MINSIZE=2 and FQD_FAST_MAXSIZE=9 with --unordered" in r.stderr
    assert base.nothing_written(outs)


@pytest.mark.parametrize("env,name", EACH, ids=EACH_IDS)
def test_resident_run_turned_off_is_refused(exe, tmp_path, env, name):
    r, outs = cli(exe, tmp_path, sized_input(5, False), env={**NO_GPU, **env, "FQD_ORDERED_RESIDENT": "0"})
    assert r.returncode == 1
    assert r.stderr.count(name) == 1 and "FQD_ORDERED_RESIDENT" in r.stderr
    assert base.nothing_written(outs)


# ---------------------------------------------------------------- GPU

CASES = [(False, False, "plain", False), (False, False, "bgzf", True), (False, True, "gzip", False),
         (True, False, "plain", True), (True, True, "bgzf", False), (True, False, "gzip", False)]
CASE_IDS = [f"{'pe' if c[0] else 'se'}-{'fasta' if c[1] else 'fastq'}-{c[2]}-to-{'gz' if c[3] else 'plain'}" for c in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_order_by_size(exe, tmp_path, case):
    paired, fasta, kind, gz_out = case
    data = sized_input(300 + CASES.index(case), paired, fasta)
    plain, _, total, dups, _ = fast.dedup(data, fasta)
    exp, gone, _, written = ref.dedup_ordered(data, fasta, by_size=True)
    exp_labelled = ref.dedup_ordered(data, fasta, by_size=True, sizeout=True)[0]
    assert has_ties_and_distinct_sizes(written) and gone == 0 and written[1] > 255 and sorted(written, reverse=True) == sorted(SIZES, reverse=True)
    all_on = {"FQD_FAST_CLUSTERS": "1", "FQD_FAST_LEVELS": "1"}
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, env=all_on, tag="d", fasta=fasta)
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**all_on, **BY_SIZE, "FQD_HOST_TIMING": "1"}, fasta=fasta)
    rs, outss = cli(exe, tmp_path, data, kind, gz_out, env={**BY_SIZE, **SIZEOUT}, tag="s", fasta=fasta)
    assert r0.returncode == 0 and r.returncode == 0 and rs.returncode == 0, r0.stderr + r.stderr + rs.stderr
    assert r.stdout == rs.stdout == r0.stdout == base.verbose_line(total, dups, paired)      # the `-v` line, and no second one
    assert f"fast: abundance order, {len(written)} clusters written, 2 of them above 255 members sorted apart\n" in r.stderr
    assert "size filter" not in r.stderr
    for j, o in enumerate(outs):
        got, default = base.read_out(o), base.read_out(outs0[j])
        assert default == plain[j]
        assert got == exp[j]
        assert got != default and record_multiset(got, fasta) == record_multiset(default, fasta)     # the same records in another order
        assert base.clusters_of(o).read_bytes() == base.clusters_of(outs0[j]).read_bytes()           # all clusters, in input order
        labelled = base.read_out(outss[j])
        assert labelled == exp_labelled[j]
        assert label_sizes(labelled) == written                                                      # the labels decrease down the file
    assert base.levels_of(outs[0]).read_bytes() == base.levels_of(outs0[0]).read_bytes() == sized.duplevels_text(SIZES)


FILTERS = [(2, None), (1, 1), (261, None), (3, 12), (1, 2147483647)]


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", FILTERS, ids=[f"min{lo}-max{hi or 'none'}" for lo, hi in FILTERS])
@pytest.mark.parametrize("paired,fasta,kind,gz_out", [(False, False, "plain", False), (True, False, "bgzf", True)], ids=["se-plain", "pe-bgzf-to-gz"])
def test_the_filter(exe, tmp_path, paired, fasta, kind, gz_out, lo, hi):
    data = sized_input(320 + int(paired), paired, fasta)
    _, _, total, dups, _ = fast.dedup(data, fasta)
    env = {"FQD_FAST_MINSIZE": str(lo), **({"FQD_FAST_MAXSIZE": str(hi)} if hi else {})}
    all_on = {"FQD_FAST_CLUSTERS": "1", "FQD_FAST_LEVELS": "1"}
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, env=all_on, tag="d", fasta=fasta)
    assert r0.returncode == 0, r0.stderr
    for by_size in (False, True):
        exp, gone, gone_records, written = ref.dedup_ordered(data, fasta, by_size=by_size, lo=lo, hi=hi, sizeout=True)
        assert (written == []) == (lo == 261) and (gone == 0) == (hi == 2147483647)
        r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**all_on, **env, **SIZEOUT, **(BY_SIZE if by_size else {}), "FQD_HOST_TIMING": "1"},
                      tag=f"f{int(by_size)}", fasta=fasta)
        assert r.returncode == 0, r.stderr
        assert r.stdout == base.verbose_line(total, dups, paired) + ref.not_written_line(gone, gone_records, paired, lo, hi)
        assert f"fast: size filter, {gone} clusters of {gone_records} records not written\n" in r.stderr
        assert [base.read_out(o) for o in outs] == exp
        assert all(o.exists() for o in outs)                                   # a filter that takes everything leaves empty files
        for j, o in enumerate(outs):
            assert base.clusters_of(o).read_bytes() == base.clusters_of(outs0[j]).read_bytes()
        assert base.levels_of(outs[0]).read_bytes() == base.levels_of(outs0[0]).read_bytes()        # counted before the filter
    if lo == 261:                                                                # what an empty-input run writes, where it writes
        _, outse = cli(exe, tmp_path, [b""] * len(data), "plain", gz_out, tag="e", fasta=fasta)
        assert all(a.read_bytes() == b.read_bytes() for a, b in zip(outs, outse) if b.exists())
        assert all(o.stat().st_size == 0 for o in outs if not gz_out)


@pytest.mark.gpu
@pytest.mark.parametrize("paired,gz_out", [(False, False), (True, True)], ids=["se", "pe-to-gz"])
def test_many_small_windows_cut_the_permuted_output(exe, tmp_path, paired, gz_out):
    data = base.mostly_distinct_input(330 + int(paired), paired)
    exp, gone, gone_records, written = ref.dedup_ordered(data, by_size=True, sizeout=True)
    assert has_ties_and_distinct_sizes(written) and len(exp[0]) > 20 * 5120     # more than twenty windows of 4 KiB (5 KiB at the most)
    r, outs = cli(exe, tmp_path, data, gz_out=gz_out, env={**BY_SIZE, **SIZEOUT, "FQD_STREAM_WINDOW_KB": "4"})
    assert r.returncode == 0, r.stderr
    assert [base.read_out(o) for o in outs] == exp
    exp2 = ref.dedup_ordered(data, by_size=True, lo=2)[0]
    r, outs = cli(exe, tmp_path, data, gz_out=gz_out, env={**BY_SIZE, "FQD_FAST_MINSIZE": "2", "FQD_STREAM_WINDOW_KB": "4"}, tag="m")
    assert r.returncode == 0, r.stderr
    assert [base.read_out(o) for o in outs] == exp2


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_best_copy_stands_at_its_clusters_place(exe, tmp_path, paired):
    data = sized_input(340 + int(paired), paired)
    exp, _, _, written = ref.dedup_ordered(data, best=True, by_size=True, sizeout=True)
    first = ref.dedup_ordered(data, by_size=True, sizeout=True)[0]
    assert exp != first and label_sizes(exp[0]) == label_sizes(first[0]) == written      # other members, the same places
    r, outs = cli(exe, tmp_path, data, env={**BY_SIZE, **SIZEOUT, "FQD_FAST_KEEP": "best", "FQD_FAST_CLUSTERS": "1"})
    assert r.returncode == 0, r.stderr
    assert [base.read_out(o) for o in outs] == exp
    for j, o in enumerate(outs):
        assert base.clusters_of(o).read_bytes() == sized.dedup_sized(data, best=True)[5][j]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_both_strands_make_the_clusters(exe, tmp_path, paired):
    data = base.small_input(350 + int(paired), paired, turned=True)
    files = [fast.parse(x, False) for x in data]
    keys = [strand.canon_key(files[0][i][2] if not paired else (files[0][i][2], files[1][i][2])) for i in range(len(files[0]))]
    exp, gone, gone_records, written = ref.dedup_ordered(data, keys=keys, by_size=True, lo=3, sizeout=True)
    assert has_ties_and_distinct_sizes(written) and gone > 0 and exp != ref.dedup_ordered(data, by_size=True, lo=3, sizeout=True)[0]
    r, outs = cli(exe, tmp_path, data, env={**BY_SIZE, **SIZEOUT, "FQD_FAST_MINSIZE": "3", "FQD_FAST_STRAND": "both"})
    assert r.returncode == 0, r.stderr
    assert r.stdout.endswith(ref.not_written_line(gone, gone_records, paired, 3, None))
    assert [base.read_out(o) for o in outs] == exp


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_umis_and_their_errors_make_the_clusters(exe, tmp_path, paired):
    data = merge_cli.as_text(merge_cli.library(360 + int(paired), paired), "colon", seed=360)
    files = [fast.parse(x, False) for x in data]
    umis = [umi.bases(umi.umi_of(files[0][i][1], merge_cli.MODE["colon"])[1]) for i in range(len(files[0]))]
    seqs = [tuple(f[i][2] for f in files) for i in range(len(files[0]))]
    owner = [int(o) for o in mref.merge(umis, seqs, 1, 1 << 30)[0]]
    exp, _, _, written = ref.dedup_ordered(data, keys=owner, by_size=True, sizeout=True)
    exact = ref.dedup_ordered(data, keys=list(zip(umis, seqs)), by_size=True, sizeout=True)[0]
    assert has_ties_and_distinct_sizes(written) and exp != exact != ref.dedup_ordered(data, by_size=True, sizeout=True)[0]
    r, outs = cli(exe, tmp_path, data, env={**BY_SIZE, **SIZEOUT, "FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1"})
    assert r.returncode == 0, r.stderr
    assert [base.read_out(o) for o in outs] == exp
    r, outs = cli(exe, tmp_path, data, env={**BY_SIZE, **SIZEOUT, "FQD_FAST_UMI": "colon"}, tag="x")
    assert r.returncode == 0, r.stderr
    assert [base.read_out(o) for o in outs] == exact


@pytest.mark.gpu
@pytest.mark.parametrize("paired,fasta,kind,gz_out", [(False, False, "plain", False), (True, False, "bgzf", True), (False, True, "gzip", False)])
def test_unset_switches_and_their_defaults_give_the_default_bytes(exe, tmp_path, paired, fasta, kind, gz_out):
    data = sized_input(370 + int(paired), paired, fasta)
    plain, _, total, dups, _ = fast.dedup(data, fasta)
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, tag="d", fasta=fasta)
    rz, outsz = cli(exe, tmp_path, data, kind, gz_out, env={"FQD_FAST_SORT": "input", "FQD_FAST_MINSIZE": "1", "FQD_HOST_TIMING": "1"}, tag="z", fasta=fasta)
    assert r0.returncode == 0 and rz.returncode == 0, r0.stderr + rz.stderr
    assert r0.stdout == rz.stdout == base.verbose_line(total, dups, paired)
    assert not any(word in rz.stderr for word in ("cluster sizes", "size filter", "abundance order", "owners and clusters"))      # not `linked`
    for j, (a, b) in enumerate(zip(outs0, outsz)):
        assert a.read_bytes() == b.read_bytes() and base.read_out(a) == plain[j]


@pytest.mark.gpu
@pytest.mark.parametrize("paired,fasta", [(False, False), (True, False), (False, True), (True, True)], ids=["se-fastq", "pe-fastq", "se-fasta", "pe-fasta"])
def test_empty_inputs_are_the_default_runs(exe, tmp_path, paired, fasta):
    """The siblings' empty-input behaviour: whatever the default run makes of empty files — exit status, both streams, the
    outputs — and no second `-v` line, whether that run ends with an error or not."""
    env = {**BY_SIZE, "FQD_FAST_MINSIZE": "2", "FQD_FAST_MAXSIZE": "9"}
    data = [b""] * (2 if paired else 1)
    r0, outs0 = cli(exe, tmp_path, data, tag="d", fasta=fasta)
    r, outs = cli(exe, tmp_path, data, env=env, fasta=fasta)
    assert (r.returncode, r.stdout, r.stderr) == (r0.returncode, r0.stdout, r0.stderr)
    assert "were not written" not in r.stdout
    for a, b in zip(outs0, outs):
        assert a.exists() == b.exists() and (not a.exists() or a.read_bytes() == b.read_bytes())


@pytest.mark.gpu
def test_a_malformed_record_is_refused_before_any_output(exe, tmp_path):
    env = {**BY_SIZE, "FQD_FAST_MINSIZE": "2"}
    good = sized_input(6, False)[0]
    r, outs = cli(exe, tmp_path, [good[:-7]], env=env, tag="m")               # the last record is cut short
    assert r.returncode == 1 and "FQD_FAST_SORT=size and FQD_FAST_MINSIZE=2" in r.stderr
    assert base.nothing_written(outs)
