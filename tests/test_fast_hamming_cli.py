"""FQD_FAST_HAMMING=D of the `--fast` mode through the CLI.  CPU part: what the switch's value and the command line decide,
before any GPU call.  GPU part, on inputs of fragments x copies with substituted bases, 300 .. 1 500 records with Illumina
names — FASTQ and FASTA, plain, BGZF and ordinary gzip, single-end and paired: the outputs, `.clusters`, `;size=N`,
`.duplevels` and the `-v` lines are those of the Python statements the other CLI tests use (tests/size_reference.py,
tests/size_order_reference.py, tests/sizein_reference.py, tests/optical_reference.py) fed the merged owners of the sequential
statement (tests/near_reference.py), alone and combined with the other switches; unset and 0 give the default run's bytes; a
seed group beyond the limit ends the run before any output."""
import os
import random
import subprocess
from pathlib import Path

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib
import fast_keep_reference as fast
import near_reference as ref
import optical_reference as optical_ref
import size_order_reference as order_ref
import size_reference as sizes
import sizein_reference as sizein
from near_cases import group_records
import test_fast_sizes_cli as base                            # its file helpers
import test_fast_umi_cli as inputs                            # PACK

SWITCHES = base.SWITCHES + ("FQD_FAST_HAMMING", "FQD_FAST_OPTICAL", "FQD_FAST_SIZEIN", "FQD_FAST_SORT", "FQD_FAST_MINSIZE", "FQD_FAST_MAXSIZE", "FQD_FAST_UMI_MISMATCH",
                            "FQD_NEAR_EDGE_ROOM")
NO_GPU = base.NO_GPU
ALL = {"FQD_FAST_SIZEOUT": "1", "FQD_FAST_LEVELS": "1", "FQD_FAST_CLUSTERS": "1"}
read_out, levels_of, clusters_of, nothing_written, verbose_line = base.read_out, base.levels_of, base.clusters_of, base.nothing_written, base.verbose_line
D = 2
PIXELS = 100


def hamming(d=D):
    return {"FQD_FAST_HAMMING": str(d)}


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


def substituted(rng, s, count):
    s = list(s)
    for at in rng.sample(range(len(s)), count):
        s[at] = rng.choice([c for c in "ACGTN" if c != s[at]])
    return "".join(s)


def copies_input(seed, paired, fasta=False, fragments=150, d=D, sizein=False):
    """Fragments x copies, shuffled: a copy is the fragment, or the copy before it, with 0 .. d + 1 bases substituted in every
    mate ('N' among the letters), so that chains form; now and then an exact copy.  Every copy has a place on the flow cell, near the
    copy before it or anywhere.  sizein: an 8th field with `;size=N` in the first word."""
    rng = random.Random(seed)
    records = []
    for _ in range(fragments):
        first = tuple("".join(rng.choice("ACGT") for _ in range(rng.choice([60, 61, 75, 100]))) for _ in range(2 if paired else 1))
        seqs, x, y = first, rng.randrange(1000, 30000), rng.randrange(1000, 30000)
        for _ in range(rng.choice([1, 1, 2, 3, 5, 8])):
            records.append((seqs, x, y))
            seqs = tuple(substituted(rng, s, rng.choice([0, 0, 1, 1, 2, d, d + 1])) for s in rng.choice([first, seqs]))
            if rng.random() < 0.5:
                x, y = x + rng.randrange(-PIXELS // 2, PIXELS // 2 + 1), y + rng.randrange(-PIXELS // 2, PIXELS // 2 + 1)
            else:
                x, y = rng.randrange(1000, 30000), rng.randrange(1000, 30000)
    rng.shuffle(records)
    lead = ">" if fasta else "@"
    files = []
    for m in range(2 if paired else 1):
        out = []
        for k, (seqs, x, y) in enumerate(records):
            tail = f":n{k};size={1 + k % 7}" if sizein else ""
            head = f"{lead}M01:7:FC1:1:1101:{x}:{y}{tail} {m + 1}:N:0:ACGT\n"
            s = seqs[m]
            out.append(f"{head}{s}\n" if fasta else f"{head}{s}\n+\n{''.join(chr(rng.randrange(40, 74)) for _ in s)}\n")
        files.append("".join(out).encode())
    return files


def statement(data, fasta, d=D):
    """(the merged owner of every record, the exact clusters, the merged clusters) by the sequential statement."""
    files = [fast.parse(x, fasta) for x in data]
    records = [tuple(f[i][2] for f in files) for i in range(len(files[0]))]
    owner, nodes, merged = ref.merged_owners(records, d)
    return [int(o) for o in owner], nodes, merged


def second_line(taken, paired, d=D):
    if paired:
        return f"{taken} distinct sequence pairs were taken for copies of another that differs in at most {d} bases a mate (FQD_FAST_HAMMING={d}).\n"
    return f"{taken} distinct sequences were taken for copies of another that differs in at most {d} bases (FQD_FAST_HAMMING={d}).\n"


# ---------------------------------------------------------------- CPU: decided before any GPU call

@pytest.mark.parametrize("value", ["4", "-1", "x", "", "1.5", "01", "1 "])
def test_a_bad_value_is_refused(exe, tmp_path, value):
    r, outs = cli(exe, tmp_path, copies_input(1, False, fragments=4), env={**NO_GPU, **hamming(value)})
    assert r.returncode == 1
    assert f"FQD_FAST_HAMMING must be 0, 1, 2 or 3, not '{value}'" in r.stderr
    assert nothing_written(outs)


def test_the_switches_it_does_not_go_with_are_refused(exe, tmp_path):
    data = copies_input(2, True, fragments=4)
    r, outs = cli(exe, tmp_path, data, env={**NO_GPU, **hamming(1), "FQD_FAST_STRAND": "both"})
    assert r.returncode == 1 and "FQD_FAST_HAMMING=1 with FQD_FAST_STRAND=both: a substituted base can change which orientation" in r.stderr
    assert nothing_written(outs)
    r, outs = cli(exe, tmp_path, data, env={**NO_GPU, **hamming(3), "FQD_FAST_UMI": "colon"})
    assert r.returncode == 1 and "FQD_FAST_HAMMING=3 with FQD_FAST_UMI=colon: which sequences under one UMI are copies of one molecule is a rule of its own" in r.stderr
    assert nothing_written(outs)
    r, outs = cli(exe, tmp_path, data, env={**NO_GPU, **hamming(2), "FQD_FAST_UMI": "underscore", "FQD_FAST_UMI_MISMATCH": "1"})
    assert r.returncode == 1 and "FQD_FAST_HAMMING=2 with FQD_FAST_UMI=underscore and FQD_FAST_UMI_MISMATCH=1: which sequences under one UMI" in r.stderr
    assert nothing_written(outs)


def test_unordered_and_several_devices_are_refused_by_name(exe, tmp_path):
    r, outs = cli(exe, tmp_path, copies_input(2, True, fragments=4), env={**NO_GPU, **hamming(3)}, extra=["--unordered"])
    assert r.returncode == 1 and "FQD_FAST_HAMMING=3 with --unordered: these modes run on ordered inputs only" in r.stderr
    assert nothing_written(outs)
    r, outs = cli(exe, tmp_path, copies_input(2, False, fragments=4), env={**NO_GPU, **hamming(1), "FQD_DEVICES": "0,1"})
    assert r.returncode == 1 and "FQD_FAST_HAMMING=1 runs on one GPU: FQD_DEVICES may name one device only" in r.stderr
    assert nothing_written(outs)
    r, outs = cli(exe, tmp_path, copies_input(2, False, fragments=4), env={**NO_GPU, **hamming(2), "FQD_FAST_KEEP": "best", "FQD_ORDERED_RESIDENT": "0"})
    assert r.returncode == 1 and "FQD_FAST_KEEP=best and FQD_FAST_HAMMING=2" in r.stderr and "FQD_ORDERED_RESIDENT" in r.stderr      # no streaming run for it
    assert nothing_written(outs)


@pytest.mark.parametrize("value", [None, "0"])
def test_zero_and_unset_are_off(exe, tmp_path, value):
    # off: `--unordered` is not refused by the switch's name (without a GPU the run then ends for that reason)
    env = {**NO_GPU, **({} if value is None else hamming(value))}
    r, _ = cli(exe, tmp_path, copies_input(3, True, fragments=4), env=env, extra=["--unordered"])
    assert "FQD_FAST_HAMMING" not in r.stderr


def test_the_inputs_of_these_tests():
    for paired in (False, True):
        for d in (1, 2, 3):
            data = copies_input(4, paired, d=d)
            owner, nodes, merged = statement(data, False, d)
            n = len(owner)
            assert 300 <= n <= 1500 and 150 <= merged < nodes - 40 and nodes < n - 20      # exact copies, merged ones, and some that stay apart
            files = [fast.parse(x, False) for x in data]
            records = [tuple(f[i][2] for f in files) for i in range(n)]
            # single linkage: members that are not near their cluster's first record
            assert sum(1 for i in range(n) if not ref.near(records[i], records[owner[i]], d)) > 0


# ---------------------------------------------------------------- GPU

CASES = base.CASES


def check_run(r, outs, data, fasta, paired, d=D, expect=None):
    """The run's two `-v` lines, outputs with labels, cluster files and level table against size_reference fed the merged owners."""
    owner, nodes, merged = statement(data, fasta, d)
    exp_out, exp_levels, total, dups, _, exp_clusters = expect(owner) if expect else sizes.dedup_sized(data, fasta, keys=owner)
    assert dups == total - merged
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired) + second_line(nodes - merged, paired, d)
    assert [read_out(o) for o in outs] == exp_out
    assert [clusters_of(o).read_bytes() for o in outs] == exp_clusters
    assert levels_of(outs[0]).read_bytes() == exp_levels
    return nodes, merged


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{'pe' if c[0] else 'se'}-{'fasta' if c[1] else 'fastq'}-{c[2]}-to-{'gz' if c[3] else 'plain'}" for c in CASES])
def test_copies_with_substituted_bases_are_removed(exe, tmp_path, case):
    paired, fasta, kind, gz_out = case
    d = 1 + CASES.index(case) % 3
    data = copies_input(500 + CASES.index(case), paired, fasta, d=d)
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**hamming(d), **ALL, "FQD_HOST_TIMING": "1"}, fasta=fasta)
    nodes, merged = check_run(r, outs, data, fasta, paired, d)
    assert f"fast: substitutions <= {d}, {nodes - merged} of {nodes} exact clusters merged into others, " in r.stderr
    assert " pairs compared, " in r.stderr and " near, largest seed group " in r.stderr and " sweeps\n" in r.stderr
    # without the labels: the records as they stand, the first of every merged cluster at its place
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env=hamming(d), tag="p", fasta=fasta)
    assert r.returncode == 0 and [read_out(o) for o in outs] == sizes.dedup_sized(data, fasta, keys=statement(data, fasta, d)[0])[4]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_best_copy_of_a_merged_cluster_is_written(exe, tmp_path, paired):
    data = copies_input(510 + paired, paired)
    r, outs = cli(exe, tmp_path, data, env={**hamming(), **ALL, "FQD_FAST_KEEP": "best"})
    check_run(r, outs, data, False, paired, expect=lambda owner: sizes.dedup_sized(data, False, best=True, keys=owner))
    assert [read_out(o) for o in outs] != sizes.dedup_sized(data, False, keys=statement(data, False)[0])[0]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_abundance_order_and_the_filter_read_the_merged_clusters(exe, tmp_path, paired):
    data = copies_input(520 + paired, paired)
    owner, nodes, merged = statement(data, False)
    exp_out, gone, gone_records, written = order_ref.dedup_ordered(data, keys=owner, by_size=True, lo=2, sizeout=True)
    assert gone > 20 and written == sorted(written, reverse=True) and written[0] > 2
    r, outs = cli(exe, tmp_path, data, gz_out=True, env={**hamming(), "FQD_FAST_SIZEOUT": "1", "FQD_FAST_SORT": "size", "FQD_FAST_MINSIZE": "2"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(len(owner), len(owner) - merged, paired) + second_line(nodes - merged, paired) + order_ref.not_written_line(gone, gone_records, paired, 2, None)
    assert [read_out(o) for o in outs] == exp_out


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_annotated_sizes_add_up_over_the_merged_clusters(exe, tmp_path, paired):
    data = copies_input(530 + paired, paired, sizein=True)
    owner, nodes, merged = statement(data, False)
    exp_out, exp_levels, total, dups, _, _, _ = sizein.dedup_weighted(data, keys=owner)
    r, outs = cli(exe, tmp_path, data, env={**hamming(), "FQD_FAST_SIZEOUT": "1", "FQD_FAST_LEVELS": "1", "FQD_FAST_SIZEIN": "1"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, total - merged, paired) + second_line(nodes - merged, paired)
    assert [read_out(o) for o in outs] == exp_out and levels_of(outs[0]).read_bytes() == exp_levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_optical_distance_splits_the_merged_clusters(exe, tmp_path, paired):
    data = copies_input(540 + paired, paired)
    owner, nodes, merged = statement(data, False)
    places = []
    for rec in fast.parse(data[0], False):
        reason, tile, x, y, surface = optical_ref.parse(rec[1])
        assert reason == optical_ref.OK
        places.append((surface, tile, x, y))
    split, info = optical_ref.split(owner, places, PIXELS)
    split = [int(o) for o in split]
    assert info["clusters_in"] == merged and info["clusters_out"] > merged + 20
    # a merged cluster of several sequences that the places cut: not what either switch makes alone
    exact = [int(o) for o in ref.exact_owners([tuple(f[i][2] for f in [fast.parse(x, False) for x in data]) for i in range(len(owner))])]
    assert split != [int(o) for o in optical_ref.split(exact, places, PIXELS)[0]] and split != owner
    exp_out, exp_levels, total, dups, _, exp_clusters = sizes.dedup_sized(data, False, keys=split)
    r, outs = cli(exe, tmp_path, data, kind="bgzf", env={**hamming(), **ALL, "FQD_FAST_OPTICAL": str(PIXELS)})
    assert r.returncode == 0, r.stderr
    more = info["clusters_out"] - merged
    assert r.stdout == (verbose_line(total, total - info["clusters_out"], paired) + second_line(nodes - merged, paired) +
                        f"{more} {'read pairs' if paired else 'reads'} that repeat an earlier sequence were written: not optical duplicates (FQD_FAST_OPTICAL={PIXELS}).\n")
    assert [read_out(o) for o in outs] == exp_out
    assert [clusters_of(o).read_bytes() for o in outs] == exp_clusters
    assert levels_of(outs[0]).read_bytes() == exp_levels


@pytest.mark.gpu
def test_the_edge_list_regrows_in_a_run(exe, tmp_path):
    data = copies_input(550, False)
    r, outs = cli(exe, tmp_path, data, env={**hamming(), **ALL, "FQD_NEAR_EDGE_ROOM": "3"})
    check_run(r, outs, data, False, False)


@pytest.mark.gpu
@pytest.mark.parametrize("paired,fasta,kind,gz_out", [(False, False, "plain", False), (True, False, "bgzf", True), (False, True, "gzip", False)])
def test_unset_and_zero_give_the_default_bytes(exe, tmp_path, paired, fasta, kind, gz_out):
    data = copies_input(560 + paired, paired, fasta)
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, tag="d", fasta=fasta)
    rz, outsz = cli(exe, tmp_path, data, kind, gz_out, env={**hamming(0), "FQD_HOST_TIMING": "1"}, tag="z", fasta=fasta)
    assert r0.returncode == 0 and rz.returncode == 0 and r0.stdout == rz.stdout, r0.stderr + rz.stderr
    assert "substitutions" not in rz.stderr
    for a, b in zip(outs0, outsz):
        assert a.read_bytes() == b.read_bytes()
    # the exact duplicates alone, as the default run counts them
    total = len(fast.parse(data[0], fasta))
    assert r0.stdout == verbose_line(total, total - statement(data, fasta)[1], paired)
    # set, the same input loses more
    r1, outs1 = cli(exe, tmp_path, data, kind, gz_out, env=hamming(3), tag="m", fasta=fasta)
    assert r1.returncode == 0 and [read_out(o) for o in outs1] == sizes.dedup_sized(data, fasta, keys=statement(data, fasta, 3)[0])[4]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_empty_inputs(exe, tmp_path, paired):
    data = [b""] * (2 if paired else 1)
    r0, outs0 = cli(exe, tmp_path, data, tag="d")
    r, outs = cli(exe, tmp_path, data, env=hamming())
    assert (r.returncode, r.stdout, r.stderr) == (r0.returncode, r0.stdout, r0.stderr)
    for a, b in zip(outs0, outs):
        assert a.exists() == b.exists() and (not a.exists() or a.read_bytes() == b.read_bytes())


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_a_seed_group_beyond_the_limit_ends_the_run_before_any_output(exe, tmp_path, paired):
    rng = random.Random(580 + paired)
    records = group_records(rng, D, ref.MAX_GROUP + 1, paired=paired)
    records = records[:60] + records[10:30] + records[60:]       # copies do not count
    lowest, entries = ref.over_limit(records, D)
    assert entries == ref.MAX_GROUP + 1
    data = ["".join(f"@r{k} {m + 1}\n{r[m].decode()}\n+\n{'I' * len(r[m])}\n" for k, r in enumerate(records)).encode() for m in range(2 if paired else 1)]
    r, outs = cli(exe, tmp_path, data, env={**hamming(), **ALL})
    assert r.returncode == 1
    assert (f"FQD_FAST_HAMMING={D}: {entries} different sequences, the one of record {lowest} (counted from 0) of " in r.stderr and
            f"share one of the {D + 1} segments their first mate is cut into; a group of at most {ref.MAX_GROUP} is compared" in r.stderr and "trim" in r.stderr)
    assert "ina0.fq" in r.stderr                                 # the file is named
    assert nothing_written(outs)
    # exactly the limit is merged
    records = group_records(rng, D, ref.MAX_GROUP, paired=paired)
    data = ["".join(f"@r{k} {m + 1}\n{r[m].decode()}\n+\n{'I' * len(r[m])}\n" for k, r in enumerate(records)).encode() for m in range(2 if paired else 1)]
    r, outs = cli(exe, tmp_path, data, env=hamming(), tag="l")
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(ref.MAX_GROUP, 1, paired) + second_line(1, paired)
