"""FQD_FAST_SIZEIN=1 of the `--fast` mode through the CLI.  CPU part: what the command line decides, before any GPU call.  GPU
part, on inputs of about 600 records (pairs) — plain, BGZF and ordinary gzip in, plain and `.gz` out, single-end and paired,
FASTA: dereplicating the concatenated `;size=` outputs of an input's two halves gives byte for byte the labelled output of the
whole input, and our own labelled output is reproduced; `<output 1>.duplevels`, the size bounds with their `-v` line and the
abundance order read weighted sizes (tests/sizein_reference.py); the label takes the annotation's place and what follows
stays; FQD_FAST_KEEP=best, FQD_FAST_STRAND=both and FQD_FAST_UMI / FQD_FAST_UMI_MISMATCH compose; malformed annotations,
mates that differ and a cluster above 2^31-1 end the run before any output; empty inputs and `0` behave as documented."""
import os
import random
import subprocess

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib
import fast_keep_reference as fast
import size_reference as sizes
import size_order_reference as order_ref
import sizein_reference as ref
import strand_reference as strand
import test_fast_sizes_cli as base                            # its small inputs and file helpers
import test_fast_umi_cli as inputs                            # PACK

SWITCHES = base.SWITCHES + ("FQD_FAST_SIZEIN", "FQD_FAST_SORT", "FQD_FAST_MINSIZE", "FQD_FAST_MAXSIZE", "FQD_FAST_UMI_MISMATCH")
NO_GPU = base.NO_GPU
SIZEIN, SIZEOUT, LEVELS = {"FQD_FAST_SIZEIN": "1"}, {"FQD_FAST_SIZEOUT": "1"}, {"FQD_FAST_LEVELS": "1"}
read_out, levels_of, clusters_of, nothing_written, verbose_line = base.read_out, base.levels_of, base.clusters_of, base.nothing_written, base.verbose_line


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


def annotated_input(seed, paired, fasta=False, n=600, distinct=False):
    """n records (pairs) of 100 .. 150 bases, most of them copies of an earlier one (distinct: about a fifth); about two thirds
    carry `;size=N` in file 1, followed by the word's end, `;` or `;ee=0.5`; file 2 says the same, or nothing."""
    rng = random.Random(seed)
    frags = []
    for k in range(n):
        if k and rng.random() < (0.2 if distinct else 0.7):
            frags.append(rng.choice(frags))
        else:
            frags.append(tuple("".join(rng.choice("ACGT") for _ in range(rng.randrange(100, 151))) for _ in range(2 if paired else 1)))
    weights = [rng.choice([1, 2, 3, 9, 10, 48, 120, 5000, 12345]) if rng.random() < 0.66 else None for _ in range(n)]
    lead = ">" if fasta else "@"
    files = []
    for m in range(2 if paired else 1):
        recs = []
        for k, f in enumerate(frags):
            w = weights[k]
            note = "" if w is None else f";size={w}" + ["", ";", ";ee=0.5"][k % 3]
            if m == 1 and k % 4 == 0:
                note = "" if w is not None or k % 8 else ";size=1"       # file 2: nothing, or 1 where file 1 has none
            head = f"{lead}read{k}{note}{['', ' ', chr(9)][k % 3]}{'' if k % 3 == 0 else f'{m + 1}:N:0'}\n"
            s = f[m]
            recs.append(f"{head}{s}\n" if fasta else f"{head}{s}\n+\n{''.join(chr(rng.randrange(40, 74)) for _ in s)}\n")
        files.append("".join(recs).encode())
    return files


def halves(data, fasta):
    per = 2 if fasta else 4
    out = ([], [])
    for x in data:
        lines = x.split(b"\n")[:-1]
        cut = len(lines) // per // 2 * per
        out[0].append(b"".join(y + b"\n" for y in lines[:cut]))
        out[1].append(b"".join(y + b"\n" for y in lines[cut:]))
    return out


# ---------------------------------------------------------------- CPU: decided before any GPU call

def test_the_switch_alone_is_refused(exe, tmp_path):
    for extra_env in ({}, {"FQD_FAST_MINSIZE": "1"}, {"FQD_FAST_SORT": "input"}, {"FQD_FAST_SIZEOUT": "0"}):
        r, outs = cli(exe, tmp_path, annotated_input(1, False, n=12), env={**NO_GPU, **SIZEIN, **extra_env})
        assert r.returncode == 1
        assert all(name in r.stderr for name in ("FQD_FAST_SIZEIN=1", "FQD_FAST_SIZEOUT", "FQD_FAST_LEVELS", "FQD_FAST_SORT=size", "FQD_FAST_MINSIZE", "FQD_FAST_MAXSIZE"))
        assert nothing_written(outs)


@pytest.mark.parametrize("env", [SIZEOUT, LEVELS, {"FQD_FAST_SORT": "size"}, {"FQD_FAST_MAXSIZE": "7"}], ids=["sizeout", "levels", "sort", "maxsize"])
def test_unordered_and_several_devices_are_refused_by_name(exe, tmp_path, env):
    r, outs = cli(exe, tmp_path, annotated_input(2, True, n=12), env={**NO_GPU, **SIZEIN, **env}, extra=["--unordered"])
    assert r.returncode == 1 and r.stderr.count("FQD_FAST_SIZEIN=1") == 1 and "--unordered" in r.stderr
    assert nothing_written(outs)
    r, outs = cli(exe, tmp_path, annotated_input(2, False, n=12), env={**NO_GPU, **SIZEIN, **env, "FQD_DEVICES": "0,1"})
    assert r.returncode == 1 and r.stderr.count("FQD_FAST_SIZEIN=1") == 1 and "FQD_DEVICES" in r.stderr
    assert nothing_written(outs)
    r, outs = cli(exe, tmp_path, annotated_input(2, False, n=12), env={**NO_GPU, **SIZEIN, **env, "FQD_ORDERED_RESIDENT": "0"})
    assert r.returncode == 1 and r.stderr.count("FQD_FAST_SIZEIN=1") == 1 and "FQD_ORDERED_RESIDENT" in r.stderr
    assert nothing_written(outs)


def test_the_inputs_of_these_tests():
    for paired in (False, True):
        data = annotated_input(3, paired)
        out, levels, total, dups, gone, gone_records, written = ref.dedup_weighted(data)
        plain = sizes.dedup_sized(data)
        assert total == 600 and dups > 200 and levels != plain[1] and max(written) > 10000
        assert sum(written) > 50 * total                       # the weights, not the records


# ---------------------------------------------------------------- GPU

CASES = base.CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{'pe' if c[0] else 'se'}-{'fasta' if c[1] else 'fastq'}-{c[2]}-to-{'gz' if c[3] else 'plain'}" for c in CASES])
def test_pooled_halves_give_the_whole_inputs_labels(exe, tmp_path, case):
    paired, fasta, kind, gz_out = case
    data = base.small_input(300 + CASES.index(case), paired, fasta)
    expect, _, total, dups, _, _ = sizes.dedup_sized(data, fasta)
    assert dups > 100
    pool = [b"", b""][:len(data)]
    for tag, half in zip("xy", halves(data, fasta)):
        r, outs = cli(exe, tmp_path, half, env=SIZEOUT, tag=tag, fasta=fasta)
        assert r.returncode == 0, r.stderr
        pool = [p + read_out(o) for p, o in zip(pool, outs)]
    n_pool = len(fast.parse(pool[0], fasta))
    assert total - dups < n_pool < total                       # clusters that both halves hold stand twice in the pool
    rw, outs_w = cli(exe, tmp_path, data, kind, gz_out, env=SIZEOUT, tag="w", fasta=fasta)
    r, outs = cli(exe, tmp_path, pool, kind, gz_out, env={**SIZEIN, **SIZEOUT, **LEVELS, "FQD_HOST_TIMING": "1"}, fasta=fasta)
    assert rw.returncode == 0 and r.returncode == 0, rw.stderr + r.stderr
    assert r.stdout == verbose_line(n_pool, n_pool - (total - dups), paired)      # the first `-v` line counts the file's records
    for j, o in enumerate(outs):
        assert read_out(o) == read_out(outs_w[j]) == expect[j]      # byte for byte the labelled output of the whole input
    assert levels_of(outs[0]).read_bytes() == sizes.dedup_sized(data, fasta)[1]
    assert f"fast: size annotations, {n_pool} of {n_pool} records annotated, total weight {total}\n" in r.stderr
    # the same pool without the switch: every record counts once and carries two labels
    r2, outs2 = cli(exe, tmp_path, pool, kind, gz_out, env=SIZEOUT, tag="n", fasta=fasta)
    assert r2.returncode == 0, r2.stderr
    assert read_out(outs2[0]) != expect[0] and read_out(outs2[0]).count(b";size=") == 2 * (total - dups)
    assert "size annotations" not in r2.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("paired,fasta,kind,gz_out", [(False, False, "plain", False), (True, False, "bgzf", True), (False, True, "gzip", False)])
def test_our_own_output_is_reproduced(exe, tmp_path, paired, fasta, kind, gz_out):
    data = annotated_input(310 + int(paired), paired, fasta)
    first = ref.dedup_weighted(data, fasta)[0]
    r1, outs1 = cli(exe, tmp_path, data, kind, gz_out, env={**SIZEIN, **SIZEOUT}, tag="f", fasta=fasta)
    assert r1.returncode == 0, r1.stderr
    once = [read_out(o) for o in outs1]
    assert once == first
    r2, outs2 = cli(exe, tmp_path, once, kind, gz_out, env={**SIZEIN, **SIZEOUT}, tag="g", fasta=fasta)
    assert r2.returncode == 0, r2.stderr
    assert [read_out(o) for o in outs2] == once
    n_once = len(fast.parse(once[0], fasta))
    assert r2.stdout == verbose_line(n_once, 0, paired)


@pytest.mark.gpu
@pytest.mark.parametrize("paired,fasta,kind,gz_out", [(False, False, "plain", False), (True, False, "gzip", True), (True, True, "bgzf", False)])
def test_levels_bounds_and_order_read_weighted_sizes(exe, tmp_path, paired, fasta, kind, gz_out):
    data = annotated_input(320 + int(paired) + 2 * int(fasta), paired, fasta)
    _, exp_levels, total, dups, _, _, _ = ref.dedup_weighted(data, fasta)
    plain_levels = sizes.dedup_sized(data, fasta)[1]
    assert exp_levels != plain_levels
    # the table, the records as they stand (stale annotations stay without FQD_FAST_SIZEOUT)
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**SIZEIN, **LEVELS}, tag="l", fasta=fasta)
    assert r.returncode == 0 and r.stdout == verbose_line(total, dups, paired), r.stderr
    assert levels_of(outs[0]).read_bytes() == exp_levels
    assert [read_out(o) for o in outs] == fast.dedup(data, fasta)[0]
    ru, outsu = cli(exe, tmp_path, data, kind, gz_out, env=LEVELS, tag="u", fasta=fasta)
    assert ru.returncode == 0 and levels_of(outsu[0]).read_bytes() == plain_levels
    # the bounds and their `-v` line
    lo, hi = 10, 6000
    exp_out, _, _, _, gone, gone_records, written = ref.dedup_weighted(data, fasta, lo=lo, hi=hi)
    unweighted = order_ref.dedup_ordered(data, fasta, lo=lo, hi=hi, sizeout=True)
    assert gone > 20 and any(s > hi for s in ref.dedup_weighted(data, fasta)[6]) and written and exp_out != unweighted[0]
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**SIZEIN, **SIZEOUT, "FQD_FAST_MINSIZE": str(lo), "FQD_FAST_MAXSIZE": str(hi)}, tag="b", fasta=fasta)
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired) + order_ref.not_written_line(gone, gone_records, paired, lo, hi)
    assert [read_out(o) for o in outs] == exp_out
    # the abundance order
    exp_sorted, _, _, _, _, _, written = ref.dedup_weighted(data, fasta, by_size=True)
    assert written == sorted(written, reverse=True) and exp_sorted != order_ref.dedup_ordered(data, fasta, by_size=True, sizeout=True)[0]
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**SIZEIN, **SIZEOUT, "FQD_FAST_SORT": "size"}, tag="s", fasta=fasta)
    assert r.returncode == 0 and r.stdout == verbose_line(total, dups, paired), r.stderr
    assert [read_out(o) for o in outs] == exp_sorted
    # the order alone, without labels: the records as they stand, in weighted order
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**SIZEIN, "FQD_FAST_SORT": "size", "FQD_FAST_MINSIZE": str(lo)}, tag="t", fasta=fasta)
    assert r.returncode == 0, r.stderr
    assert [read_out(o) for o in outs] == ref.dedup_weighted(data, fasta, by_size=True, lo=lo, sizeout=False)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("paired,gz_out", [(False, False), (True, True)])
def test_the_label_stands_where_the_annotation_stood_in_many_small_windows(exe, tmp_path, paired, gz_out):
    data = annotated_input(330 + int(paired), paired, distinct=True)
    exp_out, exp_levels, total, dups, _, _, _ = ref.dedup_weighted(data)
    assert dups > 50 and len(exp_out[0]) > 20 * 5120           # more than twenty windows of 4 KiB (5 KiB at the most)
    assert exp_out[0].count(b";ee=0.5") > 50 and exp_out[0].count(b";\n") + exp_out[0].count(b"; ") + exp_out[0].count(b";\t") > 50
    assert b";size=3;ee=0.5" in data[0] and all(x.count(b";size=") == total - dups for x in exp_out)       # one label a record
    r, outs = cli(exe, tmp_path, data, gz_out=gz_out, env={**SIZEIN, **SIZEOUT, **LEVELS, "FQD_STREAM_WINDOW_KB": "4"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    assert [read_out(o) for o in outs] == exp_out
    assert levels_of(outs[0]).read_bytes() == exp_levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_best_copy_carries_the_label_at_its_own_annotation(exe, tmp_path, paired):
    data = annotated_input(340 + int(paired), paired)
    exp_out, exp_levels, total, dups, _, _, _ = ref.dedup_weighted(data, best=True)
    assert exp_out != ref.dedup_weighted(data)[0]
    r, outs = cli(exe, tmp_path, data, env={**SIZEIN, **SIZEOUT, **LEVELS, "FQD_FAST_KEEP": "best", "FQD_FAST_CLUSTERS": "1"})
    assert r.returncode == 0 and r.stdout == verbose_line(total, dups, paired), r.stderr
    assert [read_out(o) for o in outs] == exp_out
    assert levels_of(outs[0]).read_bytes() == exp_levels
    assert [clusters_of(o).read_bytes() for o in outs] == fast.dedup(data, best=True)[1]      # original ID lines, old annotations included


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_both_strands_make_the_weighted_clusters(exe, tmp_path, paired):
    data = annotated_input(350 + int(paired), paired)
    files = [fast.parse(x, False) for x in data]
    n = len(files[0])
    rng = random.Random(5)
    turned = [[], []][:len(files)]                            # about half of the records (pairs) as their other strand
    for i in range(n):
        flip = rng.random() < 0.5
        recs = [f[i][0].split(b"\n") for f in files]
        if flip and not paired:
            recs[0][1], recs[0][3] = strand.rc(recs[0][1]), recs[0][3][::-1]
        elif flip:
            (recs[0][1], recs[0][3]), (recs[1][1], recs[1][3]) = (recs[1][1], recs[1][3]), (recs[0][1], recs[0][3])
        for m, r_ in enumerate(recs):
            turned[m].append(b"\n".join(r_))
    data = [b"".join(x) for x in turned]
    files = [fast.parse(x, False) for x in data]
    keys = [strand.canon_key(files[0][i][2] if not paired else (files[0][i][2], files[1][i][2])) for i in range(n)]
    exp_out, exp_levels, total, dups, _, _, _ = ref.dedup_weighted(data, keys=keys)
    assert dups > ref.dedup_weighted(data)[3] > 0
    r, outs = cli(exe, tmp_path, data, env={**SIZEIN, **SIZEOUT, **LEVELS, "FQD_FAST_STRAND": "both"})
    assert r.returncode == 0 and r.stdout == verbose_line(total, dups, paired), r.stderr
    assert [read_out(o) for o in outs] == exp_out
    assert levels_of(outs[0]).read_bytes() == exp_levels


def umi_chain(third, paired):
    """Three annotated records of one sequence under the UMIs AAAA, AAAT, AATT — a chain of single mismatches — standing for
    10, 5 and `third` reads, among a few others."""
    seq, other = "ACGTTGCAAGGCTTAACCGGTTAC" * 4, "TTGACCAGTAGGCATCGATCGGAT" * 4
    recs = [("m1", 10, "AAAA", seq), ("o1", None, "CCCC", other), ("m2", 5, "AAAT", seq), ("m3", third, "AATT", seq), ("o2", 2, "CCCC", other),
            ("o3", None, "GGGG", seq[:-1])]
    files = []
    for m in range(2 if paired else 1):
        text = ""
        for name, w, umi, s in recs:
            s = s if m == 0 else s[::-1]
            text += f"@{name}{'' if w is None else f';size={w}'};umi:{umi} {m + 1}:N:0\n{s}\n+\n{'I' * len(s)}\n"
        files.append(text.encode())
    return files


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_directional_rule_takes_weighted_counts(exe, tmp_path, paired):
    env = {**SIZEIN, **SIZEOUT, "FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1"}
    # 10 / 5 / 3: 10 >= 2 * 5 - 1 and 5 >= 2 * 3 - 1, the chain is one molecule of 18 reads
    r, outs = cli(exe, tmp_path, umi_chain(3, paired), env=env, tag="c")
    assert r.returncode == 0 and r.stdout == verbose_line(6, 3, paired), r.stderr
    for m, o in enumerate(outs):
        heads = [x for x in read_out(o).split(b"\n") if x.startswith(b"@")]
        assert heads == [f"@m1;size=18;umi:AAAA {m + 1}:N:0".encode(), f"@o1;umi:CCCC;size=3 {m + 1}:N:0".encode(), f"@o3;umi:GGGG;size=1 {m + 1}:N:0".encode()]
    # 10 / 5 / 4: 5 < 2 * 4 - 1, the third stays a molecule of its own
    r, outs = cli(exe, tmp_path, umi_chain(4, paired), env=env, tag="d")
    assert r.returncode == 0 and r.stdout == verbose_line(6, 2, paired), r.stderr
    heads = [x for x in read_out(outs[0]).split(b"\n") if x.startswith(b"@")]
    assert heads == [b"@m1;size=15;umi:AAAA 1:N:0", b"@o1;umi:CCCC;size=3 1:N:0", b"@m3;size=4;umi:AATT 1:N:0", b"@o3;umi:GGGG;size=1 1:N:0"]
    # counted as records — 1 / 1 / 1 — every neighbour merges: the weights are what made the difference
    r, outs = cli(exe, tmp_path, umi_chain(4, paired), env={k: v for k, v in env.items() if k != "FQD_FAST_SIZEIN"}, tag="e")
    assert r.returncode == 0 and r.stdout == verbose_line(6, 3, paired), r.stderr
    # exact UMIs: three molecules of 10, 5 and 3
    r, outs = cli(exe, tmp_path, umi_chain(3, paired), env={**SIZEIN, **SIZEOUT, "FQD_FAST_UMI": "colon"}, tag="f")
    assert r.returncode == 0 and r.stdout == verbose_line(6, 1, paired), r.stderr
    assert [x for x in read_out(outs[0]).split(b"\n") if x.startswith(b"@m")] == [b"@m1;size=10;umi:AAAA 1:N:0", b"@m2;size=5;umi:AAAT 1:N:0", b"@m3;size=3;umi:AATT 1:N:0"]


REFUSED = [("@read7;size=0 1:N:0", 0, 7, "size=0"), ("@read7;size=12x", 0, 7, "followed by"), ("@read7;size=", 0, 7, "no digit"),
           ("@read7;size=2147483648", 0, 7, "2147483647"), ("@read7;size=2;size=2", 0, 7, "twice"), ("@read9;size=4 2:N:0", 1, 9, "file 1")]


@pytest.mark.gpu
@pytest.mark.parametrize("line,file,record,words", REFUSED, ids=["zero", "bad-end", "no-digits", "too-large", "twice", "mates-differ"])
def test_a_refused_annotation_ends_the_run_before_any_output(exe, tmp_path, line, file, record, words):
    data = annotated_input(360, True, n=40)
    lines = data[file].split(b"\n")
    assert lines[4 * record].startswith(f"@read{record}".encode())
    lines[4 * record] = line.encode()
    lines[4 * 20] = b"@read20;size=00"                         # a second one, behind it: the lowest is named
    data[file] = b"\n".join(lines)
    if file == 1:
        first = data[0].split(b"\n"); first[4 * record] = f"@read{record};size=3 1:N:0".encode(); data[0] = b"\n".join(first)
    r, outs = cli(exe, tmp_path, data, kind="bgzf", env={**SIZEIN, **SIZEOUT, **LEVELS, "FQD_FAST_CLUSTERS": "1"})
    assert r.returncode == 1
    assert "FQD_FAST_SIZEIN=1" in r.stderr and f"record {record} (counted from 0)" in r.stderr and words in r.stderr
    assert f"in{'a'}{file}.fq.gz" in r.stderr                  # the file is named
    assert nothing_written(outs)


@pytest.mark.gpu
def test_a_cluster_above_the_limit_ends_the_run_before_any_output(exe, tmp_path):
    data = annotated_input(361, False, n=40)
    lines = data[0].split(b"\n")
    lines[4 * 5], lines[4 * 30] = b"@read5;size=2147483647", b"@read30;size=2 c"
    lines[4 * 30 + 1], lines[4 * 30 + 3] = lines[4 * 5 + 1], lines[4 * 5 + 3]      # record 30 is a copy of record 5
    data[0] = b"\n".join(lines)
    first = fast.clusters_of([r[2] for r in fast.parse(data[0], False)])
    owner = next(g[0] for g in first if 5 in g)
    total = sum(ref.annotations([fast.parse(data[0], False)[i][1] for i in g])[0][k] for g in first if 5 in g for k in range(len(g)))
    assert total > ref.MAX
    r, outs = cli(exe, tmp_path, data, env={**SIZEIN, **LEVELS, "FQD_FAST_CLUSTERS": "1"})
    assert r.returncode == 1
    assert "FQD_FAST_SIZEIN=1" in r.stderr and f"record {owner} (counted from 0)" in r.stderr and str(total) in r.stderr
    assert nothing_written(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_empty_inputs(exe, tmp_path, paired):
    data = [b""] * (2 if paired else 1)
    r0, outs0 = cli(exe, tmp_path, data, tag="d")
    r, outs = cli(exe, tmp_path, data, env={**SIZEIN, **SIZEOUT, **LEVELS})
    assert (r.returncode, r.stdout, r.stderr) == (r0.returncode, r0.stdout, r0.stderr)
    for a, b in zip(outs0, outs):
        assert a.exists() == b.exists()
        if a.exists():
            assert a.read_bytes() == b.read_bytes()
    assert levels_of(outs[0]).read_bytes() == sizes.duplevels_text([])


@pytest.mark.gpu
@pytest.mark.parametrize("paired,fasta,kind,gz_out", [(False, False, "plain", False), (True, False, "bgzf", True), (False, True, "gzip", False)])
def test_zero_gives_the_bytes_of_a_run_without_the_switch(exe, tmp_path, paired, fasta, kind, gz_out):
    data = annotated_input(370 + int(paired), paired, fasta)
    exp_out, exp_levels, total, dups, _, _ = sizes.dedup_sized(data, fasta)      # every record counts once, the label goes behind the word
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, env={**SIZEOUT, **LEVELS}, tag="d", fasta=fasta)
    rz, outsz = cli(exe, tmp_path, data, kind, gz_out, env={**SIZEOUT, **LEVELS, "FQD_FAST_SIZEIN": "0", "FQD_HOST_TIMING": "1"}, tag="z", fasta=fasta)
    assert r0.returncode == 0 and rz.returncode == 0, r0.stderr + rz.stderr
    assert r0.stdout == rz.stdout == verbose_line(total, dups, paired)
    assert "size annotations" not in rz.stderr
    for j, (a, b) in enumerate(zip(outs0, outsz)):
        assert a.read_bytes() == b.read_bytes()
        assert read_out(a) == exp_out[j]
    assert levels_of(outsz[0]).read_bytes() == levels_of(outs0[0]).read_bytes() == exp_levels
    assert b";ee=0.5;size=" in exp_out[0]                       # the second label behind the word, as before
