"""FQD_FAST_OPTICAL=D of the `--fast` mode through the CLI.  CPU part: what the switch's value and the command line decide,
before any GPU call, and the new FastModes field in a small native harness (tests/native/fast_optical_check.cpp).  GPU part,
on inputs of fragments x PCR copies x optical copies with Illumina names, 200 .. 2 000 records — FASTQ and FASTA, plain,
BGZF and ordinary gzip, single-end and paired: the outputs, `.clusters`, `;size=N`, `.duplevels` and both `-v` lines are
those of tests/size_reference.py fed the groups of the sequential statement (tests/optical_reference.py), alone and
combined with the other switches; a D that keeps every cluster whole gives the default run's bytes; copies that all sit on
different tiles give the input back; a malformed name and a cluster above the cap end the run before any output."""
import os
import random
import subprocess
from pathlib import Path

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib
import fast_keep_reference as fast
import optical_reference as ref
import size_order_reference as order_ref
import size_reference as sizes
import sizein_reference as sizein
import strand_reference as strand
import umi_merge_reference as umi_merge
import umi_reference as umi
import test_fast_sizes_cli as base                            # its file helpers
import test_fast_umi_cli as inputs                            # PACK

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
SWITCHES = base.SWITCHES + ("FQD_FAST_OPTICAL", "FQD_FAST_SIZEIN", "FQD_FAST_SORT", "FQD_FAST_MINSIZE", "FQD_FAST_MAXSIZE", "FQD_FAST_UMI_MISMATCH")
NO_GPU = base.NO_GPU
ALL = {"FQD_FAST_SIZEOUT": "1", "FQD_FAST_LEVELS": "1", "FQD_FAST_CLUSTERS": "1"}
read_out, levels_of, clusters_of, nothing_written, verbose_line = base.read_out, base.levels_of, base.clusters_of, base.nothing_written, base.verbose_line
D = 100


def optical(d=D):
    return {"FQD_FAST_OPTICAL": str(d)}


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


def flowcell_input(seed, paired, fasta=False, fragments=150, behind="", tiles=(1101, 1102, 2101), turned=False, umi_errors=False):
    """Fragments x PCR copies x optical copies, shuffled.  A PCR copy lands anywhere on one of the tiles; its optical copies
    within D / 2 of it, now and then chained a little further.  behind: what follows y in the first word — "" nothing,
    "colon" / "underscore" a UMI of the copy's molecule as 8th field / behind '_', "sizein" an 8th field with `;size=N`.
    Returns (files, one (sequence(s), UMI) per record)."""
    rng = random.Random(seed)
    records = []
    for _ in range(fragments):
        seqs = tuple("".join(rng.choice("ACGT") for _ in range(rng.randrange(60, 101))) for _ in range(2 if paired else 1))
        for _ in range(rng.choice([1, 1, 2, 3])):              # molecules of the fragment (UMIs)
            u = "".join(rng.choice("ACGT") for _ in range(6))
            for _ in range(rng.choice([1, 1, 1, 2, 4])):       # PCR copies
                tile, x, y = rng.choice(tiles), rng.randrange(1000, 30000), rng.randrange(1000, 30000)
                for k in range(rng.choice([1, 1, 1, 2, 3, 5])):  # optical copies
                    uu = u
                    if umi_errors and rng.random() < 0.2:
                        at = rng.randrange(6)
                        uu = u[:at] + rng.choice("ACGT") + u[at + 1:]
                    records.append((seqs, uu, tile, x, y))
                    x, y = x + rng.randrange(-D // 2, D // 2 + 1), y + rng.randrange(-D // 2, D // 2 + 1)
    rng.shuffle(records)
    lead = ">" if fasta else "@"
    files = []
    for m in range(2 if paired else 1):
        out = []
        for k, (seqs, u, tile, x, y) in enumerate(records):
            s = seqs[m]
            if turned and k % 2:
                s = strand.rc(seqs[0].encode()).decode() if not paired else seqs[1 - m]
            tail = {"": "", "colon": f":{u}", "underscore": f"_{u}", "sizein": f":n{k};size={1 + k % 7}"}[behind]
            head = f"{lead}M01:7:FC1:{1 + (k % 50 == 0)}:{tile}:{x}:{y}{tail} {m + 1}:N:0:ACGT\n"
            out.append(f"{head}{s}\n" if fasta else f"{head}{s}\n+\n{''.join(chr(rng.randrange(40, 74)) for _ in s)}\n")
        files.append("".join(out).encode())
    return files


def statement(data, fasta, keys=None, d=D):
    """The optical groups of the clusters that `keys` make (default: the sequences): (owner per record, clusters before,
    clusters behind the split)."""
    files = [fast.parse(x, fasta) for x in data]
    n = len(files[0])
    if keys is None:
        keys = [tuple(f[i][2] for f in files) for i in range(n)]
    first = {}
    owner = [first.setdefault(k, i) for i, k in enumerate(keys)]
    places = []
    for i in range(n):
        reason, tile, x, y, surface = ref.parse(files[0][i][1])
        assert reason == ref.OK
        places.append((surface, tile, x, y))
    out, info = ref.split(owner, places, d)
    return [int(o) for o in out], info["clusters_in"], info["clusters_out"]


def second_line(more, paired, d=D):
    return f"{more} {'read pairs' if paired else 'reads'} that repeat an earlier sequence were written: not optical duplicates (FQD_FAST_OPTICAL={d}).\n"


# ---------------------------------------------------------------- CPU: decided before any GPU call

@pytest.mark.parametrize("value", ["-1", "x", "", "1.5", "2147483648", "99999999999", "1 ", "+5", "0x10"])
def test_a_bad_value_is_refused(exe, tmp_path, value):
    r, outs = cli(exe, tmp_path, flowcell_input(1, False, fragments=4), env={**NO_GPU, **optical(value)})
    assert r.returncode == 1
    assert "FQD_FAST_OPTICAL must be a decimal integer in 1 .. 2147483647" in r.stderr and f"'{value}'" in r.stderr
    assert nothing_written(outs)


def test_unordered_and_several_devices_are_refused_by_name(exe, tmp_path):
    r, outs = cli(exe, tmp_path, flowcell_input(2, True, fragments=4), env={**NO_GPU, **optical(2500)}, extra=["--unordered"])
    assert r.returncode == 1 and r.stderr.count("FQD_FAST_OPTICAL=2500") == 1 and "--unordered" in r.stderr
    assert nothing_written(outs)
    r, outs = cli(exe, tmp_path, flowcell_input(2, False, fragments=4), env={**NO_GPU, **optical(2147483647), "FQD_DEVICES": "0,1"})
    assert r.returncode == 1 and r.stderr.count("FQD_FAST_OPTICAL=2147483647") == 1 and "FQD_DEVICES" in r.stderr
    assert nothing_written(outs)
    r, outs = cli(exe, tmp_path, flowcell_input(2, False, fragments=4), env={**NO_GPU, **optical(7), "FQD_FAST_KEEP": "best", "FQD_ORDERED_RESIDENT": "0"})
    assert r.returncode == 1 and "FQD_FAST_KEEP=best and FQD_FAST_OPTICAL=7" in r.stderr and "FQD_ORDERED_RESIDENT" in r.stderr
    assert nothing_written(outs)


@pytest.mark.parametrize("value", [None, "0", "000"])
def test_zero_and_unset_are_off(exe, tmp_path, value):
    # off: `--unordered` is not refused by the switch's name (without a GPU the run then ends for that reason)
    env = {**NO_GPU, **({} if value is None else optical(value))}
    r, _ = cli(exe, tmp_path, flowcell_input(3, True, fragments=4), env=env, extra=["--unordered"])
    assert "FQD_FAST_OPTICAL" not in r.stderr


@pytest.fixture(scope="module")
def modes_harness():
    target = HERE / "native" / "fast_optical_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "include"), "-o", str(target), str(HERE / "native" / "fast_optical_check.cpp"),
                    str(ROOT / "fastq-dupaway_amd" / "host" / "fast_modes.cpp")], check=True, capture_output=True)
    return str(target)


def modes(harness, env, *args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("FQD_")}
    e.update(env)
    r = subprocess.run([harness, *args], capture_output=True, text=True, env=e, timeout=60)
    assert r.returncode == 0, r.stderr
    return dict(line.split(" ", 1) if " " in line else (line, "") for line in r.stdout.splitlines())


def test_the_field_of_fast_modes(modes_harness):
    off = modes(modes_harness, {})
    assert (off["optical"], off["linked"], off["any"], off["names"]) == ("0", "0", "0", "") and "OPTICAL" not in off["note"]
    assert modes(modes_harness, optical(0)) == off and modes(modes_harness, optical("00")) == off      # byte for byte the unset switch's
    on = modes(modes_harness, optical(2500))
    assert (on["optical"], on["linked"], on["any"], on["names"], on["check"]) == ("2500", "1", "1", "FQD_FAST_OPTICAL=2500", "passed")
    assert on["note"].startswith(off["note"]) and "FQD_FAST_OPTICAL takes 16 bytes a record" in on["note"][len(off["note"]):]
    assert "fewer than 7 fields" in on["reason"]
    both = modes(modes_harness, {**optical(1), "FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1", "FQD_FAST_SIZEOUT": "1"})
    assert both["names"] == "FQD_FAST_UMI=colon and FQD_FAST_UMI_MISMATCH=1 and FQD_FAST_OPTICAL=1 and FQD_FAST_SIZEOUT=1"
    assert modes(modes_harness, optical(2147483647))["optical"] == "2147483647"
    assert "refusal" in modes(modes_harness, optical(5), "1") and "--unordered" in modes(modes_harness, optical(5), "1")["refusal"]
    assert "FQD_DEVICES" in modes(modes_harness, optical(5), "0", "2")["refusal"]
    for bad in ("2147483648", "-3", "", "7x"):
        assert "FQD_FAST_OPTICAL must be a decimal integer in 1 .. 2147483647" in modes(modes_harness, optical(bad))["error"]


def test_the_inputs_of_these_tests():
    for paired in (False, True):
        data = flowcell_input(4, paired)
        owner, before, behind = statement(data, False)
        n = len(owner)
        assert 200 <= n <= 2000 and before < behind < n - 50 and behind - before > 30


# ---------------------------------------------------------------- GPU

CASES = base.CASES


def check_run(r, outs, data, fasta, paired, keys, expect=None, d=D):
    """The run's two `-v` lines, outputs with labels, cluster files and level table against size_reference fed the groups."""
    owner, before, behind = statement(data, fasta, keys, d)
    exp_out, exp_levels, total, dups, _, exp_clusters = expect(owner) if expect else sizes.dedup_sized(data, fasta, keys=owner)
    assert dups == total - behind
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired) + second_line(behind - before, paired, d)
    assert [read_out(o) for o in outs] == exp_out
    assert [clusters_of(o).read_bytes() for o in outs] == exp_clusters
    assert levels_of(outs[0]).read_bytes() == exp_levels
    return before, behind


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{'pe' if c[0] else 'se'}-{'fasta' if c[1] else 'fastq'}-{c[2]}-to-{'gz' if c[3] else 'plain'}" for c in CASES])
def test_only_optical_duplicates_are_removed(exe, tmp_path, case):
    paired, fasta, kind, gz_out = case
    data = flowcell_input(400 + CASES.index(case), paired, fasta)
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**optical(), **ALL, "FQD_HOST_TIMING": "1"}, fasta=fasta)
    before, behind = check_run(r, outs, data, fasta, paired, None)
    assert f"fast: optical duplicates within {D} pixels, " in r.stderr and f" of {before} clusters split, {behind - before} more written, " in r.stderr
    # without the labels: the records as they stand
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env=optical(), tag="p", fasta=fasta)
    assert r.returncode == 0 and [read_out(o) for o in outs] == sizes.dedup_sized(data, fasta, keys=statement(data, fasta)[0])[4]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_best_copy_of_an_optical_group_is_written(exe, tmp_path, paired):
    data = flowcell_input(410 + paired, paired)
    r, outs = cli(exe, tmp_path, data, env={**optical(), **ALL, "FQD_FAST_KEEP": "best"})
    check_run(r, outs, data, False, paired, None, expect=lambda owner: sizes.dedup_sized(data, False, best=True, keys=owner))
    assert [read_out(o) for o in outs] != sizes.dedup_sized(data, False, keys=statement(data, False)[0])[0]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_both_strands_make_the_clusters_that_are_split(exe, tmp_path, paired):
    data = flowcell_input(420 + paired, paired, turned=True)
    files = [fast.parse(x, False) for x in data]
    keys = [strand.canon_key(files[0][i][2] if not paired else (files[0][i][2], files[1][i][2])) for i in range(len(files[0]))]
    assert statement(data, False, keys)[1] < statement(data, False)[1]
    r, outs = cli(exe, tmp_path, data, kind="bgzf", env={**optical(), **ALL, "FQD_FAST_STRAND": "both"})
    check_run(r, outs, data, False, paired, keys)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,paired", [("colon", False), ("colon", True), ("underscore", False), ("underscore", True)])
def test_umis_make_the_clusters_that_are_split(exe, tmp_path, mode, paired):
    data = flowcell_input(430 + paired, paired, behind=mode)
    files = [fast.parse(x, False) for x in data]
    sep = b":" if mode == "colon" else b"_"
    keys = [umi.key_of(files[0][i][1], sep, *(f[i][2] for f in files)) for i in range(len(files[0]))]
    assert statement(data, False, keys)[1] > statement(data, False)[1]
    r, outs = cli(exe, tmp_path, data, env={**optical(), **ALL, "FQD_FAST_UMI": mode})
    check_run(r, outs, data, False, paired, keys)


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_merged_umis_make_the_clusters_that_are_split(exe, tmp_path, paired):
    data = flowcell_input(440 + paired, paired, behind="colon", umi_errors=True)
    files = [fast.parse(x, False) for x in data]
    n = len(files[0])
    umis = [umi.key_of(files[0][i][1], b":")[0] for i in range(n)]
    merged, info, *_ = umi_merge.merge(umis, [tuple(f[i][2] for f in files) for i in range(n)], 1, 4096)
    assert info["merged"] > 10
    r, outs = cli(exe, tmp_path, data, env={**optical(), **ALL, "FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1"})
    check_run(r, outs, data, False, paired, [int(o) for o in merged])


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_abundance_order_and_the_filter_read_the_split_clusters(exe, tmp_path, paired):
    data = flowcell_input(450 + paired, paired)
    owner, before, behind = statement(data, False)
    exp_out, gone, gone_records, written = order_ref.dedup_ordered(data, keys=owner, by_size=True, lo=2, sizeout=True)
    assert gone > 50 and written == sorted(written, reverse=True) and written[0] > 2
    r, outs = cli(exe, tmp_path, data, gz_out=True, env={**optical(), "FQD_FAST_SIZEOUT": "1", "FQD_FAST_SORT": "size", "FQD_FAST_MINSIZE": "2"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(len(owner), len(owner) - behind, paired) + second_line(behind - before, paired) + order_ref.not_written_line(gone, gone_records, paired, 2, None)
    assert [read_out(o) for o in outs] == exp_out


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_annotated_sizes_add_up_over_the_split_clusters(exe, tmp_path, paired):
    data = flowcell_input(460 + paired, paired, behind="sizein")
    owner, before, behind = statement(data, False)
    exp_out, exp_levels, total, dups, _, _, _ = sizein.dedup_weighted(data, keys=owner)
    r, outs = cli(exe, tmp_path, data, env={**optical(), "FQD_FAST_SIZEOUT": "1", "FQD_FAST_LEVELS": "1", "FQD_FAST_SIZEIN": "1"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, total - behind, paired) + second_line(behind - before, paired)
    assert [read_out(o) for o in outs] == exp_out and levels_of(outs[0]).read_bytes() == exp_levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired,fasta,kind,gz_out", [(False, False, "plain", False), (True, False, "bgzf", True), (False, True, "gzip", False)])
def test_a_distance_that_keeps_every_cluster_whole_gives_the_default_bytes(exe, tmp_path, paired, fasta, kind, gz_out):
    data = flowcell_input(470 + paired, paired, fasta, tiles=(1101,))
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, tag="d", fasta=fasta)
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env=optical(2147483647), fasta=fasta)
    assert r0.returncode == 0 and r.returncode == 0, r0.stderr + r.stderr
    total = len(fast.parse(data[0], fasta))
    lane_two = statement(data, fasta, d=2147483647)            # (one record in fifty sits on another lane: those stay apart)
    assert r.stdout == verbose_line(total, total - lane_two[2], paired) + second_line(lane_two[2] - lane_two[1], paired, 2147483647)
    one_lane = [x.replace(b"M01:7:FC1:2:", b"M01:7:FC1:1:") for x in data]
    r0, outs0 = cli(exe, tmp_path, one_lane, kind, gz_out, tag="e", fasta=fasta)
    r, outs = cli(exe, tmp_path, one_lane, kind, gz_out, env=optical(2147483647), tag="f", fasta=fasta)
    assert r0.returncode == 0 and r.returncode == 0, r0.stderr + r.stderr
    assert r.stdout == r0.stdout + second_line(0, paired, 2147483647)
    for a, b in zip(outs0, outs):
        assert a.read_bytes() == b.read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_copies_on_different_tiles_give_the_input_back(exe, tmp_path, paired):
    rng = random.Random(480 + paired)
    seqs = [tuple("".join(rng.choice("ACGT") for _ in range(80)) for _ in range(2 if paired else 1)) for _ in range(40)]
    files = []
    for m in range(2 if paired else 1):
        files.append("".join(f"@M01:7:FC1:1:{1000 + k}:500:500 {m + 1}:N:0\n{seqs[k % 40][m]}\n+\n{'I' * 80}\n" for k in range(400)).encode())
    r, outs = cli(exe, tmp_path, files, env=optical(2147483647))
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(400, 0, paired) + second_line(360, paired, 2147483647)
    assert [read_out(o) for o in outs] == files


REFUSED = [("@M01:7:FC1:1:1101:15589 1:N:0", "fewer than 7 fields"), ("@M01:7:FC1::1101:15589:1332", "is empty"), ("@M01:7:FC1:1:11x1:15589:1332", "no digit"),
           ("@M01:7:FC1:1:1101:1234567890:1332", "more than 9 digits"), ("@M01:7:FC1:1:1101:15589:1332;size=3", "followed by")]


@pytest.mark.gpu
@pytest.mark.parametrize("line,words", REFUSED, ids=["few-fields", "empty-field", "not-digit", "too-long", "bad-end"])
def test_a_malformed_name_ends_the_run_before_any_output(exe, tmp_path, line, words):
    data = flowcell_input(490, True, fragments=30)
    lines = data[0].split(b"\n")
    lines[4 * 7] = line.encode()
    lines[4 * 20] = b"@SRR1.21 21"                            # a second one, behind it: the lowest is named
    data[0] = b"\n".join(lines)
    r, outs = cli(exe, tmp_path, data, kind="bgzf", env={**optical(), **ALL})
    assert r.returncode == 1
    assert f"FQD_FAST_OPTICAL={D}" in r.stderr and "record 7 (counted from 0)" in r.stderr and words in r.stderr
    assert "ina0.fq.gz" in r.stderr                            # the file is named
    assert nothing_written(outs)


@pytest.mark.gpu
def test_a_cluster_above_the_cap_ends_the_run_before_any_output(exe, tmp_path):
    cap = ref.MAX_CLUSTER
    seq, other = "ACGTTGCA" * 5, "TTGACCAG" * 5
    recs = [f"@M01:7:FC1:1:1101:5:5\n{other}\n+\n{'I' * 40}\n"] * 3 + [f"@M01:7:FC1:1:1101:{k}:7\n{seq}\n+\n{'I' * 40}\n" for k in range(cap + 1)]
    r, outs = cli(exe, tmp_path, ["".join(recs).encode()], env={**optical(), **ALL})
    assert r.returncode == 1
    assert f"FQD_FAST_OPTICAL={D}" in r.stderr and "record 3 (counted from 0)" in r.stderr and str(cap + 1) in r.stderr and "trim" in r.stderr
    assert nothing_written(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_empty_inputs_and_zero(exe, tmp_path, paired):
    data = [b""] * (2 if paired else 1)
    r0, outs0 = cli(exe, tmp_path, data, tag="d")
    r, outs = cli(exe, tmp_path, data, env=optical())
    assert (r.returncode, r.stdout, r.stderr) == (r0.returncode, r0.stdout, r0.stderr)
    for a, b in zip(outs0, outs):
        assert a.exists() == b.exists() and (not a.exists() or a.read_bytes() == b.read_bytes())
    data = flowcell_input(495 + paired, paired)
    r0, outs0 = cli(exe, tmp_path, data, kind="bgzf", gz_out=True, tag="e")
    rz, outsz = cli(exe, tmp_path, data, kind="bgzf", gz_out=True, env={**optical(0), "FQD_HOST_TIMING": "1"}, tag="z")
    assert r0.returncode == 0 and rz.returncode == 0 and r0.stdout == rz.stdout, r0.stderr + rz.stderr
    assert "optical" not in rz.stderr
    for a, b in zip(outs0, outsz):
        assert a.read_bytes() == b.read_bytes()
