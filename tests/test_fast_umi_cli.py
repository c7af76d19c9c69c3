"""FQD_FAST_UMI=colon|underscore of the `--fast` mode through the CLI.  CPU part: what the switch's value and the command
line decide, before any GPU call.  GPU part: on small FASTQ and FASTA inputs — plain, BGZF and ordinary gzip, single-end and
paired, with hand-placed records of one sequence and different UMIs, and of one UMI and sequence — the outputs are the
ORIGINAL text of the records tests/umi_reference.py keeps and the `-v` line matches; with FQD_FAST_CLUSTERS=1 the cluster
files are the statement's, with FQD_FAST_KEEP=best the best-quality copy of a cluster is written at its own place, with
FQD_FAST_STRAND=both the UMI stands in front of the canonical read (tests/fast_keep_reference.py fed the keys of the
statement); every way a file can be refused ends the run with its message before any output exists; `off` and an unset
switch give the default run's bytes."""
import gzip
import os
import random
import subprocess
from pathlib import Path

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib
import fast_keep_reference as fast
import strand_reference as strand
import umi_reference as ref
from inflate_cases import bgzf

SWITCHES = ("FQD_FAST_UMI", "FQD_FAST_STRAND", "FQD_FAST_KEEP", "FQD_FAST_CLUSTERS", "FQD_ORDERED_RESIDENT", "FQD_DEVICES", "FQD_GUNZIP_DEVICE", "FQD_HOST_TIMING")
NO_GPU = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
MODE = {"colon": b":", "underscore": b"_"}


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


def rand_umi(rng, dual):
    return rand_seq(rng, 4) + b"+" + rand_seq(rng, 4) if dual else rand_seq(rng, 8, "ACGTN")


def molecules(seed, paired, n=600, dual=False, turned=False):
    """[(UMI, mate 1, mate 2 or None)] in input order.  The first records are placed by hand: one sequence under two UMIs
    (two molecules), one UMI and sequence twice (one molecule), one UMI over two sequences, and — turned — a molecule and its
    other strand; the rest draw from pools of UMIs and of fragments, so that every combination occurs."""
    rng = random.Random(seed)

    def fresh(L=None):
        return (rand_seq(rng, L or rng.choice([1, 20, 75, 150, 150, 200]), "ACGTN" if rng.random() < 0.1 else "ACGT"),
                rand_seq(rng, rng.choice([1, 30, 150])) if paired else None)

    def turn(f):
        return (f[1], f[0]) if paired else (strand.rc(f[0]), None)

    f = [fresh(150), fresh(151), fresh(33), fresh(16)]
    u = [rand_umi(rng, dual) for _ in range(4)]
    out = [(u[0], *f[0]), (u[1], *f[0]), (u[0], *f[0]), (u[0], *f[1]), (u[2], *f[2]), (u[2], *f[2]), (u[1], *f[0]), (u[3], *f[3])]
    if turned:
        out += [(u[0], *turn(f[0])), (u[3], *turn(f[1])), (u[3], *f[1]), (u[2], *turn(f[3]))]
    umis = [rand_umi(rng, dual) for _ in range(12)]
    pool = [fresh() for _ in range(n // 6)]
    while len(out) < n:
        g = rng.choice(pool)
        out.append((rng.choice(umis), *(turn(g) if turned and rng.random() < 0.5 else g)))
    out.append((u[1], *f[0]))                                   # and one far behind its first copy
    return out


def id_line(k, umi, mode, fasta, mate):
    lead = ">" if fasta else "@"
    if mode == "colon":
        return f"{lead}A00:7:FC_1:{k}:{umi.decode()} {mate + 1}:N:0:ATCACG\n"
    return f"{lead}r{k}:x_y_{umi.decode()}\tmate_{mate + 1}\n"


def as_text(mols, mode, fasta=False, flat=None, seed=0, umi_in_file_two=True):
    """The files' bytes: one per mate.  File 2 carries the same UMIs, or (umi_in_file_two=False) none at all."""
    rng = random.Random(seed)
    files = []
    for m in range(2 if mols[0][2] is not None else 1):
        recs = []
        for k, (umi, *mates) in enumerate(mols):
            s = mates[m].decode()
            head = id_line(k, umi, mode, fasta, m) if m == 0 or umi_in_file_two else f"{'>' if fasta else '@'}second{k}\n"
            if fasta:
                recs.append(f"{head}{s}\n")
                continue
            lo = rng.choice([33, 40, 60, 70])
            q = flat * len(s) if flat else "".join(chr(rng.randrange(lo, lo + 6)) for _ in range(len(s)))
            recs.append(f"{head}{s}\n+\n{q}\n")
        files.append("".join(recs).encode())
    return files


def restate(inputs, mode, fasta=False, best=False, both=False):
    """tests/fast_keep_reference.py's dedup with the clusters taken over the statement's keys — (UMI bases, sequences), the
    sequences in their canonical form with `both`: (outputs, cluster files, total, duplicates, clusters whose written
    member changed)."""
    files = [fast.parse(x, fasta) for x in inputs]
    n = len(files[0])
    keys = []
    for i in range(n):
        seqs = tuple(f[i][2] for f in files)
        if both:
            c = strand.canon_key(seqs[0] if len(seqs) == 1 else seqs)
            seqs = (c,) if len(files) == 1 else tuple(c)
        keys.append(ref.key_of(files[0][i][1], MODE[mode], *seqs))
    groups = fast.clusters_of(keys)
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
        keep = ref.expected_keep(keys)
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


def umi(mode):
    return {"FQD_FAST_UMI": mode}


# ---------------------------------------------------------------- CPU: decided before any GPU call

@pytest.mark.parametrize("value", ["comma", "", "COLON", "colon ", "1", ":"])
def test_unknown_value_is_refused(exe, tmp_path, value):
    r, outs = cli(exe, tmp_path, as_text(molecules(1, False, n=12), "colon"), env={**NO_GPU, "FQD_FAST_UMI": value})
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_UMI") == 1 and "'off', 'colon' or 'underscore'" in r.stderr
    assert nothing_written(outs)


def test_unordered_is_refused(exe, tmp_path):
    r, outs = cli(exe, tmp_path, as_text(molecules(2, True, n=12), "colon"), env={**NO_GPU, **umi("colon")}, extra=["--unordered"])
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_UMI=colon") == 1 and "--unordered" in r.stderr
    assert nothing_written(outs)


def test_several_devices_are_refused(exe, tmp_path):
    r, outs = cli(exe, tmp_path, as_text(molecules(3, False, n=12), "underscore"), env={**NO_GPU, **umi("underscore"), "FQD_DEVICES": "0,1"})
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_UMI=underscore") == 1 and "FQD_DEVICES" in r.stderr
    assert nothing_written(outs)


def test_resident_run_turned_off_is_refused(exe, tmp_path):
    r, outs = cli(exe, tmp_path, as_text(molecules(4, False, n=12), "colon"), env={**NO_GPU, **umi("colon"), "FQD_ORDERED_RESIDENT": "0"})
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_UMI") == 1 and "FQD_ORDERED_RESIDENT" in r.stderr
    assert nothing_written(outs)


def test_the_hand_placed_records_of_the_statement():
    # of the yardstick: one sequence under two UMIs stays, one UMI and sequence twice goes
    for mode in MODE:
        data = as_text(molecules(5, False, n=20), mode)
        outs, _, total, dups, _ = restate(data, mode)
        kept = [r[1] for r in fast.parse(outs[0], False)]
        lines = [r[1] for r in fast.parse(data[0], False)]
        assert lines[0] in kept and lines[1] in kept and lines[2] not in kept and lines[3] in kept and lines[5] not in kept and lines[6] not in kept
        assert fast.dedup(data)[3] > dups > 0


# ---------------------------------------------------------------- GPU

CASES = [(paired, fasta, kind, gz_out, mode) for paired in (False, True) for fasta, kind, gz_out, mode in
         ((False, "plain", False, "colon"), (False, "bgzf", True, "underscore"), (False, "gzip", False, "colon"), (True, "plain", False, "underscore"),
          (True, "gzip", False, "colon"))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{'pe' if c[0] else 'se'}-{'fasta' if c[1] else 'fastq'}-{c[2]}-to-{'gz' if c[3] else 'plain'}-{c[4]}" for c in CASES])
def test_outputs_clusters_and_the_verbose_line(exe, tmp_path, case):
    paired, fasta, kind, gz_out, mode = case
    k = CASES.index(case)
    data = as_text(molecules(100 + k, paired, dual=k % 2 == 1), mode, fasta, seed=k)
    exp_out, exp_cl, total, dups, _ = restate(data, mode, fasta)
    plain_out, _, _, plain_dups, _ = fast.dedup(data, fasta)
    assert plain_dups > dups > 0                                # one sequence under several UMIs AND true copies
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, tag="d", fasta=fasta)
    assert r0.returncode == 0 and r0.stdout == verbose_line(total, plain_dups, paired), r0.stderr
    assert read_out(outs0[0]) == plain_out[0] != exp_out[0]     # without the switch: the other molecules are dropped
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**umi(mode), "FQD_HOST_TIMING": "1"}, fasta=fasta)
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    assert f"fast: UMI, 8 bases behind the last '{MODE[mode].decode()}' of the first word\n" in r.stderr
    for j, o in enumerate(outs):
        assert read_out(o) == exp_out[j]                        # original text, ID lines and all
        assert not clusters_of(o).exists()
    rc_, outsc = cli(exe, tmp_path, data, kind, gz_out, env={**umi(mode), "FQD_FAST_CLUSTERS": "1"}, tag="c", fasta=fasta)
    assert rc_.returncode == 0, rc_.stderr
    assert rc_.stdout == r.stdout
    for j, o in enumerate(outsc):
        assert read_out(o) == exp_out[j]
        assert clusters_of(o).read_bytes() == exp_cl[j]


@pytest.mark.gpu
def test_file_two_is_not_looked_at(exe, tmp_path):
    mols = molecules(21, True)
    with_umi, without = as_text(mols, "colon", seed=1), as_text(mols, "colon", seed=1, umi_in_file_two=False)
    assert with_umi[0] == without[0] and with_umi[1] != without[1]
    exp_out, _, total, dups, _ = restate(without, "colon")
    r, outs = cli(exe, tmp_path, without, env=umi("colon"))
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, True)
    assert [read_out(o) for o in outs] == exp_out


@pytest.mark.gpu
@pytest.mark.parametrize("paired,fasta,kind,gz_out", [(False, False, "plain", False), (True, False, "bgzf", True), (False, True, "gzip", False)])
def test_off_and_an_unset_switch_give_the_default_bytes(exe, tmp_path, paired, fasta, kind, gz_out):
    data = as_text(molecules(50 + int(paired), paired), "colon", fasta, seed=1)
    plain_out, _, total, plain_dups, _ = fast.dedup(data, fasta)
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, tag="d", fasta=fasta)
    rg, outsg = cli(exe, tmp_path, data, kind, gz_out, env={"FQD_FAST_UMI": "off", "FQD_HOST_TIMING": "1"}, tag="g", fasta=fasta)
    assert r0.returncode == 0 and rg.returncode == 0, r0.stderr + rg.stderr
    assert r0.stdout == rg.stdout == verbose_line(total, plain_dups, paired)
    assert "UMI" not in rg.stderr
    for k, (a, b) in enumerate(zip(outs0, outsg)):
        assert a.read_bytes() == b.read_bytes()
        assert read_out(a) == plain_out[k]


@pytest.mark.gpu
@pytest.mark.parametrize("paired,kind,gz_out,mode", [(False, "plain", False, "underscore"), (True, "bgzf", True, "colon")])
def test_best_copy_of_a_molecule(exe, tmp_path, paired, kind, gz_out, mode):
    data = as_text(molecules(7 + int(paired), paired), mode, seed=3)
    exp_out, exp_cl, total, dups, moved = restate(data, mode, best=True)
    first_out, _, _, _, _ = restate(data, mode)
    assert moved > 0 and exp_out != first_out
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**umi(mode), "FQD_FAST_KEEP": "best", "FQD_FAST_CLUSTERS": "1", "FQD_HOST_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    assert f"fast: best-quality pick, {moved} of {total - dups} clusters changed\n" in r.stderr
    for k, o in enumerate(outs):
        assert read_out(o) == exp_out[k]
        assert clusters_of(o).read_bytes() == exp_cl[k]


@pytest.mark.gpu
@pytest.mark.parametrize("paired,kind,gz_out,mode", [(False, "plain", False, "colon"), (True, "plain", False, "underscore"), (True, "gzip", True, "colon")])
def test_both_strands_under_one_umi(exe, tmp_path, paired, kind, gz_out, mode):
    data = as_text(molecules(30 + int(paired), paired, turned=True), mode, seed=4)
    exp_out, exp_cl, total, dups, _ = restate(data, mode, both=True)
    _, _, _, dups_given, _ = restate(data, mode)
    assert dups > dups_given > 0                                # both strands of one molecule among the records
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**umi(mode), "FQD_FAST_STRAND": "both", "FQD_FAST_CLUSTERS": "1", "FQD_HOST_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired)
    assert "fast: both strands, " in r.stderr and "fast: UMI, 8 bases" in r.stderr
    for k, o in enumerate(outs):
        assert read_out(o) == exp_out[k]
        assert clusters_of(o).read_bytes() == exp_cl[k]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_empty_inputs_give_what_the_default_run_gives(exe, tmp_path, paired):
    # no record, no UMI to look for: the default run's result, whatever it is, and with it
    data = [b""] * (2 if paired else 1)
    r0, outs0 = cli(exe, tmp_path, data, tag="d")
    r, outs = cli(exe, tmp_path, data, env=umi("colon"))
    assert (r.returncode, r.stdout, r.stderr) == (r0.returncode, r0.stdout, r0.stderr)
    for a, b in zip(outs0, outs):
        assert a.exists() == b.exists()
        if a.exists():
            assert a.read_bytes() == b.read_bytes()
        assert not clusters_of(b).exists()


REFUSALS = [
    ("no separator", "colon", 5, b"@READ5 1:N:0:ACGT\n", "record 5", "holds no ':'"),
    ("no separator, underscore", "underscore", 0, b"@READ:ACGTACGT x_y\n", "record 0", "holds no '_'"),
    ("empty", "colon", 7, b"@A00:7: 1:N:0\n", "record 7", "UMI is empty"),
    ("no base", "colon", 64, b"@A00:7:+ 1:N:0\n", "record 64", "UMI has no base"),
    ("too long", "underscore", 3, b"@r3_" + b"ACGT" * 16 + b"A\n", "record 3", "longer than 64 bytes"),
    ("a lower-case byte", "colon", 130, b"@A00:7:ACGTacgt 1:N:0\n", "record 130", "outside ACGTN+-_"),
    ("a digit, as in a read name without a UMI", "colon", 2, b"@A00:7:FC:1101:2000 1:N:0\n", "record 2", "outside ACGTN+-_"),
    ("a longer UMI", "colon", 199, b"@A00:7:ACGTACGTA 1:N:0\n", "record 199", "differs from record 0's"),
    ("a joiner where record 0 has a base", "colon", 1, b"@A00:7:ACG+ACGT 1:N:0\n", "record 1", "differs from record 0's"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,at,line,record,reason", REFUSALS, ids=[r[0] for r in REFUSALS])
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_a_file_the_rule_refuses_ends_the_run_before_any_output(exe, tmp_path, paired, name, mode, at, line, record, reason):
    data = as_text(molecules(60, paired, n=200), mode, seed=2)
    recs = fast.parse(data[0], False)
    assert recs[at][0].startswith(recs[at][1])
    later = min(at + 50, len(recs) - 1)                          # the same fault once more further on: the lowest is named
    for k in (at, later):
        recs[k] = (line + recs[k][0][len(recs[k][1]):], line, recs[k][2])
    data[0] = b"".join(r[0] for r in recs)
    r, outs = cli(exe, tmp_path, data, env={**umi(mode), "FQD_FAST_CLUSTERS": "1"})
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_UMI") == 1 and f"FQD_FAST_UMI={mode}: {record} " in r.stderr and reason in r.stderr, r.stderr
    assert nothing_written(outs)


@pytest.mark.gpu
def test_a_pipe_is_refused(exe, tmp_path):
    fifo = tmp_path / "in.fq"
    os.mkfifo(fifo)
    out = tmp_path / "o.fq"
    r = run(exe, "-i", fifo, "-o", out, "--fast", env=umi("colon"))    # refused on the file's type: the pipe is never opened
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_UMI") == 1 and "not a regular file" in r.stderr
    assert not out.exists()


@pytest.mark.gpu
def test_a_bad_base_is_refused_and_the_message_says_what_the_position_counts(exe, tmp_path):
    good = as_text(molecules(11, False, n=200), "colon")[0]
    at = good.index(b"\n") + 1                                 # the first base of the first record
    r, outs = cli(exe, tmp_path, [good[:at] + b"R" + good[at + 1:]], env=umi("colon"))
    assert r.returncode == 1
    assert r.stderr.count("FQD_FAST_UMI") == 1 and "unknown character" in r.stderr
    assert "position 8" in r.stderr and "counts the 8 UMI bases in front of the sequence" in r.stderr
    assert nothing_written(outs)


@pytest.mark.gpu
def test_a_compare_seq_run_does_not_look_at_the_switch(exe, tmp_path):
    data = as_text(molecules(5, False, n=40), "colon")[0]
    src = tmp_path / "in.fq"; src.write_bytes(data)
    outs = []
    for tag, env in (("a", {"FQD_FAST_UMI": "comma"}), ("b", umi("colon")), ("c", {})):
        out = tmp_path / f"o{tag}.fq"
        r = run(exe, "-i", src, "-o", out, "--compare-seq", "tight", "-v", env=env)
        assert r.returncode == 0, r.stderr
        assert "FQD_FAST_UMI" not in r.stderr
        outs.append((r.stdout, out.read_bytes()))
    assert outs[0] == outs[1] == outs[2]
