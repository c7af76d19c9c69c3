"""FQD_FAST_UMI_HAMMING=D of the `--fast` mode through the CLI.  CPU part: what the switch's value and the command line decide,
before any GPU call.  GPU part, on inputs of fragments x UMIs x copies with 0 .. D + 1 substituted bases a mate, Illumina names
with the UMI as the 8th field (colon) or behind a '_' (underscore), single-end and paired, plain, BGZF and ordinary gzip: the
outputs, `.clusters`, `;size=N`, `.duplevels` and the `-v` lines are those of the Python statements the other CLI tests use
(tests/size_reference.py, tests/size_order_reference.py, tests/optical_reference.py, tests/consensus_reference.py) fed the
molecules of the sequential statement (tests/near_umi_reference.py; its links from tests/umi_merge_reference.py), alone and
combined with the other switches; unset and 0 give the FQD_FAST_UMI run's bytes; a seed group beyond the limit ends the run
before any output."""
import os
import random
import subprocess

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib
import consensus_reference as cref
import near_umi_reference as ref
import optical_reference as optical_ref
import size_order_reference as order_ref
import size_reference as sizes
import umi_merge_reference as umi_merge
import umi_reference as umi
from near_cases import group_records
import test_fast_consensus_cli as cons                        # with_consensus, consensus_line
import test_fast_hamming_cli as ham                           # its file helpers
import test_fast_umi_cli as inputs                            # PACK

SWITCHES = ham.SWITCHES + ("FQD_FAST_UMI_HAMMING", "FQD_FAST_CONSENSUS")
NO_GPU = ham.NO_GPU
ALL = ham.ALL
read_out, levels_of, clusters_of, nothing_written, verbose_line = ham.read_out, ham.levels_of, ham.clusters_of, ham.nothing_written, ham.verbose_line
SEP = {"colon": b":", "underscore": b"_"}
D = 2
PIXELS = 100


def switch(d=D, mode="colon", **more):
    return {"FQD_FAST_UMI_HAMMING": str(d), **({"FQD_FAST_UMI": mode} if mode else {}), **more}


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


def cli(exe, tmp_path, data, kind="plain", gz_out=False, env=None, tag="a", extra=()):
    ins = [tmp_path / f"in{tag}{k}.fq{'' if kind == 'plain' else '.gz'}" for k in range(len(data))]
    outs = [tmp_path / f"out{tag}{k}.fq{'.gz' if gz_out else ''}" for k in range(len(data))]
    for p, x in zip(ins, data):
        p.write_bytes(inputs.PACK[kind](x))
    args = ["-i", ins[0], "-o", outs[0]]
    if len(data) == 2:
        args += ["-u", ins[1], "-p", outs[1]]
    return run(exe, *args, "--fast", "-v", *extra, env=env), outs


def fastq(rows, mode="colon", rng=None):
    """rows: (mates as str, UMI, x, y).  Names are Illumina's with the UMI behind the y field — the 8th field with colon — and
    the record's number in the comment."""
    sep = SEP[mode].decode()
    rng = rng or random.Random(len(rows))
    files = []
    for m in range(len(rows[0][0])):
        out = []
        for k, (seqs, u, x, y) in enumerate(rows):
            quality = "".join(rng.choice("!#+5:?DFFFIIIIII") for _ in seqs[m])
            out.append(f"@M01:7:FC1:1:1101:{x}:{y}{sep}{u} {m + 1}:N:0:r{k}:ACGT\n{seqs[m]}\n+\n{quality}\n")
        files.append("".join(out).encode())
    return files


def copies_input(seed, paired, mode="colon", fragments=90, d=D, dual=False):
    """Fragments x UMIs x copies, shuffled.  A fragment has a UMI of its own, a second one that is far from it and one that is
    one base from it; a copy is the fragment, or the copy before it, with 0 .. d + 1 bases substituted in every mate, under the
    first UMI mostly.  Every copy has a place on the flow cell, near the copy before it or anywhere.  dual: UMIs of two halves
    joined by '+' or '-', whichever: one tag."""
    rng = random.Random(seed)
    rows = []
    for _ in range(fragments):
        first = tuple("".join(rng.choice("ACGT") for _ in range(rng.choice([36, 50, 51, 75]))) for _ in range(2 if paired else 1))
        own, far = ("".join(rng.choice("ACGT") for _ in range(8)) for _ in range(2))
        close = ham.substituted(rng, own, 1).replace("N", "A" if own[0] != "A" else "C")
        seqs, x, y = first, rng.randrange(1000, 30000), rng.randrange(1000, 30000)
        for _ in range(rng.choice([1, 2, 3, 5, 8, 12])):
            u = rng.choice([own] * 7 + [far] * 2 + [close])
            if dual:
                u = u[:4] + rng.choice("+-") + u[4:]
            rows.append((seqs, u, x, y))
            seqs = tuple(ham.substituted(rng, s, rng.choice([0, 0, 0, 1, 1, d, d + 1])) for s in rng.choice([first, seqs]))
            if rng.random() < 0.5:
                x, y = x + rng.randrange(-PIXELS // 2, PIXELS // 2 + 1), y + rng.randrange(-PIXELS // 2, PIXELS // 2 + 1)
            else:
                x, y = rng.randrange(1000, 30000), rng.randrange(1000, 30000)
    rng.shuffle(rows)
    return fastq(rows, mode, rng)


def records_of(data, mode):
    """(U, mates) of every record, as the statement takes them."""
    files = [cref.parse_fastq(x) for x in data]
    out = []
    for i, rec in enumerate(files[0]):
        _, u = umi.umi_of(rec[0] + b"\n", SEP[mode])
        assert isinstance(u, bytes), rec[0]
        out.append((u, tuple(f[i][1] for f in files)))
    return out


def statement(data, mode, d=D, mismatch=0):
    """(every record's molecule owner, the clusters in front of the stage, the molecules, the owners in front of the stage)."""
    records = records_of(data, mode)
    joiners = ref.joiners_of(records[0][0])
    link = None
    if mismatch:
        link = umi_merge.merge([umi.bases(u) for u, _ in records], [m for _, m in records], mismatch, 4096)[0]
    owner, nodes, molecules, links = ref.molecules(records, d, joiners, link)
    before = link if mismatch else ref.exact_owners(records, joiners)
    assert nodes - links == len({int(o) for o in before})
    return [int(o) for o in owner], nodes - links, molecules, [int(o) for o in before]


def second_line(taken, paired, d=D):
    if paired:
        return f"{taken} distinct sequence pairs under one UMI were taken for copies of another that differs in at most {d} bases a mate (FQD_FAST_UMI_HAMMING={d}).\n"
    return f"{taken} distinct sequences under one UMI were taken for copies of another that differs in at most {d} bases (FQD_FAST_UMI_HAMMING={d}).\n"


# ---------------------------------------------------------------- CPU: decided before any GPU call

@pytest.mark.parametrize("value", ["4", "-1", "x", "", "1.5", "01", "1 "])
def test_a_bad_value_is_refused(exe, tmp_path, value):
    r, outs = cli(exe, tmp_path, copies_input(1, False, fragments=4), env={**NO_GPU, **switch(value)})
    assert r.returncode == 1
    assert f"FQD_FAST_UMI_HAMMING must be 0, 1, 2 or 3, not '{value}'" in r.stderr
    assert nothing_written(outs)


def test_the_switch_alone_and_with_both_strands_is_refused(exe, tmp_path):
    data = copies_input(2, True, fragments=4)
    r, outs = cli(exe, tmp_path, data, env={**NO_GPU, **switch(1, None)})
    assert r.returncode == 1 and ("FQD_FAST_UMI_HAMMING=1 merges the sequences under one of the UMIs that FQD_FAST_UMI finds: set FQD_FAST_UMI=colon or "
                                  "FQD_FAST_UMI=underscore as well") in r.stderr
    assert nothing_written(outs)
    r, outs = cli(exe, tmp_path, data, env={**NO_GPU, **switch(3), "FQD_FAST_STRAND": "both"})
    assert r.returncode == 1 and "FQD_FAST_UMI_HAMMING=3 with FQD_FAST_STRAND=both: a substituted base can change which orientation" in r.stderr
    assert nothing_written(outs)
    # FQD_FAST_HAMMING's refusal with UMIs stays what it was, and comes first
    r, outs = cli(exe, tmp_path, data, env={**NO_GPU, **switch(2, "underscore"), "FQD_FAST_HAMMING": "2"})
    assert r.returncode == 1 and "FQD_FAST_HAMMING=2 with FQD_FAST_UMI=underscore: which sequences under one UMI are copies of one molecule is a rule of its own" in r.stderr
    assert nothing_written(outs)


def test_unordered_and_several_devices_are_refused_by_name(exe, tmp_path):
    r, outs = cli(exe, tmp_path, copies_input(2, True, fragments=4), env={**NO_GPU, **switch(3)}, extra=["--unordered"])
    assert r.returncode == 1 and "FQD_FAST_UMI=colon and FQD_FAST_UMI_HAMMING=3 with --unordered: these modes run on ordered inputs only" in r.stderr
    assert nothing_written(outs)
    r, outs = cli(exe, tmp_path, copies_input(2, False, fragments=4), env={**NO_GPU, **switch(1), "FQD_DEVICES": "0,1"})
    assert r.returncode == 1 and "FQD_FAST_UMI=colon and FQD_FAST_UMI_HAMMING=1 runs on one GPU: FQD_DEVICES may name one device only" in r.stderr
    assert nothing_written(outs)
    r, outs = cli(exe, tmp_path, copies_input(2, False, fragments=4), env={**NO_GPU, **switch(2), "FQD_ORDERED_RESIDENT": "0"})
    assert r.returncode == 1 and "FQD_FAST_UMI=colon and FQD_FAST_UMI_HAMMING=2" in r.stderr and "FQD_ORDERED_RESIDENT" in r.stderr      # no streaming run for it
    assert nothing_written(outs)


@pytest.mark.parametrize("value", [None, "0"])
def test_zero_and_unset_are_off(exe, tmp_path, value):
    # off: the switch needs no FQD_FAST_UMI and is named by no refusal (without a GPU the run then ends for that reason)
    env = {**NO_GPU, **({} if value is None else switch(value, None))}
    r, _ = cli(exe, tmp_path, copies_input(3, True, fragments=4), env=env, extra=["--unordered"])
    assert "FQD_FAST_UMI_HAMMING" not in r.stderr


def test_the_inputs_of_these_tests():
    for paired in (False, True):
        for d in (1, 2, 3):
            for mode, dual in (("colon", False), ("underscore", True)):
                data = copies_input(4, paired, mode, d=d, dual=dual)
                owner, before, molecules, exact = statement(data, mode, d)
                n = len(owner)
                assert 250 <= n <= 1500 and 90 < molecules < before - 30 and before < n - 20      # exact copies, merged ones, and some that stay apart
                records = records_of(data, mode)
                joiners = ref.joiners_of(records[0][0])
                assert (joiners != 0) == dual
                # no molecule holds two tags; some hold members that are not near their first record (single linkage)
                assert all(ref.tag(records[i][0], joiners) == ref.tag(records[owner[i]][0], joiners) for i in range(n))
                assert len({(ref.tag(u, joiners), m) for u, m in records}) > len({m for _, m in records}) + 20       # one sequence under several UMIs
                linked, clusters, both, _ = statement(data, mode, d, mismatch=1)
                assert both < molecules and both < clusters < before


# ---------------------------------------------------------------- GPU

CASES = [(False, "colon", "plain", False), (False, "underscore", "bgzf", True), (False, "colon", "gzip", False),
         (True, "underscore", "plain", True), (True, "colon", "bgzf", False), (True, "underscore", "gzip", False)]
CASE_IDS = [f"{'pe' if c[0] else 'se'}-{c[1]}-{c[2]}-to-{'gz' if c[3] else 'plain'}" for c in CASES]


def check_run(r, outs, data, mode, paired, d=D, mismatch=0, expect=None):
    """The run's two `-v` lines, outputs with labels, cluster files and level table against size_reference fed the molecules."""
    owner, before, molecules, _ = statement(data, mode, d, mismatch)
    exp_out, exp_levels, total, dups, _, exp_clusters = expect(owner) if expect else sizes.dedup_sized(data, False, keys=owner)
    assert dups == total - molecules
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired) + second_line(before - molecules, paired, d)
    assert [read_out(o) for o in outs] == exp_out
    assert [clusters_of(o).read_bytes() for o in outs] == exp_clusters
    assert levels_of(outs[0]).read_bytes() == exp_levels
    return before, molecules


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_copies_with_substituted_bases_under_one_umi_are_removed(exe, tmp_path, case):
    paired, mode, kind, gz_out = case
    d = 1 + CASES.index(case) % 3
    data = copies_input(500 + CASES.index(case), paired, mode, d=d, dual=mode == "underscore")
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env={**switch(d, mode), **ALL, "FQD_HOST_TIMING": "1"})
    before, molecules = check_run(r, outs, data, mode, paired, d)
    assert f"fast: UMI substitutions <= {d}, {before - molecules} of {before} clusters merged into others, " in r.stderr
    assert " pairs compared, " in r.stderr and " near, 0 links, largest seed group " in r.stderr and " sweeps\n" in r.stderr
    # without the labels: the records as they stand, the first of every molecule at its place
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env=switch(d, mode), tag="p")
    assert r.returncode == 0 and [read_out(o) for o in outs] == sizes.dedup_sized(data, False, keys=statement(data, mode, d)[0])[4]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_best_copy_of_a_molecule_is_written(exe, tmp_path, paired):
    data = copies_input(510 + paired, paired)
    r, outs = cli(exe, tmp_path, data, env={**switch(), **ALL, "FQD_FAST_KEEP": "best"})
    check_run(r, outs, data, "colon", paired, expect=lambda owner: sizes.dedup_sized(data, False, best=True, keys=owner))
    assert [read_out(o) for o in outs] != sizes.dedup_sized(data, False, keys=statement(data, "colon")[0])[0]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_abundance_order_and_the_filter_read_the_molecules(exe, tmp_path, paired):
    data = copies_input(520 + paired, paired, "underscore")
    owner, before, molecules, _ = statement(data, "underscore")
    exp_out, gone, gone_records, written = order_ref.dedup_ordered(data, keys=owner, by_size=True, lo=2, sizeout=True)
    assert gone > 20 and written == sorted(written, reverse=True) and written[0] > 2
    r, outs = cli(exe, tmp_path, data, gz_out=True, env={**switch(D, "underscore"), "FQD_FAST_SIZEOUT": "1", "FQD_FAST_SORT": "size", "FQD_FAST_MINSIZE": "2"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(len(owner), len(owner) - molecules, paired) + second_line(before - molecules, paired) + order_ref.not_written_line(gone, gone_records, paired, 2, None)
    assert [read_out(o) for o in outs] == exp_out


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_optical_distance_splits_the_molecules(exe, tmp_path, paired):
    data = copies_input(540 + paired, paired)                    # colon: the UMI is the 8th field, behind the place
    owner, before, molecules, exact = statement(data, "colon")
    places = []
    for rec in cref.parse_fastq(data[0]):
        reason, tile, x, y, surface = optical_ref.parse(rec[0] + b"\n")
        assert reason == optical_ref.OK
        places.append((surface, tile, x, y))
    split, info = optical_ref.split(owner, places, PIXELS)
    split = [int(o) for o in split]
    assert info["clusters_in"] == molecules and info["clusters_out"] > molecules + 20
    assert split != [int(o) for o in optical_ref.split(exact, places, PIXELS)[0]] and split != owner
    exp_out, exp_levels, total, dups, _, exp_clusters = sizes.dedup_sized(data, False, keys=split)
    r, outs = cli(exe, tmp_path, data, kind="bgzf", env={**switch(), **ALL, "FQD_FAST_OPTICAL": str(PIXELS)})
    assert r.returncode == 0, r.stderr
    more = info["clusters_out"] - molecules
    assert r.stdout == (verbose_line(total, total - info["clusters_out"], paired) + second_line(before - molecules, paired) +
                        f"{more} {'read pairs' if paired else 'reads'} that repeat an earlier sequence were written: not optical duplicates (FQD_FAST_OPTICAL={PIXELS}).\n")
    assert [read_out(o) for o in outs] == exp_out
    assert [clusters_of(o).read_bytes() for o in outs] == exp_clusters
    assert levels_of(outs[0]).read_bytes() == exp_levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired,mode,mismatch", [(False, "colon", 1), (True, "underscore", 1), (False, "underscore", 2)], ids=["se-colon-1", "pe-underscore-1", "se-underscore-2"])
def test_the_triple_with_the_mismatch_switch(exe, tmp_path, paired, mode, mismatch):
    data = copies_input(550 + paired + mismatch, paired, mode, dual=mode == "underscore")
    env = {**switch(D, mode), "FQD_FAST_UMI_MISMATCH": str(mismatch), **ALL, "FQD_HOST_TIMING": "1"}
    r, outs = cli(exe, tmp_path, data, env=env)
    before, molecules = check_run(r, outs, data, mode, paired, mismatch=mismatch)
    nodes = len(set(statement(data, mode)[3]))
    assert f"fast: UMI substitutions <= {D}, {before - molecules} of {before} clusters merged into others, " in r.stderr
    assert f" near, {nodes - before} links, largest seed group " in r.stderr and nodes > before
    # neither switch alone gives these molecules
    assert molecules < statement(data, mode)[2] and molecules < before
    # the regrowth of the edge list covers the links
    r, outs = cli(exe, tmp_path, data, env={**env, "FQD_NEAR_EDGE_ROOM": "3"}, tag="r")
    check_run(r, outs, data, mode, paired, mismatch=mismatch)


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_a_family_whose_first_copy_carries_the_error_is_written_with_the_majority_s_sequence(exe, tmp_path, paired):
    good = ["ACGTTGCAAGGCTTAACCGGTATCGATCGGATCCAT", "TTGACCAGTAGGCATCAGGATACCAGATTTACG"]
    bad = ["ACGTTGCAAGGCTTAACCGGAATCGATCGGATCCAT", "TTGACCAGTAGGCATCAGGATACCAGATTTACC"]           # one base off in each
    rows = [(bad, "AACCGGTT"), (good, "TTGGCCAA"), (good, "AACCGGTT"), (good, "AACCGGTT")]           # record 1: the good read under ANOTHER UMI
    data = []
    for m in range(2 if paired else 1):
        data.append("".join(f"@x:r{k}:{u} {m + 1}\n{row[m]}\n+\n{('#' if row is bad else 'I') * len(row[m])}\n" for k, (row, u) in enumerate(rows)).encode())
    r, outs = cli(exe, tmp_path, data, env={**switch(1), "FQD_FAST_CONSENSUS": "1", "FQD_HOST_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    for m, o in enumerate(outs):
        got = cref.parse_fastq(read_out(o))
        # record 0's name, the good copies' bases; Phred 40 + 40 - 2 where the error stood, 40 + 40 + 2 elsewhere
        at = next(k for k in range(len(good[m])) if good[m][k] != bad[m][k])
        quality = "".join(chr(33 + 78) if k == at else chr(33 + 82) for k in range(len(good[m])))
        assert got == [(f"@x:r0:AACCGGTT {m + 1}".encode(), good[m].encode(), b"+", quality.encode()),
                       (f"@x:r1:TTGGCCAA {m + 1}".encode(), good[m].encode(), b"+", b"I" * len(good[m]))]
    mates = 2 if paired else 1
    assert r.stdout == verbose_line(4, 2, paired) + second_line(1, paired, 1) + cons.consensus_line(mates, 1, paired)
    assert f"fast: consensus, 1 clusters of 3 records voted, largest 3, {mates} bases in 1 {'read pairs' if paired else 'reads'} replaced\n" in r.stderr
    # without the new switch the three are two clusters of one sequence each: the vote can change no base
    r, outs = cli(exe, tmp_path, data, env={"FQD_FAST_UMI": "colon", "FQD_FAST_CONSENSUS": "1"}, tag="w")
    assert r.returncode == 0 and r.stdout == verbose_line(4, 1, paired) + cons.consensus_line(0, 0, paired)
    assert cref.parse_fastq(read_out(outs[0]))[0][1] == bad[0].encode()


@pytest.mark.gpu
@pytest.mark.parametrize("paired,kind,gz_out,mismatch", [(False, "plain", False, 0), (True, "bgzf", True, 0), (False, "gzip", True, 1), (True, "plain", False, 1)],
                         ids=["se-plain", "pe-bgzf-to-gz", "se-gzip-to-gz-mismatch", "pe-plain-mismatch"])
def test_molecules_are_written_as_their_consensus(exe, tmp_path, paired, kind, gz_out, mismatch):
    d = 2 if paired else 1
    data = copies_input(600 + paired + 2 * mismatch, paired, d=d)
    owner, before, molecules, _ = statement(data, "colon", d, mismatch)
    plain_labelled, exp_levels, total, dups, plain, exp_clusters = sizes.dedup_sized(data, keys=owner)
    exp_out, bases, reads = cons.with_consensus(plain_labelled, data, owner)
    assert bases > 5 and exp_out != plain_labelled
    env = {**switch(d), **ALL, "FQD_FAST_CONSENSUS": "1", **({"FQD_FAST_UMI_MISMATCH": str(mismatch)} if mismatch else {})}
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env=env)
    assert r.returncode == 0, r.stderr
    assert [read_out(o) for o in outs] == exp_out                # `.gz` outputs: inflated and compared
    assert r.stdout == verbose_line(total, dups, paired) + second_line(before - molecules, paired, d) + cons.consensus_line(bases, reads, paired)
    assert [clusters_of(o).read_bytes() for o in outs] == exp_clusters and levels_of(outs[0]).read_bytes() == exp_levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired,mode,kind,gz_out", [(False, "colon", "plain", False), (True, "underscore", "bgzf", True), (False, "underscore", "gzip", False)])
def test_unset_and_zero_give_the_umi_run_s_bytes(exe, tmp_path, paired, mode, kind, gz_out):
    data = copies_input(560 + paired, paired, mode)
    umi_only = {"FQD_FAST_UMI": mode}
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, env=umi_only, tag="d")
    rz, outsz = cli(exe, tmp_path, data, kind, gz_out, env={**switch(0, mode), "FQD_HOST_TIMING": "1"}, tag="z")
    assert r0.returncode == 0 and rz.returncode == 0 and r0.stdout == rz.stdout, r0.stderr + rz.stderr
    assert "substitutions" not in rz.stderr
    for a, b in zip(outs0, outsz):
        assert a.read_bytes() == b.read_bytes()
    # the exact duplicates under their UMIs alone
    owner, before, molecules, exact = statement(data, mode)
    assert r0.stdout == verbose_line(len(owner), len(owner) - before, paired)
    assert [read_out(o) for o in outs0] == sizes.dedup_sized(data, False, keys=exact)[4]
    # with the mismatch switch as well: that run's bytes
    both = {**umi_only, "FQD_FAST_UMI_MISMATCH": "1", **ALL}
    r1, outs1 = cli(exe, tmp_path, data, kind, gz_out, env=both, tag="m")
    r2, outs2 = cli(exe, tmp_path, data, kind, gz_out, env={**both, "FQD_FAST_UMI_HAMMING": "0"}, tag="n")
    assert r1.returncode == 0 and r2.returncode == 0 and r1.stdout == r2.stdout
    for a, b in zip(outs1, outs2):
        assert a.read_bytes() == b.read_bytes() and clusters_of(a).read_bytes() == clusters_of(b).read_bytes()
    # set, the same input loses more
    r3, outs3 = cli(exe, tmp_path, data, kind, gz_out, env=switch(3, mode), tag="s")
    assert r3.returncode == 0 and [read_out(o) for o in outs3] == sizes.dedup_sized(data, False, keys=statement(data, mode, 3)[0])[4]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_empty_inputs(exe, tmp_path, paired):
    data = [b""] * (2 if paired else 1)
    r0, outs0 = cli(exe, tmp_path, data, tag="d")
    r, outs = cli(exe, tmp_path, data, env={**switch(), "FQD_FAST_UMI_MISMATCH": "1"})
    assert (r.returncode, r.stdout, r.stderr) == (r0.returncode, r0.stdout, r0.stderr)
    for a, b in zip(outs0, outs):
        assert a.exists() == b.exists() and (not a.exists() or a.read_bytes() == b.read_bytes())


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_a_seed_group_beyond_the_limit_ends_the_run_before_any_output(exe, tmp_path, paired):
    rng = random.Random(580 + paired)

    def text(records, umi_of_record):
        return ["".join(f"@r{k}:{umi_of_record(k)} {m + 1}\n{r[m].decode()}\n+\n{'I' * len(r[m])}\n" for k, r in enumerate(records)).encode() for m in range(2 if paired else 1)]

    records = group_records(rng, D, ref.MAX_GROUP + 1, paired=paired)
    records = records[:60] + records[10:30] + records[60:]       # copies do not count
    lowest, entries = ref.over_limit([(b"ACGTACGT", r) for r in records], D, 0)
    assert entries == ref.MAX_GROUP + 1
    r, outs = cli(exe, tmp_path, text(records, lambda k: "ACGTACGT"), env={**switch(), **ALL})
    assert r.returncode == 1
    assert (f"FQD_FAST_UMI_HAMMING={D}: {entries} different sequences under one UMI, the one of record {lowest} (counted from 0) of " in r.stderr and
            f"share one of the {D + 1} segments their first mate is cut into; a group of at most {ref.MAX_GROUP} is compared" in r.stderr)
    assert "ina0.fq" in r.stderr                                 # the file is named
    assert nothing_written(outs)
    # the same sequences under two UMIs are two groups within the limit
    r, outs = cli(exe, tmp_path, text(records, lambda k: "ACGTACGT" if k % 2 else "TTGTACGT"), env=switch(), tag="l")
    assert r.returncode == 0, r.stderr
