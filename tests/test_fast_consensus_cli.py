"""FQD_FAST_CONSENSUS=1 of the `--fast` mode through the CLI.  CPU part: the three refusals, before any GPU call and any output.
GPU part, on inputs of tens to a few hundred reads with unique names: every output is the output of the run without the switch
— as the Python statements the other CLI tests use give it — with the sequence and quality lines of every written record
replaced by the consensus of its cluster (tests/consensus_reference.py), the clusters being those of the exact key, of
tests/near_reference.py (FQD_FAST_HAMMING), of tests/optical_reference.py or of the UMI key; with FQD_FAST_KEEP=best, the labels,
the abundance order and the filter, a `.gz` output; `.clusters` and `.duplevels` as without the switch; the `-v` line; unset and
0; empty inputs."""
import random
import re

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib
import consensus_reference as cref
import near_reference as near
import optical_reference as optical_ref
import size_order_reference as order_ref
import size_reference as sizes
import test_fast_hamming_cli as ham                           # its file helpers

NO_GPU = ham.NO_GPU
ON = {"FQD_FAST_CONSENSUS": "1"}
ALL = ham.ALL
cli, read_out, levels_of, clusters_of, nothing_written, verbose_line = ham.cli, ham.read_out, ham.levels_of, ham.clusters_of, ham.nothing_written, ham.verbose_line
PIXELS = 100


@pytest.fixture(scope="module")
def exe():
    if not _lib.CLI_PATH.exists():
        fqd.build_native("all")
    return str(_lib.CLI_PATH)


def consensus_line(bases, reads, paired):
    return f"{bases} bases in {reads} {'read pairs' if paired else 'reads'} were replaced by their cluster's consensus (FQD_FAST_CONSENSUS=1).\n"


# ---- inputs and the statement ------------------------------------------------------------------------------------------------------

def reads_input(seed, paired, fragments=40, d=1, exact_only=False):
    """Fragments x copies, shuffled.  A copy is the fragment with 0 .. d bases substituted a mate (none with exact_only) and
    qualities of its own, a few of them low.  Names are Illumina's with the record's number and an 8-base UMI — one UMI a
    fragment, now and then another — as the 8th and 9th field: unique, with a place on the flow cell, with a UMI."""
    rng = random.Random(seed)
    records = []
    for _ in range(fragments):
        first = tuple("".join(rng.choice("ACGT") for _ in range(rng.choice([36, 50, 51, 75]))) for _ in range(2 if paired else 1))
        umis = ["".join(rng.choice("ACGT") for _ in range(8)) for _ in range(2)]
        x, y = rng.randrange(1000, 30000), rng.randrange(1000, 30000)
        for _ in range(rng.choice([1, 1, 2, 3, 4, 6, 11])):
            seqs = first if exact_only else tuple(ham.substituted(rng, s, rng.choice([0, 0, 0, 1, d])) for s in first)
            records.append((seqs, x, y, umis[rng.random() < 0.2]))
            if rng.random() < 0.6:
                x, y = x + rng.randrange(-PIXELS // 2, PIXELS // 2 + 1), y + rng.randrange(-PIXELS // 2, PIXELS // 2 + 1)
            else:
                x, y = rng.randrange(1000, 30000), rng.randrange(1000, 30000)
    rng.shuffle(records)
    files = []
    for m in range(2 if paired else 1):
        out = []
        for k, (seqs, x, y, umi) in enumerate(records):
            quality = "".join(rng.choice("!#+5:?DFFFIIIIII") for _ in seqs[m])
            out.append(f"@M01:7:FC1:1:1101:{x}:{y}:r{k}:{umi} {m + 1}:N:0:ACGT\n{seqs[m]}\n+\n{quality}\n")
        files.append("".join(out).encode())
    return files


def sequences(data):
    files = [cref.parse_fastq(x) for x in data]
    return [tuple(f[i][1] for f in files) for i in range(len(files[0]))]


def exact_owners(data):
    return [int(o) for o in near.exact_owners(sequences(data))]


def near_owners(data, d):
    return [int(o) for o in near.merged_owners(sequences(data), d)[0]]


def umi_owners(data):
    first = {}
    ids = [r[0] for r in cref.parse_fastq(data[0])]
    return [first.setdefault((ids[i].split(b" ")[0].rsplit(b":", 1)[1], s), i) for i, s in enumerate(sequences(data))]


def record_number(id_line):
    return int(re.search(rb":r(\d+):", id_line).group(1))


def with_consensus(outputs, data, owner):
    """The outputs of a run without the switch (file contents), every written record's lines replaced by its cluster's
    consensus: the cluster is the records of its owner, the written member the record that stands in the output.  Returns
    (the outputs, bases changed, records (pairs) changed) over the records that are written."""
    files = [cref.parse_fastq(x) for x in data]
    members = {}
    for i, o in enumerate(owner):
        members.setdefault(o, []).append(i)
    outs = [cref.parse_fastq(o) for o in outputs]
    bases, reads = 0, 0
    for j in range(len(outs[0])):
        w = record_number(outs[0][j][0])
        c = [w] + [i for i in members[owner[w]] if i != w]
        if len(c) < 2:
            continue
        touched = False
        for s, f in enumerate(files):
            assert record_number(outs[s][j][0]) == w and outs[s][j][1] == f[w][1]
            seq, qual, n = cref.vote([(f[i][1], f[i][3]) for i in c])
            outs[s][j] = (outs[s][j][0], seq, outs[s][j][2], qual)
            bases += n
            touched |= n > 0
        reads += touched
    return [cref.format_fastq(o) for o in outs], bases, reads


# ---------------------------------------------------------------- CPU: decided before any GPU call

def test_fasta_is_refused(exe, tmp_path):
    data = [b">a\nACGT\n>b\nACGT\n"]
    r, outs = cli(exe, tmp_path, data, env={**NO_GPU, **ON}, fasta=True)
    assert r.returncode == 1
    assert "FQD_FAST_CONSENSUS=1 with --format fasta: the vote weighs every base by its quality, and FASTA records have no quality lines" in r.stderr
    assert nothing_written(outs)


def test_both_strands_are_refused(exe, tmp_path):
    r, outs = cli(exe, tmp_path, reads_input(1, True, fragments=3), env={**NO_GPU, **ON, "FQD_FAST_STRAND": "both"})
    assert r.returncode == 1
    assert "FQD_FAST_CONSENSUS=1 with FQD_FAST_STRAND=both: the members of a cluster may be keyed in opposite orientations" in r.stderr
    assert nothing_written(outs)


def test_size_annotations_are_refused(exe, tmp_path):
    r, outs = cli(exe, tmp_path, reads_input(2, False, fragments=3), env={**NO_GPU, **ON, "FQD_FAST_SIZEIN": "1", "FQD_FAST_SIZEOUT": "1"})
    assert r.returncode == 1
    assert "FQD_FAST_CONSENSUS=1 with FQD_FAST_SIZEIN=1: a record that stands for several reads has lost the quality lines of the reads it stands for" in r.stderr
    assert nothing_written(outs)


def test_the_refusals_of_every_linked_switch_name_it(exe, tmp_path):
    data = reads_input(3, True, fragments=3)
    r, outs = cli(exe, tmp_path, data, env={**NO_GPU, **ON}, extra=["--unordered"])
    assert r.returncode == 1 and "FQD_FAST_CONSENSUS=1 with --unordered: these modes run on ordered inputs only" in r.stderr and nothing_written(outs)
    r, outs = cli(exe, tmp_path, data, env={**NO_GPU, **ON, "FQD_DEVICES": "0,1"})
    assert r.returncode == 1 and "FQD_FAST_CONSENSUS=1 runs on one GPU: FQD_DEVICES may name one device only" in r.stderr and nothing_written(outs)
    r, outs = cli(exe, tmp_path, data, env={**NO_GPU, **ON, "FQD_ORDERED_RESIDENT": "0"})
    assert r.returncode == 1 and "FQD_FAST_CONSENSUS=1" in r.stderr and "FQD_ORDERED_RESIDENT" in r.stderr and nothing_written(outs)      # no streaming run for it


def test_the_inputs_of_these_tests():
    for paired in (False, True):
        data = reads_input(4, paired)
        exact, merged = exact_owners(data), near_owners(data, 1)
        n = len(exact)
        assert 60 <= n <= 300 and len(set(merged)) < len(set(exact)) < n
        default = sizes.dedup_sized(data, keys=merged)[4]
        _, bases, reads = with_consensus(default, data, merged)
        assert bases > 5 and 3 < reads < len(set(merged))
        # by the exact key every member has the written one's sequence: no base changes
        assert with_consensus(sizes.dedup_sized(data, keys=exact)[4], data, exact)[1:] == (0, 0)


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_an_error_copy_that_comes_first_is_corrected(exe, tmp_path, paired):
    good = ["ACGTTGCAAGGCTTAACCGGTATCGATCGGATCCAT", "TTGACCAGTAGGCATCAGGATACCAGATTTACG"]
    bad = ["ACGTTGCAAGGCTTAACCGGAATCGATCGGATCCAT", "TTGACCAGTAGGCATCAGGATACCAGATTTACC"]           # one base off in each
    other = ["G" * 36, "C" * 33]
    rows = [bad, other, good, good]
    data = []
    for m in range(2 if paired else 1):
        data.append("".join(f"@x:r{k}:AAAA {m + 1}\n{row[m]}\n+\n{('#' if row is bad else 'I') * len(row[m])}\n" for k, row in enumerate(rows)).encode())
    r, outs = cli(exe, tmp_path, data, env={**ON, "FQD_FAST_HAMMING": "1", "FQD_HOST_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    for m, o in enumerate(outs):
        got = cref.parse_fastq(read_out(o))
        # record 0's name, the good copies' bases; Phred 40 + 40 - 2 where the error stood, 40 + 40 + 2 elsewhere
        at = next(k for k in range(len(good[m])) if good[m][k] != bad[m][k])
        quality = "".join(chr(33 + 78) if k == at else chr(33 + 82) for k in range(len(good[m])))
        assert got == [(f"@x:r0:AAAA {m + 1}".encode(), good[m].encode(), b"+", quality.encode()),
                       (f"@x:r1:AAAA {m + 1}".encode(), other[m].encode(), b"+", b"I" * len(other[m]))]
    mates = 2 if paired else 1
    assert r.stdout == verbose_line(4, 2, paired) + ham.second_line(1, paired, 1) + consensus_line(mates, 1, paired)
    assert f"fast: consensus, 1 clusters of 3 records voted, largest 3, {mates} bases in 1 {'read pairs' if paired else 'reads'} replaced\n" in r.stderr
    # without the switch the erroneous read is what survives
    r, outs = cli(exe, tmp_path, data, env={"FQD_FAST_HAMMING": "1"}, tag="w")
    assert r.returncode == 0 and cref.parse_fastq(read_out(outs[0]))[0][1] == bad[0].encode()


@pytest.mark.gpu
@pytest.mark.parametrize("paired,kind,gz_out", [(False, "plain", False), (True, "bgzf", True), (False, "gzip", True), (True, "plain", False)],
                         ids=["se-plain", "pe-bgzf-to-gz", "se-gzip-to-gz", "pe-plain"])
def test_merged_clusters_are_written_as_their_consensus(exe, tmp_path, paired, kind, gz_out):
    d = 2 if paired else 1
    data = reads_input(600 + paired, paired, d=d)
    owner = near_owners(data, d)
    plain_labelled, exp_levels, total, dups, plain, exp_clusters = sizes.dedup_sized(data, keys=owner)
    exp_out, bases, reads = with_consensus(plain_labelled, data, owner)
    assert bases > 5 and exp_out != plain_labelled
    env = {**ON, **ALL, "FQD_FAST_HAMMING": str(d)}
    r, outs = cli(exe, tmp_path, data, kind, gz_out, env=env)
    assert r.returncode == 0, r.stderr
    assert [read_out(o) for o in outs] == exp_out                # `.gz` outputs: inflated and compared
    nodes = len(set(exact_owners(data)))
    assert r.stdout == verbose_line(total, dups, paired) + ham.second_line(nodes - (total - dups), paired, d) + consensus_line(bases, reads, paired)
    # the cluster files and the level table: those of the run without the switch
    r0, outs0 = cli(exe, tmp_path, data, kind, gz_out, env={**ALL, "FQD_FAST_HAMMING": str(d)}, tag="w")
    assert r0.returncode == 0 and [read_out(o) for o in outs0] == plain_labelled
    assert [clusters_of(o).read_bytes() for o in outs] == [clusters_of(o).read_bytes() for o in outs0] == exp_clusters
    assert levels_of(outs[0]).read_bytes() == levels_of(outs0[0]).read_bytes() == exp_levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_exact_clusters_keep_their_bases_and_add_their_qualities(exe, tmp_path, paired):
    data = reads_input(610 + paired, paired, exact_only=True)
    owner = exact_owners(data)
    r0, outs0 = cli(exe, tmp_path, data, tag="d")
    r, outs = cli(exe, tmp_path, data, env=ON)
    assert r0.returncode == 0 and r.returncode == 0, r0.stderr + r.stderr
    default = [read_out(o) for o in outs0]
    assert default == sizes.dedup_sized(data, keys=owner)[4]
    exp_out, bases, reads = with_consensus(default, data, owner)
    got = [read_out(o) for o in outs]
    assert got == exp_out and (bases, reads) == (0, 0)
    assert r.stdout == r0.stdout + consensus_line(0, 0, paired)
    changed = 0
    for a, b in zip(got, default):
        for x, y in zip(cref.parse_fastq(a), cref.parse_fastq(b)):
            assert x[:3] == y[:3]                                # ID, sequence and '+' lines are the default run's
            changed += x[3] != y[3]
    assert changed > 10                                          # the quality lines are the sums


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_best_copy_carries_the_consensus(exe, tmp_path, paired):
    data = reads_input(620 + paired, paired)
    owner = near_owners(data, 1)
    plain_labelled, exp_levels, total, dups, plain, exp_clusters = sizes.dedup_sized(data, best=True, keys=owner)
    assert plain_labelled != sizes.dedup_sized(data, keys=owner)[0]
    exp_out, bases, reads = with_consensus(plain_labelled, data, owner)
    r, outs = cli(exe, tmp_path, data, env={**ON, **ALL, "FQD_FAST_HAMMING": "1", "FQD_FAST_KEEP": "best"})
    assert r.returncode == 0, r.stderr
    assert [read_out(o) for o in outs] == exp_out
    assert [clusters_of(o).read_bytes() for o in outs] == exp_clusters and levels_of(outs[0]).read_bytes() == exp_levels
    assert r.stdout.endswith(consensus_line(bases, reads, paired))


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_labels_abundance_order_and_filter(exe, tmp_path, paired):
    data = reads_input(630 + paired, paired)
    owner = near_owners(data, 1)
    ordered, gone, gone_records, written = order_ref.dedup_ordered(data, keys=owner, by_size=True, lo=2, sizeout=True)
    assert gone > 5 and written == sorted(written, reverse=True) and written[0] > 2
    exp_out, bases, reads = with_consensus(ordered, data, owner)     # (a cluster of one is not voted on: the filter takes none that is)
    r, outs = cli(exe, tmp_path, data, gz_out=True, env={**ON, "FQD_FAST_HAMMING": "1", "FQD_FAST_SIZEOUT": "1", "FQD_FAST_SORT": "size", "FQD_FAST_MINSIZE": "2"})
    assert r.returncode == 0, r.stderr
    assert [read_out(o) for o in outs] == exp_out
    assert r.stdout.endswith(order_ref.not_written_line(gone, gone_records, paired, 2, None) + consensus_line(bases, reads, paired))


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_optical_groups_are_voted_on_their_own(exe, tmp_path, paired):
    data = reads_input(640 + paired, paired, exact_only=True)
    places = []
    for rec in cref.parse_fastq(data[0]):
        reason, tile, x, y, surface = optical_ref.parse(rec[0] + b"\n")
        assert reason == optical_ref.OK
        places.append((surface, tile, x, y))
    exact = exact_owners(data)
    split = [int(o) for o in optical_ref.split(exact, places, PIXELS)[0]]
    assert len(set(split)) > len(set(exact)) + 3
    plain = sizes.dedup_sized(data, keys=split)[4]
    exp_out, bases, reads = with_consensus(plain, data, split)
    assert exp_out != with_consensus(plain, data, exact)[0]          # the groups' sums, not the clusters'
    r, outs = cli(exe, tmp_path, data, env={**ON, "FQD_FAST_OPTICAL": str(PIXELS)})
    assert r.returncode == 0, r.stderr
    assert [read_out(o) for o in outs] == exp_out and r.stdout.endswith(consensus_line(bases, reads, paired))


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_umi_clusters_are_voted_on_their_own(exe, tmp_path, paired):
    data = reads_input(650 + paired, paired, exact_only=True)
    owner = umi_owners(data)
    assert len(set(owner)) > len(set(exact_owners(data))) + 3
    plain = sizes.dedup_sized(data, keys=owner)[4]
    exp_out, bases, reads = with_consensus(plain, data, owner)
    r, outs = cli(exe, tmp_path, data, env={**ON, "FQD_FAST_UMI": "colon"})
    assert r.returncode == 0, r.stderr
    assert [read_out(o) for o in outs] == exp_out and r.stdout.endswith(consensus_line(bases, reads, paired))


@pytest.mark.gpu
@pytest.mark.parametrize("value", [None, "0"])
def test_unset_and_zero_give_the_default_bytes(exe, tmp_path, value):
    data = reads_input(660, True)
    r0, outs0 = cli(exe, tmp_path, data, gz_out=True, env={"FQD_FAST_HAMMING": "1", "FQD_FAST_CLUSTERS": "1"}, tag="d")
    env = {"FQD_FAST_HAMMING": "1", "FQD_FAST_CLUSTERS": "1", "FQD_HOST_TIMING": "1", **({} if value is None else {"FQD_FAST_CONSENSUS": value})}
    r, outs = cli(exe, tmp_path, data, gz_out=True, env=env, tag="z")
    assert r0.returncode == 0 and r.returncode == 0 and r0.stdout == r.stdout, r0.stderr + r.stderr
    assert "consensus" not in r.stderr and "consensus" not in r.stdout
    for a, b in zip(outs0, outs):
        assert a.read_bytes() == b.read_bytes() and clusters_of(a).read_bytes() == clusters_of(b).read_bytes()
    if value == "0":                                             # alone, 0 is no switch at all: the streaming run's bytes
        r0, outs0 = cli(exe, tmp_path, data, tag="e")
        r, outs = cli(exe, tmp_path, data, env={"FQD_FAST_CONSENSUS": "0"}, tag="f")
        assert (r.returncode, r.stdout) == (r0.returncode, r0.stdout) and all(a.read_bytes() == b.read_bytes() for a, b in zip(outs0, outs))


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_empty_inputs(exe, tmp_path, paired):
    data = [b""] * (2 if paired else 1)
    r0, outs0 = cli(exe, tmp_path, data, tag="d")
    r, outs = cli(exe, tmp_path, data, env=ON)
    assert (r.returncode, r.stdout, r.stderr) == (r0.returncode, r0.stdout, r0.stderr)
    for a, b in zip(outs0, outs):
        assert a.exists() == b.exists() and (not a.exists() or a.read_bytes() == b.read_bytes())
