"""FQD_FAST_PREFIX=L of the `--fast` mode through the CLI.  CPU part: what the switch's value and the command line decide,
before any GPU call.  GPU part, on inputs of fragments x copies cut to different lengths, a few hundred records with Illumina
names — FASTQ and FASTA, plain, BGZF and ordinary gzip in and `.gz` out, single-end and paired: the outputs, `.clusters`,
`;size=N`, `.duplevels` and the `-v` lines are those of the Python statements the other CLI tests use (tests/size_reference.py,
tests/size_order_reference.py, tests/sizein_reference.py, tests/optical_reference.py, tests/centroid_reference.py) fed the merged
owners of the sequential statement (tests/prefix_reference.py), byte for byte, alone and combined with the other switches;
FQD_FAST_CENTROID=longest writes every cluster by the first copy of its longest sequence; unset and 0 give the default run's
bytes; a seed group beyond the limit and every refusal of the switches end the run before any output."""
import random

import numpy as np
import pytest

import centroid_reference as centroid_ref
import fast_keep_reference as fast
import optical_reference as optical_ref
import prefix_reference as ref
import size_order_reference as order_ref
import size_reference as sizes
import sizein_reference as sizein
from prefix_cases import group_records
import test_fast_hamming_cli as ham                           # cli and the file helpers

exe = ham.exe
NO_GPU, ALL, CASES = ham.NO_GPU, ham.ALL, ham.CASES
read_out, levels_of, clusters_of, nothing_written, verbose_line = ham.read_out, ham.levels_of, ham.clusters_of, ham.nothing_written, ham.verbose_line
L = 20
PIXELS = 100


def prefix(value=L):
    return {"FQD_FAST_PREFIX": str(value)}


def other_base(rng, s, at):
    return s[:at] + rng.choice([c for c in "ACGTN" if c != s[at]]) + s[at + 1:]


def truncated_input(seed, paired, fasta=False, fragments=90, sizein=False):
    """Fragments x copies, shuffled: a copy is the fragment with every mate cut to one of a few lengths (L - 1 and L among them),
    now and then with a base substituted inside what is left, so that it is nobody's prefix; a tenth of the fragments are two
    different reads with one beginning (two maximal sequences over the short copies).  Every copy has a place on the flow cell,
    near the copy before it or anywhere.  sizein: an 8th field with `;size=N` in the first word."""
    rng = random.Random(seed)
    cuts = [L - 1, L, L + 1, 36, 50, 75, 100, 100]
    records = []
    for f in range(fragments):
        whole = tuple("".join(rng.choice("ACGT") for _ in range(100)) for _ in range(2 if paired else 1))
        twin = tuple(s[:40] + "".join(rng.choice("ACGT") for _ in range(60)) for s in whole) if f % 10 == 0 else None
        x, y = rng.randrange(1000, 30000), rng.randrange(1000, 30000)
        for _ in range(rng.choice([1, 2, 3, 5, 8])):
            source = twin if twin and rng.random() < 0.4 else whole
            seqs = tuple(s[:rng.choice(cuts)] for s in source)
            if rng.random() < 0.15:
                seqs = tuple(other_base(rng, s, rng.randrange(len(s))) for s in seqs)
            records.append((seqs, x, y))
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


def records_of(data, fasta):
    files = [fast.parse(x, fasta) for x in data]
    return [tuple(f[i][2] for f in files) for i in range(len(files[0]))]


def statement(data, fasta, overlap=L):
    """(the merged owner of every record, the exact clusters, the merged clusters) by the sequential statement."""
    owner, counts = ref.merged_owners(records_of(data, fasta), overlap)
    return [int(o) for o in owner], counts["nodes"], counts["merged"]


def second_line(taken, paired, overlap=L):
    if paired:
        return (f"{taken} distinct sequence pairs were taken for copies of a longer sequence pair that begins with them, mate by mate, over at least {overlap} bases a mate "
                f"(FQD_FAST_PREFIX={overlap}).\n")
    return f"{taken} distinct sequences were taken for copies of a longer sequence that begins with them, over at least {overlap} bases (FQD_FAST_PREFIX={overlap}).\n"


def centroid_line(moved, paired, which):
    return (f"{moved} clusters were written by a copy of their {'most abundant' if which == 'abundant' else 'longest'} {'sequence pair' if paired else 'sequence'}, not by "
            f"their first {'read pair' if paired else 'read'} (FQD_FAST_CENTROID={which}).\n")


# ---------------------------------------------------------------- CPU: decided before any GPU call

@pytest.mark.parametrize("value", ["", "x", "-1", "01", "1 ", "+1", "65536"])
def test_a_bad_value_is_refused(exe, tmp_path, value):
    r, outs = ham.cli(exe, tmp_path, truncated_input(1, False, fragments=4), env={**NO_GPU, **prefix(value)})
    assert r.returncode == 1
    assert f"FQD_FAST_PREFIX must be a decimal integer in 1 .. 65535 (or 0 for off), not '{value}'" in r.stderr
    assert nothing_written(outs)


@pytest.mark.parametrize("env,words", [
    ({"FQD_FAST_HAMMING": "2"}, "FQD_FAST_PREFIX=20 with FQD_FAST_HAMMING=2: a truncated copy with substituted bases inside the overlap is a rule of its own"),
    ({"FQD_FAST_UMI": "colon"}, "FQD_FAST_PREFIX=20 with FQD_FAST_UMI=colon: which sequences under one UMI are copies of one molecule is a rule of its own"),
    ({"FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1"}, "FQD_FAST_PREFIX=20 with FQD_FAST_UMI=colon and FQD_FAST_UMI_MISMATCH=1: which sequences under one UMI"),
    ({"FQD_FAST_UMI": "underscore", "FQD_FAST_UMI_HAMMING": "1"}, "FQD_FAST_PREFIX=20 with FQD_FAST_UMI=underscore and FQD_FAST_UMI_HAMMING=1: which sequences under one UMI"),
    ({"FQD_FAST_STRAND": "both"}, "FQD_FAST_PREFIX=20 with FQD_FAST_STRAND=both: a truncated read's reverse complement is a suffix of its untrimmed copy's, not a prefix"),
    ({"FQD_FAST_CONSENSUS": "1"}, "FQD_FAST_PREFIX=20 with FQD_FAST_CONSENSUS=1: the members of a merged cluster differ in length"),
], ids=["hamming", "umi", "umi-mismatch", "umi-hamming", "strand", "consensus"])
def test_the_switches_it_does_not_go_with_are_refused(exe, tmp_path, env, words):
    r, outs = ham.cli(exe, tmp_path, truncated_input(2, True, fragments=4), env={**NO_GPU, **prefix(), **env})
    assert r.returncode == 1 and words in r.stderr, r.stderr
    assert nothing_written(outs)


def test_centroid_longest_without_it_is_refused(exe, tmp_path):
    for env in ({}, prefix(0), {"FQD_FAST_HAMMING": "1"}):
        r, outs = ham.cli(exe, tmp_path, truncated_input(2, False, fragments=4), env={**NO_GPU, "FQD_FAST_CENTROID": "longest", **env})
        assert r.returncode == 1 and "FQD_FAST_CENTROID=longest chooses the sequence that all others of a merged cluster are prefixes of, and nothing else: set FQD_FAST_PREFIX" in r.stderr
        assert nothing_written(outs)


def test_unordered_and_several_devices_are_refused_by_name(exe, tmp_path):
    r, outs = ham.cli(exe, tmp_path, truncated_input(2, True, fragments=4), env={**NO_GPU, **prefix(32)}, extra=["--unordered"])
    assert r.returncode == 1 and "FQD_FAST_PREFIX=32 with --unordered: these modes run on ordered inputs only" in r.stderr
    assert nothing_written(outs)
    r, outs = ham.cli(exe, tmp_path, truncated_input(2, False, fragments=4), env={**NO_GPU, **prefix(32), "FQD_DEVICES": "0,1"})
    assert r.returncode == 1 and "FQD_FAST_PREFIX=32 runs on one GPU: FQD_DEVICES may name one device only" in r.stderr
    assert nothing_written(outs)
    r, outs = ham.cli(exe, tmp_path, truncated_input(2, False, fragments=4), env={**NO_GPU, **prefix(32), "FQD_FAST_KEEP": "best", "FQD_ORDERED_RESIDENT": "0"})
    assert r.returncode == 1 and "FQD_FAST_KEEP=best and FQD_FAST_PREFIX=32" in r.stderr and "FQD_ORDERED_RESIDENT" in r.stderr      # no streaming run for it
    assert nothing_written(outs)


@pytest.mark.parametrize("value", [None, "0"])
def test_zero_and_unset_are_off(exe, tmp_path, value):
    # off: `--unordered` is not refused by the switch's name (without a GPU the run then ends for that reason)
    r, _ = ham.cli(exe, tmp_path, truncated_input(3, True, fragments=4), env={**NO_GPU, **({} if value is None else prefix(value))}, extra=["--unordered"])
    assert "FQD_FAST_PREFIX" not in r.stderr


def test_the_inputs_of_these_tests():
    for paired in (False, True):
        data = truncated_input(4, paired)
        records = records_of(data, False)
        owner, nodes, merged = statement(data, False)
        n = len(owner)
        assert 200 <= n <= 600 and merged < nodes - 30 and nodes < n - 10           # exact copies, merged ones
        assert merged > len({r for r in records if not ref.eligible(r, L)}) + 90    # ... and some that stay apart beside the short ones
        assert ref.check_the_theorems(records, L) > 0
        _, ids, parent = ref.parents(records, L)
        assert max(ref.depth_of(parent, v) for v in ids) >= 2                        # chains
        longest = [max(g, key=lambda i: (ref.span(records[i]), -i)) for g in fast.clusters_of(owner)]
        assert sum(c != g[0] for c, g in zip(longest, fast.clusters_of(owner))) > 9   # a short copy comes first in a tenth of the fragments at least


# ---------------------------------------------------------------- GPU

def check_run(r, outs, data, fasta, paired, overlap=L, expect=None):
    """The run's two `-v` lines, outputs with labels, cluster files and level table against size_reference fed the merged owners."""
    owner, nodes, merged = statement(data, fasta, overlap)
    exp_out, exp_levels, total, dups, _, exp_clusters = expect(owner) if expect else sizes.dedup_sized(data, fasta, keys=owner)
    assert dups == total - merged
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, dups, paired) + second_line(nodes - merged, paired, overlap)
    assert [read_out(o) for o in outs] == exp_out
    assert [clusters_of(o).read_bytes() for o in outs] == exp_clusters
    assert levels_of(outs[0]).read_bytes() == exp_levels
    return nodes, merged


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{'pe' if c[0] else 'se'}-{'fasta' if c[1] else 'fastq'}-{c[2]}-to-{'gz' if c[3] else 'plain'}" for c in CASES])
def test_truncated_copies_are_removed(exe, tmp_path, case):
    paired, fasta, kind, gz_out = case
    overlap = [L, 32, 36][CASES.index(case) % 3]
    data = truncated_input(500 + CASES.index(case), paired, fasta)
    r, outs = ham.cli(exe, tmp_path, data, kind, gz_out, env={**prefix(overlap), **ALL, "FQD_HOST_TIMING": "1"}, fasta=fasta)
    nodes, merged = check_run(r, outs, data, fasta, paired, overlap)
    assert f"fast: prefixes >= {overlap}, {nodes - merged} of {nodes} exact clusters merged into others, " in r.stderr
    assert " pairs compared, " in r.stderr and " related, largest seed group " in r.stderr and ", deepest chain " in r.stderr and " jumps\n" in r.stderr
    # without the labels: the records as they stand, the first of every merged cluster at its place
    r, outs = ham.cli(exe, tmp_path, data, kind, gz_out, env=prefix(overlap), tag="p", fasta=fasta)
    assert r.returncode == 0 and [read_out(o) for o in outs] == sizes.dedup_sized(data, fasta, keys=statement(data, fasta, overlap)[0])[4]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_best_copy_of_a_merged_cluster_is_written(exe, tmp_path, paired):
    data = truncated_input(510 + paired, paired)
    r, outs = ham.cli(exe, tmp_path, data, env={**prefix(), **ALL, "FQD_FAST_KEEP": "best"})
    check_run(r, outs, data, False, paired, expect=lambda owner: sizes.dedup_sized(data, False, best=True, keys=owner))
    assert [read_out(o) for o in outs] != sizes.dedup_sized(data, False, keys=statement(data, False)[0])[0]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_abundance_order_and_the_filter_read_the_merged_clusters(exe, tmp_path, paired):
    data = truncated_input(520 + paired, paired)
    owner, nodes, merged = statement(data, False)
    exp_out, gone, gone_records, written = order_ref.dedup_ordered(data, keys=owner, by_size=True, lo=2, sizeout=True)
    assert gone > 20 and written == sorted(written, reverse=True) and written[0] > 2
    r, outs = ham.cli(exe, tmp_path, data, gz_out=True, env={**prefix(), "FQD_FAST_SIZEOUT": "1", "FQD_FAST_SORT": "size", "FQD_FAST_MINSIZE": "2"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(len(owner), len(owner) - merged, paired) + second_line(nodes - merged, paired) + order_ref.not_written_line(gone, gone_records, paired, 2, None)
    assert [read_out(o) for o in outs] == exp_out


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_annotated_sizes_add_up_over_the_merged_clusters(exe, tmp_path, paired):
    data = truncated_input(530 + paired, paired, sizein=True)
    owner, nodes, merged = statement(data, False)
    exp_out, exp_levels, total, dups, _, _, _ = sizein.dedup_weighted(data, keys=owner)
    r, outs = ham.cli(exe, tmp_path, data, env={**prefix(), "FQD_FAST_SIZEOUT": "1", "FQD_FAST_LEVELS": "1", "FQD_FAST_SIZEIN": "1"})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(total, total - merged, paired) + second_line(nodes - merged, paired)
    assert [read_out(o) for o in outs] == exp_out and levels_of(outs[0]).read_bytes() == exp_levels


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_optical_distance_splits_the_merged_clusters(exe, tmp_path, paired):
    data = truncated_input(540 + paired, paired)
    owner, nodes, merged = statement(data, False)
    places = []
    for rec in fast.parse(data[0], False):
        reason, tile, x, y, surface = optical_ref.parse(rec[1])
        assert reason == optical_ref.OK
        places.append((surface, tile, x, y))
    split, info = optical_ref.split(owner, places, PIXELS)
    split = [int(o) for o in split]
    assert info["clusters_in"] == merged and info["clusters_out"] > merged + 20
    exact = [int(o) for o in ref.exact_owners(records_of(data, False))]
    assert split != [int(o) for o in optical_ref.split(exact, places, PIXELS)[0]] and split != owner
    exp_out, exp_levels, total, dups, _, exp_clusters = sizes.dedup_sized(data, False, keys=split)
    r, outs = ham.cli(exe, tmp_path, data, kind="bgzf", env={**prefix(), **ALL, "FQD_FAST_OPTICAL": str(PIXELS)})
    assert r.returncode == 0, r.stderr
    more = info["clusters_out"] - merged
    assert r.stdout == (verbose_line(total, total - info["clusters_out"], paired) + second_line(nodes - merged, paired) +
                        f"{more} {'read pairs' if paired else 'reads'} that repeat an earlier sequence were written: not optical duplicates (FQD_FAST_OPTICAL={PIXELS}).\n")
    assert [read_out(o) for o in outs] == exp_out
    assert [clusters_of(o).read_bytes() for o in outs] == exp_clusters
    assert levels_of(outs[0]).read_bytes() == exp_levels


def centroid_statement(data, owner, which, best=False):
    """What a run with FQD_FAST_CENTROID=which writes (FASTQ): dict(outputs with labels, clusters, levels, moved).  abundant: the
    first copy of the most abundant exact sequence (tests/centroid_reference.py); longest: the same pick with every record's span
    in the place of its abundance; best: then the best-scored copy of that sequence."""
    files = [fast.parse(x, False) for x in data]
    records = records_of(data, False)
    n = len(records)
    exact = [int(o) for o in ref.exact_owners(records)]
    groups = fast.clusters_of(owner)
    perm = np.array([i for g in groups for i in g], np.uint32)
    head = np.zeros(n, np.uint8)
    head[np.cumsum([0] + [len(g) for g in groups[:-1]])] = 1
    stored = [ref.span(r) for r in records] if which == "longest" else None
    centroids = centroid_ref.written(perm, head, exact, None, None, stored)
    chosen = centroids
    if best:
        scores = [min(fast.SAT, sum(fast.score(f[i][0]) for f in files)) for i in range(n)]
        chosen = centroid_ref.written(perm, head, exact, None, scores, stored)
    listing, moved = [], 0
    for g, c, b in zip(groups, centroids, chosen):
        order = list(g)
        for pick in (c, b):                                    # the two exchanges with the head's place, one after the other
            at = order.index(pick)
            order[0], order[at] = order[at], order[0]
        moved += c != g[0]
        listing.append(order)
    written = sorted((order[0], len(order)) for order in listing)
    outputs = [b"".join(sizes.labelled(f[i][0], size) for i, size in written) for f in files]
    cluster_files = [b"".join((b"" if k == 0 else b"--") + f[i][1] for order in listing for k, i in enumerate(order)) for f in files]
    return dict(outputs=outputs, clusters=cluster_files, levels=sizes.duplevels_text([len(g) for g in groups]), moved=moved, written=[i for i, _ in written])


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("which,best", [("abundant", False), ("longest", False), ("longest", True)], ids=["abundant", "longest", "longest-best"])
def test_the_centroid_of_a_merged_cluster_is_written(exe, tmp_path, which, best, paired):
    data = truncated_input(550 + paired, paired)
    records = records_of(data, False)
    owner, nodes, merged = statement(data, False)
    want = centroid_statement(data, owner, which, best)
    first = centroid_statement(data, owner, "abundant" if which == "longest" else "longest")
    assert want["moved"] > 0 and want["written"] != first["written"]              # (the two rules choose differently)
    if which == "longest":                                                          # every cluster is written by a copy of its root sequence
        _, ids, parent = ref.parents(records, L)
        exact = ref.exact_owners(records)
        assert all(ref.root_of(parent, int(exact[i])) == int(exact[i]) for i in want["written"])
    r, outs = ham.cli(exe, tmp_path, data, env={**prefix(), **ALL, "FQD_FAST_CENTROID": which, **({"FQD_FAST_KEEP": "best"} if best else {})})
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(len(owner), len(owner) - merged, paired) + second_line(nodes - merged, paired) + centroid_line(want["moved"], paired, which)
    assert [read_out(o) for o in outs] == want["outputs"]
    assert [clusters_of(o).read_bytes() for o in outs] == want["clusters"]
    assert levels_of(outs[0]).read_bytes() == want["levels"]


@pytest.mark.gpu
@pytest.mark.parametrize("paired,fasta,kind,gz_out", [(False, False, "plain", False), (True, False, "bgzf", True), (False, True, "gzip", False)])
def test_unset_and_zero_give_the_default_bytes(exe, tmp_path, paired, fasta, kind, gz_out):
    data = truncated_input(560 + paired, paired, fasta)
    r0, outs0 = ham.cli(exe, tmp_path, data, kind, gz_out, tag="d", fasta=fasta)
    rz, outsz = ham.cli(exe, tmp_path, data, kind, gz_out, env={**prefix(0), "FQD_HOST_TIMING": "1"}, tag="z", fasta=fasta)
    assert r0.returncode == 0 and rz.returncode == 0 and r0.stdout == rz.stdout, r0.stderr + rz.stderr
    assert "prefixes" not in rz.stderr
    for a, b in zip(outs0, outsz):
        assert a.read_bytes() == b.read_bytes()
    # the exact duplicates alone, as the default run counts them
    total = len(fast.parse(data[0], fasta))
    assert r0.stdout == verbose_line(total, total - statement(data, fasta)[1], paired)
    # set, the same input loses more
    r1, outs1 = ham.cli(exe, tmp_path, data, kind, gz_out, env=prefix(), tag="m", fasta=fasta)
    want = sizes.dedup_sized(data, fasta, keys=statement(data, fasta)[0])[4]
    assert r1.returncode == 0 and [read_out(o) for o in outs1] == want and want != [read_out(o) for o in outs0]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_empty_inputs(exe, tmp_path, paired):
    data = [b""] * (2 if paired else 1)
    r0, outs0 = ham.cli(exe, tmp_path, data, tag="d")
    r, outs = ham.cli(exe, tmp_path, data, env=prefix())
    assert (r.returncode, r.stdout, r.stderr) == (r0.returncode, r0.stdout, r0.stderr)
    for a, b in zip(outs0, outs):
        assert a.exists() == b.exists() and (not a.exists() or a.read_bytes() == b.read_bytes())


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_a_seed_group_beyond_the_limit_ends_the_run_before_any_output(exe, tmp_path, paired):
    rng = random.Random(580 + paired)
    overlap = 16
    records = group_records(rng, overlap, ref.MAX_GROUP + 1, paired=paired)
    records = records[:60] + records[10:30] + records[60:]       # copies do not count
    lowest, entries = ref.over_limit(records, overlap)
    assert entries == ref.MAX_GROUP + 1
    data = ["".join(f"@r{k} {m + 1}\n{r[m].decode()}\n+\n{'I' * len(r[m])}\n" for k, r in enumerate(records)).encode() for m in range(2 if paired else 1)]
    r, outs = ham.cli(exe, tmp_path, data, env={**prefix(overlap), **ALL})
    assert r.returncode == 1
    assert (f"FQD_FAST_PREFIX={overlap}: {entries} different sequences, the one of record {lowest} (counted from 0) of " in r.stderr and
            f"begin with the same {overlap} bases{' in each mate' if paired else ''}; a group of at most {ref.MAX_GROUP} is compared" in r.stderr and
            "set a larger FQD_FAST_PREFIX, or trim the reads first" in r.stderr)
    assert "ina0.fq" in r.stderr                                 # the file is named
    assert nothing_written(outs)
    # exactly the limit is merged
    records = group_records(rng, overlap, ref.MAX_GROUP, paired=paired)
    data = ["".join(f"@r{k} {m + 1}\n{r[m].decode()}\n+\n{'I' * len(r[m])}\n" for k, r in enumerate(records)).encode() for m in range(2 if paired else 1)]
    r, outs = ham.cli(exe, tmp_path, data, env=prefix(overlap), tag="l")
    assert r.returncode == 0, r.stderr
    assert r.stdout == verbose_line(ref.MAX_GROUP, 1, paired) + second_line(1, paired, overlap)
