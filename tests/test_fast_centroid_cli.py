"""FQD_FAST_CENTROID=abundant of the `--fast` mode through the CLI.  CPU part: what the switch's value and the command line decide,
before any GPU call.  GPU part, on families of reads — the clean copies of a fragment and a few copies with a substituted base
or a wrong UMI base, AN ERROR COPY OFTEN FIRST — with Illumina names, 300 .. 1 500 records, single-end and paired, FASTQ and
FASTA, plain, BGZF and ordinary gzip: the outputs, `.clusters`, `;size=N`, `.duplevels` and every `-v` line are those of the
statement below, which writes every merged cluster by the member tests/centroid_reference.py names, fed the merged owners of
the sequential statements the other CLI tests use (tests/near_reference.py, tests/umi_merge_reference.py,
tests/near_umi_reference.py, tests/optical_reference.py) and their exact owners; alone and with the other switches.  `first`
and unset give the bytes of the run without the switch; clusters, counts and level table never depend on it."""
import random

import numpy as np
import pytest

import centroid_reference as ref
import consensus_reference as cref
import fast_keep_reference as fast
import near_reference as near
import near_umi_reference as near_umi
import optical_reference as optical_ref
import size_order_reference as order_ref
import size_reference as sizes
import sizein_reference as sizein
import umi_merge_reference as umi_merge
import umi_reference as umi
import test_fast_consensus_cli as cons                        # consensus_line
import test_fast_hamming_cli as ham                           # cli and the file helpers
import test_fast_umi_hamming_cli as uh                        # fastq, records_of, statement

exe = ham.exe
NO_GPU, ALL = ham.NO_GPU, ham.ALL
read_out, levels_of, clusters_of, nothing_written, verbose_line = ham.read_out, ham.levels_of, ham.clusters_of, ham.nothing_written, ham.verbose_line
ABUNDANT = {"FQD_FAST_CENTROID": "abundant"}
PIXELS = 100
ALONE = ("FQD_FAST_CENTROID=abundant chooses among the different sequences of a merged cluster and nothing else: set one of FQD_FAST_UMI_MISMATCH, "
         "FQD_FAST_HAMMING or FQD_FAST_UMI_HAMMING as well, which merge them (without one every cluster holds one sequence)")


# ---- inputs --------------------------------------------------------------------------------------------------------------------

def other_base(rng, s, at):
    return s[:at] + rng.choice([c for c in "ACGT" if c != s[at]]) + s[at + 1:]


def family_rows(seed, paired, fragments=110, umi_errors=False, seq_errors=True):
    """rows (mates, UMI, x, y) for uh.fastq: a family is a fragment's clean copies (1 .. 9) and up to three error copies — one
    base of one mate substituted, or one base of the UMI — two of which may be the same copy twice.  Half of the families with
    an error copy have it FIRST.  Copies lie near the copy before them on the flow cell or anywhere; the families' members
    are dealt round robin, so that a family's order is its order in the file."""
    rng = random.Random(seed)
    families = []
    for _ in range(fragments):
        clean = tuple("".join(rng.choice("ACGT") for _ in range(rng.choice([36, 50, 51, 75]))) for _ in range(2 if paired else 1))
        u = "".join(rng.choice("ACGT") for _ in range(8))
        members = [(clean, u)] * rng.choice([1, 1, 2, 3, 3, 5, 9])
        errors = []
        for _ in range(rng.choice([0, 1, 1, 2, 3])):
            if errors and rng.random() < 0.4:
                errors.append(rng.choice(errors))               # the same error once more: a sub-cluster of its own of two
                continue
            seqs, v = clean, u
            if seq_errors and (not umi_errors or rng.random() < 0.5):
                m = rng.randrange(len(clean))
                seqs = tuple(other_base(rng, s, rng.randrange(len(s))) if k == m else s for k, s in enumerate(clean))
            else:
                v = other_base(rng, u, rng.randrange(8))
            errors.append((seqs, v))
        if len(set(errors)) >= 2 and rng.random() < 0.4:
            # a lone error copy in front of two sub-clusters of two: the tie goes to the one that starts earlier
            a, b = sorted(set(errors))[:2]
            two = [(clean, u), b] if rng.random() < 0.5 else [b, (clean, u)]
            members, errors = [a] + two + two, []
        if errors and rng.random() < 0.5:
            members = errors[:1] + members
            errors = errors[1:]
        for e in errors:
            members.insert(rng.randrange(1, len(members) + 1), e)
        x, y = rng.randrange(1000, 30000), rng.randrange(1000, 30000)
        placed = []
        for seqs, v in members:
            placed.append((seqs, v, x, y))
            if rng.random() < 0.6:
                x, y = x + rng.randrange(-PIXELS // 2, PIXELS // 2 + 1), y + rng.randrange(-PIXELS // 2, PIXELS // 2 + 1)
            else:
                x, y = rng.randrange(1000, 30000), rng.randrange(1000, 30000)
        families.append(placed)
    keyed = sorted((k, rng.random(), f) for f, fam in enumerate(families) for k in range(len(fam)))
    return [families[f][k] for k, _, f in keyed]


def as_fasta(data):
    return [b"".join(b">" + r[0][1:] + b"\n" + r[1] + b"\n" for r in cref.parse_fastq(x)) for x in data]


def with_weights(data, seed):
    """`;size=N` at the end of every first word (the same in both files): mostly 1, now and then up to 9."""
    rng = random.Random(seed)
    n = len(cref.parse_fastq(data[0]))
    w = [rng.choice([1, 1, 1, 1, 2, 4, 9]) for _ in range(n)]
    out = []
    for x in data:
        recs = cref.parse_fastq(x)
        out.append(cref.format_fastq([(r[0][:r[0].index(b" ")] + b";size=%d" % w[i] + r[0][r[0].index(b" "):],) + r[1:] for i, r in enumerate(recs)]))
    return out, w


# ---- the statement ---------------------------------------------------------------------------------------------------------------

def owners_hamming(data, fasta, d):
    """(merged owners, exact owners, the `-v` line of the merge)."""
    files = [fast.parse(x, fasta) for x in data]
    records = [tuple(f[i][2] for f in files) for i in range(len(files[0]))]
    owner, nodes, merged = near.merged_owners(records, d)
    return [int(o) for o in owner], [int(o) for o in near.exact_owners(records)], ham.second_line(nodes - merged, len(data) == 2, d)


def owners_umi(data, mismatch=0, d=0):
    """FQD_FAST_UMI=colon with FQD_FAST_UMI_MISMATCH and / or FQD_FAST_UMI_HAMMING."""
    records = uh.records_of(data, "colon")
    joiners = near_umi.joiners_of(records[0][0])
    exact = [int(o) for o in near_umi.exact_owners(records, joiners)]
    if d:
        owner, before, molecules, _ = uh.statement(data, "colon", d, mismatch)
        return owner, exact, uh.second_line(before - molecules, len(data) == 2, d)
    owner = umi_merge.merge([umi.bases(u) for u, _ in records], [m for _, m in records], mismatch, 4096)[0]
    return [int(o) for o in owner], exact, ""


def optically_split(data, owner):
    places = []
    for rec in fast.parse(data[0], False):
        reason, tile, x, y, surface = optical_ref.parse(rec[1])
        assert reason == optical_ref.OK
        places.append((surface, tile, x, y))
    split, info = optical_ref.split(owner, places, PIXELS)
    return [int(o) for o in split], info


def centroid_line(moved, paired):
    return (f"{moved} clusters were written by a copy of their most abundant {'sequence pair' if paired else 'sequence'}, not by their first "
            f"{'read pair' if paired else 'read'} (FQD_FAST_CENTROID=abundant).\n")


def arrays_of(owner):
    """(perm, head) as fqd_group_owners leaves them."""
    groups = fast.clusters_of(owner)
    perm = np.array([i for g in groups for i in g], np.uint32)
    head = np.zeros(len(perm), np.uint8)
    head[np.cumsum([0] + [len(g) for g in groups[:-1]])] = 1
    return groups, perm, head


def run_statement(data, fasta, owner, exact, abundant=True, best=False, weights=None, sizeout=False, by_size=False, lo=1, hi=None, consensus=False):
    """What a run writes: dict(outputs, clusters (the `.clusters` files), levels, total, dups, moved, gone, gone_records,
    bases, reads).  Every cluster is written by ref.written's member (its first without `abundant`)."""
    files = [fast.parse(x, fasta) for x in data]
    n = len(files[0])
    groups, perm, head = arrays_of(owner)
    scores = [min(fast.SAT, sum(fast.score(f[i][0]) for f in files)) for i in range(n)]
    w = weights or [1] * n
    centroids = ref.written(perm, head, exact, w) if abundant else [g[0] for g in groups]
    if best:
        chosen = ref.written(perm, head, exact if abundant else [0] * n, w, scores)
    else:
        chosen = centroids
    listing, moved = [], 0
    for g, c, b in zip(groups, centroids, chosen):
        order = list(g)
        for pick in (c, b):                                    # the two exchanges with the head's place, one after the other
            at = order.index(pick)
            order[0], order[at] = order[at], order[0]
        moved += c != g[0]
        listing.append(order)
    total_of = [sum(w[i] for i in g) for g in groups]
    bases = reads = 0
    records = [[r[0] for r in f] for f in files]
    if consensus:
        voted, bases, reads = cref.consensus_records([cref.parse_fastq(x) for x in data], listing)
        records = [[cref.format_fastq([r]) for r in f] for f in voted]
    outside = lambda t: t < lo or bool(hi and t > hi)
    written = [(order[0], t, g[0]) for order, t, g in zip(listing, total_of, groups) if not outside(t)]
    gone = [t for t in total_of if outside(t)]
    written.sort(key=(lambda t: (-t[1], t[2])) if by_size else (lambda t: t[0]))
    relabel = sizein.relabelled if weights else sizes.labelled
    outputs = [b"".join(relabel(recs[i], size) if sizeout else recs[i] for i, size, _ in written) for recs in records]
    cluster_files = [b"".join((b"" if k == 0 else b"--") + f[i][1] for order in listing for k, i in enumerate(order)) for f in files]
    return dict(outputs=outputs, clusters=cluster_files, levels=sizes.duplevels_text(total_of), total=n, dups=n - len(groups), moved=moved, gone=len(gone),
                gone_records=sum(gone), bases=bases, reads=reads, written=[i for i, _, _ in written])


def check_outputs(r, outs, want, stdout, with_files=True):
    assert r.returncode == 0, r.stderr
    assert r.stdout == stdout
    assert [read_out(o) for o in outs] == want["outputs"]
    if with_files:
        assert [clusters_of(o).read_bytes() for o in outs] == want["clusters"]
        assert levels_of(outs[0]).read_bytes() == want["levels"]


# ---------------------------------------------------------------- CPU: decided before any GPU call

@pytest.mark.parametrize("value", ["", "best", "Abundant", "1"])
def test_a_bad_value_is_refused(exe, tmp_path, value):
    r, outs = ham.cli(exe, tmp_path, uh.fastq(family_rows(1, False, fragments=4)), env={**NO_GPU, "FQD_FAST_CENTROID": value, "FQD_FAST_HAMMING": "1"})
    assert r.returncode == 1
    assert f"FQD_FAST_CENTROID must be 'first' or 'abundant', not '{value}'" in r.stderr
    assert nothing_written(outs)


def test_alone_and_in_the_wrong_run_it_is_refused(exe, tmp_path):
    data = uh.fastq(family_rows(2, True, fragments=4))
    for more in ({}, {"FQD_FAST_KEEP": "best"}, {"FQD_FAST_OPTICAL": "100"}, {"FQD_FAST_UMI": "colon"}):
        r, outs = ham.cli(exe, tmp_path, data, env={**NO_GPU, **ABUNDANT, **more})
        assert r.returncode == 1 and ALONE in r.stderr, more
        assert nothing_written(outs)
    env = {**NO_GPU, **ABUNDANT, "FQD_FAST_HAMMING": "2"}
    r, outs = ham.cli(exe, tmp_path, data, env=env, extra=["--unordered"])
    assert r.returncode == 1 and "FQD_FAST_HAMMING=2 and FQD_FAST_CENTROID=abundant with --unordered: these modes run on ordered inputs only" in r.stderr
    assert nothing_written(outs)
    r, outs = ham.cli(exe, tmp_path, data, env={**env, "FQD_DEVICES": "0,1"})
    assert r.returncode == 1 and "FQD_FAST_HAMMING=2 and FQD_FAST_CENTROID=abundant runs on one GPU: FQD_DEVICES may name one device only" in r.stderr
    assert nothing_written(outs)
    r, outs = ham.cli(exe, tmp_path, data, env={**env, "FQD_ORDERED_RESIDENT": "0"})
    assert r.returncode == 1 and "FQD_FAST_HAMMING=2 and FQD_FAST_CENTROID=abundant" in r.stderr and "FQD_ORDERED_RESIDENT" in r.stderr     # no streaming run for it
    assert nothing_written(outs)
    # of two bad settings the one in front in check()'s order is said
    r, outs = ham.cli(exe, tmp_path, data, env={**NO_GPU, **ABUNDANT, "FQD_FAST_UMI_MISMATCH": "1"})
    assert r.returncode == 1 and "FQD_FAST_UMI_MISMATCH=1 merges the UMIs that FQD_FAST_UMI finds" in r.stderr and ALONE not in r.stderr
    r, outs = ham.cli(exe, tmp_path, data, env={**NO_GPU, **ABUNDANT}, extra=["--unordered"])
    assert r.returncode == 1 and ALONE in r.stderr and "--unordered" not in r.stderr


@pytest.mark.parametrize("value", [None, "first"])
def test_first_and_unset_are_off(exe, tmp_path, value):
    # off: `--unordered` is not refused by the switch's name (without a GPU the run then ends for that reason)
    env = {**NO_GPU, **({} if value is None else {"FQD_FAST_CENTROID": value})}
    r, _ = ham.cli(exe, tmp_path, uh.fastq(family_rows(3, True, fragments=4)), env=env, extra=["--unordered"])
    assert "FQD_FAST_CENTROID" not in r.stderr


def test_the_inputs_of_these_tests():
    """From the statement: a fifth of the merged clusters change their written record, a tie goes each way, an optical group
    holds a label that another group holds too, and a weight turns a majority."""
    for paired in (False, True):
        data = uh.fastq(family_rows(4 + paired, paired))
        owner, exact, _ = owners_hamming(data, False, 2)
        groups, perm, head = arrays_of(owner)
        assert 300 <= len(owner) <= 1500
        stored, _, info = ref.abundances(perm, head, exact)
        centroids = ref.written(perm, head, exact, stored=stored)
        mixed = [(g, c) for g, c in zip(groups, centroids) if len({exact[i] for i in g}) > 1]
        assert info["mixed"] == len(mixed) > 40
        assert 5 * sum(c != g[0] for g, c in mixed) >= len(mixed)
        kept = taken = 0
        for g, c in mixed:
            top = max(stored[i] for i in g)
            tied = len({exact[i] for i in g if stored[i] == top}) > 1
            kept += tied and c == g[0]
            taken += tied and c != g[0]
        assert kept > 0 and taken > 0, (kept, taken)
        split, _ = optically_split(data, owner)
        label_groups = {}
        for i, o in enumerate(split):
            label_groups.setdefault(exact[i], set()).add(o)
        assert sum(len(v) > 1 for v in label_groups.values()) > 10
        sized, w = with_weights(data, 9)
        _, perm, head = arrays_of(owner)
        assert sum(a != b for a, b in zip(ref.written(perm, head, exact, w), centroids)) > 3
    for mismatch, d in ((1, 0), (0, 2), (1, 1)):
        data = uh.fastq(family_rows(6, False, umi_errors=True, seq_errors=d > 0))
        owner, exact, _ = owners_umi(data, mismatch, d)
        groups, perm, head = arrays_of(owner)
        centroids = ref.written(perm, head, exact)
        mixed = [(g, c) for g, c in zip(groups, centroids) if len({exact[i] for i in g}) > 1]
        assert len(mixed) > 30 and 5 * sum(c != g[0] for g, c in mixed) >= len(mixed)


# ---------------------------------------------------------------- GPU

CASES = [(False, False, "plain", False), (True, False, "bgzf", True), (False, True, "gzip", False), (True, True, "plain", False)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{'pe' if c[0] else 'se'}-{'fasta' if c[1] else 'fastq'}-{c[2]}-to-{'gz' if c[3] else 'plain'}" for c in CASES])
def test_the_majority_sequence_is_written(exe, tmp_path, case):
    paired, fasta, kind, gz_out = case
    data = uh.fastq(family_rows(600 + CASES.index(case), paired))
    if fasta:
        data = as_fasta(data)
    owner, exact, merge_line = owners_hamming(data, fasta, 2)
    want = run_statement(data, fasta, owner, exact, sizeout=True)
    env = {"FQD_FAST_HAMMING": "2", **ALL}
    r, outs = ham.cli(exe, tmp_path, data, kind, gz_out, env={**env, **ABUNDANT, "FQD_HOST_TIMING": "1"}, fasta=fasta)
    check_outputs(r, outs, want, verbose_line(want["total"], want["dups"], paired) + merge_line + centroid_line(want["moved"], paired))
    clusters = want["total"] - want["dups"]
    assert f"fast: most abundant sequence, {want['moved']} of {clusters} clusters changed, " in r.stderr and "fast: most abundant sequence on the GPU" in r.stderr
    assert want["moved"] > 10
    # every written record carries its cluster's majority sequence
    files = [fast.parse(x, fasta) for x in data]
    _, perm, head = arrays_of(owner)
    stored, _, _ = ref.abundances(perm, head, exact)
    for i in want["written"]:
        assert stored[i] == max(stored[j] for j in range(len(owner)) if owner[j] == owner[i])
    # `first` and unset: the run without the switch, byte for byte; clusters, counts and level table are the same in all three
    plain = run_statement(data, fasta, owner, exact, abundant=False, sizeout=True)
    assert plain["outputs"] != want["outputs"] and (plain["levels"], plain["total"], plain["dups"]) == (want["levels"], want["total"], want["dups"])
    runs = [ham.cli(exe, tmp_path, data, kind, gz_out, env={**env, **more}, tag=tag, fasta=fasta) for more, tag in (({}, "u"), ({"FQD_FAST_CENTROID": "first"}, "f"))]
    for rr, oo in runs:
        check_outputs(rr, oo, plain, verbose_line(plain["total"], plain["dups"], paired) + merge_line)
        assert "most abundant" not in rr.stderr
    assert [o.read_bytes() for o in runs[0][1]] == [o.read_bytes() for o in runs[1][1]]
    assert levels_of(outs[0]).read_bytes() == levels_of(runs[0][1][0]).read_bytes()
    assert len(files[0]) == want["total"]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("mismatch,d", [(1, 0), (0, 2), (1, 1)], ids=["umi_mismatch", "umi_hamming", "both"])
def test_the_majority_umi_is_in_the_written_name(exe, tmp_path, paired, mismatch, d):
    data = uh.fastq(family_rows(620 + 3 * paired + d, paired, umi_errors=True, seq_errors=d > 0))
    owner, exact, merge_line = owners_umi(data, mismatch, d)
    want = run_statement(data, False, owner, exact, sizeout=True)
    env = {"FQD_FAST_UMI": "colon", **({"FQD_FAST_UMI_MISMATCH": str(mismatch)} if mismatch else {}), **({"FQD_FAST_UMI_HAMMING": str(d)} if d else {}), **ALL}
    r, outs = ham.cli(exe, tmp_path, data, "bgzf" if paired else "plain", env={**env, **ABUNDANT})
    check_outputs(r, outs, want, verbose_line(want["total"], want["dups"], paired) + merge_line + centroid_line(want["moved"], paired))
    assert want["moved"] > 10
    # where UMIs merge, written names carry another UMI than the cluster's first record; where sequences merge (under one UMI),
    # written reads another sequence
    records = uh.records_of(data, "colon")
    if mismatch:
        assert sum(records[i][0] != records[owner[i]][0] for i in want["written"]) > 3
    if d:
        assert sum(records[i][1] != records[owner[i]][1] for i in want["written"]) > 3
    r0, outs0 = ham.cli(exe, tmp_path, data, "bgzf" if paired else "plain", env=env, tag="u")
    plain = run_statement(data, False, owner, exact, abundant=False, sizeout=True)
    check_outputs(r0, outs0, plain, verbose_line(plain["total"], plain["dups"], paired) + merge_line)


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_with_the_optical_split(exe, tmp_path, paired):
    data = uh.fastq(family_rows(640 + paired, paired))
    merged, exact, merge_line = owners_hamming(data, False, 2)
    owner, info = optically_split(data, merged)
    want = run_statement(data, False, owner, exact, sizeout=True)
    r, outs = ham.cli(exe, tmp_path, data, env={"FQD_FAST_HAMMING": "2", "FQD_FAST_OPTICAL": str(PIXELS), **ALL, **ABUNDANT})
    more = info["clusters_out"] - info["clusters_in"]
    assert more > 20 and want["moved"] > 5
    check_outputs(r, outs, want, verbose_line(want["total"], want["dups"], paired) + merge_line +
                  f"{more} {'read pairs' if paired else 'reads'} that repeat an earlier sequence were written: not optical duplicates (FQD_FAST_OPTICAL={PIXELS}).\n" +
                  centroid_line(want["moved"], paired))


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_best_copy_of_the_majority_sequence_and_the_consensus(exe, tmp_path, paired):
    data = uh.fastq(family_rows(650 + paired, paired))
    owner, exact, merge_line = owners_hamming(data, False, 2)
    env = {"FQD_FAST_HAMMING": "2", **ALL, **ABUNDANT}
    want = run_statement(data, False, owner, exact, best=True, sizeout=True)
    r, outs = ham.cli(exe, tmp_path, data, env={**env, "FQD_FAST_KEEP": "best"})
    check_outputs(r, outs, want, verbose_line(want["total"], want["dups"], paired) + merge_line + centroid_line(want["moved"], paired))
    assert want["outputs"] != run_statement(data, False, owner, exact, sizeout=True)["outputs"]                    # not the first copy of the majority,
    assert want["outputs"] != run_statement(data, False, owner, exact, abundant=False, best=True, sizeout=True)["outputs"]   # nor the whole cluster's best
    for consensus_env, best in (({}, False), ({"FQD_FAST_KEEP": "best"}, True)):
        want = run_statement(data, False, owner, exact, best=best, sizeout=True, consensus=True)
        r, outs = ham.cli(exe, tmp_path, data, gz_out=best, env={**env, **consensus_env, "FQD_FAST_CONSENSUS": "1"}, tag="c" + str(int(best)))
        check_outputs(r, outs, want, verbose_line(want["total"], want["dups"], paired) + merge_line + centroid_line(want["moved"], paired) +
                      cons.consensus_line(want["bases"], want["reads"], paired))
        assert want["bases"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_annotated_weights_turn_the_majority(exe, tmp_path, paired):
    data, w = with_weights(uh.fastq(family_rows(660 + paired, paired)), 660)
    owner, exact, merge_line = owners_hamming(data, False, 2)
    want = run_statement(data, False, owner, exact, weights=w, sizeout=True)
    assert want["written"] != run_statement(data, False, owner, exact, sizeout=True)["written"]
    r, outs = ham.cli(exe, tmp_path, data, env={"FQD_FAST_HAMMING": "2", "FQD_FAST_SIZEIN": "1", **ALL, **ABUNDANT})
    check_outputs(r, outs, want, verbose_line(want["total"], want["dups"], paired) + merge_line + centroid_line(want["moved"], paired))


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_abundance_order_and_the_filter(exe, tmp_path, paired):
    data = uh.fastq(family_rows(670 + paired, paired))
    owner, exact, merge_line = owners_hamming(data, False, 2)
    want = run_statement(data, False, owner, exact, sizeout=True, by_size=True, lo=2, hi=9)
    assert want["gone"] > 10 and want["moved"] > 10
    env = {"FQD_FAST_HAMMING": "2", "FQD_FAST_SIZEOUT": "1", "FQD_FAST_SORT": "size", "FQD_FAST_MINSIZE": "2", "FQD_FAST_MAXSIZE": "9", **ABUNDANT}
    r, outs = ham.cli(exe, tmp_path, data, gz_out=True, env=env)
    check_outputs(r, outs, want, verbose_line(want["total"], want["dups"], paired) + merge_line + order_ref.not_written_line(want["gone"], want["gone_records"], paired, 2, 9) +
                  centroid_line(want["moved"], paired), with_files=False)
    want = run_statement(data, False, owner, exact, lo=3)
    r, outs = ham.cli(exe, tmp_path, data, env={"FQD_FAST_HAMMING": "2", "FQD_FAST_MINSIZE": "3", **ABUNDANT}, tag="f")
    check_outputs(r, outs, want, verbose_line(want["total"], want["dups"], paired) + merge_line + order_ref.not_written_line(want["gone"], want["gone_records"], paired, 3, None) +
                  centroid_line(want["moved"], paired), with_files=False)
