"""fqd_consensus (csrc/fqd_consensus.hip) through the binding, byte for byte against the sequential statement
(tests/consensus_reference.py) over the WHOLE text buffer — so that ID lines, '+' lines, newlines, the members that are not
written, clusters of one, the gaps between records and the guard bytes behind the text are shown untouched — and the info's
counts exactly.  Every read length round the four-byte chunk, the sixteen lanes' round of 64 columns and a workgroup's round of
256; every start alignment of the rows; cluster sizes at both tier bounds and over several workgroups (FQD_CONSENSUS_SMALL_TIERS)
and one of 5000 members with the default bounds; members scattered through the input and a written member that is not the
lowest record; columns of one kind (ties, all N, all '!', sums across 93, a winner outweighed); random inputs; pairs counted
once through `changed`; misuse; and the same bytes from call to call."""
import random

import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, _lib
from fastq_dupaway_amd._lib import FqdError
import consensus_reference as ref
from consensus_cases import LENGTHS, SIZES, laid_out, noisy_cluster, scattered, special_clusters

pytestmark = pytest.mark.gpu
SMALL = _lib.CONSENSUS_SMALL_TIERS


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def voted(rows, perm, head):
    """The statement, once per input whatever its layout: (the rows with every written member's lines replaced, the info less
    reads_changed's dependence on `changed`, the written records with a changed base)."""
    after = list(rows)
    clusters = ref.clusters_of(perm, head)
    info = dict(clusters=0, members=0, bases_changed=0, largest=max(len(c) for c in clusters))
    touched = set()
    for c in clusters:
        if len(c) < 2:
            continue
        seq, qual, n = ref.vote([rows[r] for r in c])
        after[c[0]] = (seq, qual)
        info["clusters"] += 1
        info["members"] += len(c)
        info["bases_changed"] += n
        if n:
            touched.add(c[0])
    return after, info, touched


def call(e, text, arrays, perm, head, flags=0, changed=None):
    """One call over the text (bytes-like) laid out with `arrays`; returns (the whole buffer afterwards, the info)."""
    start, size, seq_off, seq_len = arrays
    d_text = dev(np.frombuffer(bytes(text), np.uint8).copy())
    info = e.consensus(dev(perm), dev(head), len(perm), d_text, dev(start), dev(size), dev(seq_off), dev(seq_len), flags, changed)
    e.sync()
    return d_text.cpu().numpy().tobytes(), info


def check(e, rows, perm, head, flags=0, align=0, gaps=None, want=None):
    """One call against the statement; the layout's gaps from random.Random(gaps).  Returns the bytes the call left."""
    after, info, touched = want or voted(rows, perm, head)
    text, *arrays = laid_out(rows, align, random.Random(gaps) if gaps is not None else None)
    expect, *_ = laid_out(after, align, random.Random(gaps) if gaps is not None else None)
    got, said = call(e, text, arrays, perm, head, flags)
    if got != bytes(expect):
        at = next(k for k in range(len(expect)) if got[k] != expect[k])
        rec = int(np.searchsorted(arrays[0], at, side="right")) - 1
        raise AssertionError((flags, align, "first differing byte", at, "in record", rec, got[at - 8:at + 8], bytes(expect[at - 8:at + 8])))
    assert (said.clusters, said.members, said.bases_changed, said.reads_changed, said.largest) == (
        info["clusters"], info["members"], info["bases_changed"], len(touched), info["largest"])
    return got


def test_the_statement_agrees_with_itself_over_a_laid_out_text():
    # ref.apply over text and arrays, and voted() over rows: two routes to one text (no GPU call; the other tests lean on it)
    rng = random.Random(1)
    rows, perm, head = scattered(rng, [noisy_cluster(rng, m, L) for m, L in [(1, 9), (2, 17), (5, 4), (3, 0), (1, 0), (4, 64)]], written="any")
    after, info, touched = voted(rows, perm, head)
    text, *arrays = laid_out(rows, 3, random.Random(5))
    expect, *_ = laid_out(after, 3, random.Random(5))
    said = ref.apply(text, *arrays, ref.clusters_of(perm, head))
    assert bytes(text) == bytes(expect)
    assert said == dict(info, reads_changed=len(touched))


# ---- read lengths and alignments -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def every_length():
    """Clusters of 2 and 3 (sixteen lanes), 9 (a workgroup) and 65 members (several workgroups, with the small tiers) at every
    length, voted once."""
    rng = random.Random(2)
    clusters = [noisy_cluster(rng, m, L) for L in LENGTHS for m in (2, 3, 9, 65)] + [noisy_cluster(rng, 1, L) for L in LENGTHS]
    rows, perm, head = scattered(rng, clusters)
    return rows, perm, head, voted(rows, perm, head)


@pytest.mark.parametrize("aligns", [range(0, 4), range(4, 8), range(8, 12), range(12, 16)], ids=["0-3", "4-7", "8-11", "12-15"])
def test_every_length_at_every_alignment(every_length, aligns):
    rows, perm, head, want = every_length
    assert want[1]["bases_changed"] > 100
    with Engine() as e:
        for align in aligns:
            check(e, rows, perm, head, SMALL, align, want=want)                       # back to back: record k's rows move with the ID lines in front
            check(e, rows, perm, head, SMALL if align % 2 else 0, align, gaps=align, want=want)


# ---- cluster sizes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("length", [5, 151])
def test_cluster_sizes_round_the_tier_bounds(length):
    rng = random.Random(3 + length)
    clusters = [noisy_cluster(rng, m, length) for m in SIZES for _ in range(2)]
    rows, perm, head = scattered(rng, clusters, written="any")          # the order behind a best-quality pick
    want = voted(rows, perm, head)
    assert want[1]["largest"] == 129 and want[1]["clusters"] == 2 * (len(SIZES) - 1)
    with Engine() as e:
        small = check(e, rows, perm, head, SMALL, 1, gaps=7, want=want)
        again = check(e, rows, perm, head, SMALL, 1, gaps=7, want=want)
        default = check(e, rows, perm, head, 0, 1, gaps=7, want=want)      # the same clusters through the other tiers
    assert small == again == default


def test_five_thousand_members_with_the_default_bounds():
    rng = random.Random(4)
    clusters = [noisy_cluster(rng, 5000, 67, error_rate=0.3), noisy_cluster(rng, 2, 67), noisy_cluster(rng, 1, 67)]
    rows, perm, head = scattered(rng, clusters, written="any")
    want = voted(rows, perm, head)
    assert want[1]["largest"] == 5000
    with Engine() as e:
        a = check(e, rows, perm, head, 0, 5, gaps=1, want=want)
        b = check(e, rows, perm, head, SMALL, 5, gaps=1, want=want)         # 313 workgroups' atomics
    assert a == b


def test_more_places_than_the_tile_scans_first_round():
    """The one block that scans the head counts takes 1024 tiles of 2048 places a round: 1024 tiles, one tile and three places
    more, of ten-byte records (`@`, two bases, `+`, two qualities).  Clusters of one but for a few of 3 to 5 members: at the
    start, across the round's edge, in the tile behind it and across the last tile's edge.  ref.apply over the same text is the statement."""
    n = 1024 * 2048 + 2048 + 3
    rng = np.random.default_rng(8)
    text = np.tile(np.frombuffer(b"@\nAC\n+\nII\n", np.uint8), n).reshape(n, 10)
    runs = [(100, 3), (1024 * 2048 - 2, 5), (1024 * 2048 + 1000, 4), (n - 5, 5)]       # (the last one across the last tile's edge)
    head = np.ones(n, np.uint8)
    for at, m in runs:
        head[at + 1:at + m] = 0
        text[at:at + m, 2:4] = rng.choice(np.frombuffer(b"ACGTN", np.uint8), (m, 2))
        text[at:at + m, 7:9] = rng.integers(33, 75, (m, 2))
    text = np.concatenate([text.reshape(-1), np.full(32, 0xEE, np.uint8)])
    start = np.arange(n, dtype=np.uint64) * np.uint64(10)
    arrays = (start, np.full(n, 10, np.uint32), start + np.uint64(2), np.full(n, 2, np.uint32))
    expect = bytearray(text.tobytes())
    info = ref.apply(expect, *arrays, [list(range(at, at + m)) for at, m in runs])
    assert info["clusters"] == 4 and info["bases_changed"] > 0
    with Engine() as e:
        got, said = call(e, text.tobytes(), arrays, np.arange(n, dtype=np.uint32), head)
    assert got == bytes(expect)
    assert (said.clusters, said.members, said.bases_changed, said.reads_changed, said.largest) == (
        4, 17, info["bases_changed"], info["reads_changed"], 5)


# ---- columns of one kind -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("copies", [1, 3, 22], ids=["as they are", "9 members at most", "66 members at most"])
def test_columns_of_one_kind(copies):
    # every member `copies` times: a tie stays a tie, sums grow; 2 or 3 members, 6 or 9, 44 or 66
    rng = random.Random(5)
    clusters = []
    for length in (1, 17, 70):
        for name, members in special_clusters(length):
            clusters.append([members[0]] + members[1:] * copies + [members[0]] * (copies - 1))
    rows, perm, head = scattered(rng, clusters)
    want = voted(rows, perm, head)
    after = want[0]
    written = {c[0]: c for c in ref.clusters_of(perm, head)}
    by_first_line = {rows[w]: after[w] for w in written}
    L = 17
    assert by_first_line[(b"C" * L, b"5" * L)][0] == b"C" * L and by_first_line[(b"T" * L, b"!" * L)][0] == b"C" * L      # ties: with, without the own letter
    assert by_first_line[(b"N" * L, b"~" * L)] == (b"N" * L, b"!" * L) and by_first_line[(b"G" * L, b"!" * L)] == (b"G" * L, b"!" * L)
    assert by_first_line[(b"A" * L, b"~" * L)] == (b"A" * L, b"~" * L) and by_first_line[(b"A" * L, b"I" * L)] == (b"A" * L, b"!" * L)
    assert by_first_line[(b"T" * L, b"#" * L)][0] == b"G" * L                          # the error copy that came first is corrected
    with Engine() as e:
        for flags in (0, SMALL):
            check(e, rows, perm, head, flags, 2, gaps=3, want=want)


# ---- random inputs, pairs --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [6, 7])
def test_random_pairs_are_counted_once(seed):
    rng = random.Random(seed)
    sizes = [rng.choice([1, 1, 1, 2, 2, 3, 4, 5, 9, 12, 30, 70]) for _ in range(120)]
    lengths = [(rng.choice([20, 31, 50, 75, 100, 150]), rng.choice([20, 31, 50, 75, 100, 150])) for _ in sizes]
    rate = [rng.choice([0.0, 0.0, 0.02, 0.1]) for _ in sizes]          # clusters in which nothing changes among them
    mate1 = [noisy_cluster(rng, m, L[0], error_rate=r, n_rate=r / 2) for m, L, r in zip(sizes, lengths, rate)]
    mate2 = [noisy_cluster(rng, m, L[1], error_rate=r, n_rate=r / 2) for m, L, r in zip(sizes, lengths, rate)]
    (rows1, rows2), perm, head = scattered(rng, mate1, written="any", mates=mate2)      # the same (perm, head) serves both files
    n = len(rows1)
    want1, want2 = voted(rows1, perm, head), voted(rows2, perm, head)
    either = want1[2] | want2[2]
    assert want1[2] - want2[2] and want2[2] - want1[2] and want1[2] & want2[2] and len(either) < want1[1]["clusters"]
    with Engine() as e:
        for flags in (0, SMALL):
            changed = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
            changed[n:] = 0xEE
            infos = []
            for rows, want in ((rows1, want1), (rows2, want2)):
                text, *arrays = laid_out(rows, 0, random.Random(seed))
                expect, *_ = laid_out(want[0], 0, random.Random(seed))
                got, said = call(e, text, arrays, perm, head, flags, changed)
                assert got == bytes(expect)
                assert (said.clusters, said.members, said.bases_changed, said.largest) == tuple(want[1][k] for k in ("clusters", "members", "bases_changed", "largest"))
                infos.append(said)
            assert infos[0].reads_changed == len(want1[2]) and infos[1].reads_changed == len(want2[2] - want1[2])
            assert infos[0].reads_changed + infos[1].reads_changed == len(either)
            flag = changed.cpu().numpy()
            assert set(np.nonzero(flag[:n])[0].tolist()) == either and np.all(flag[:n] <= 1) and np.all(flag[n:] == 0xEE)


# ---- degenerate inputs and misuse -------------------------------------------------------------------------------------------------

def test_nothing_and_only_clusters_of_one():
    with Engine() as e:
        info = e.consensus(None, None, 0, None, None, None, None, None)
        assert (info.clusters, info.members, info.bases_changed, info.reads_changed, info.largest) == (0, 0, 0, 0, 0)
        rng = random.Random(8)
        rows, perm, head = scattered(rng, [noisy_cluster(rng, 1, L) for L in (0, 1, 150, 7)])
        check(e, rows, perm, head, 0, 0)
        check(e, rows, perm, head, SMALL, 3, gaps=2)


def test_misuse_is_refused_and_stores_nothing():
    rng = random.Random(9)
    clusters = [noisy_cluster(rng, m, 40, error_rate=0.3) for m in (3, 1, 9, 70, 2)]
    rows, perm, head = scattered(rng, clusters)
    n = len(rows)
    text, start, size, seq_off, seq_len = laid_out(rows, 0, random.Random(1))
    before = bytes(text)
    three = next(c for c in ref.clusters_of(perm, head) if len(c) == 3)
    first_of_three, last_of_three = three[0], max(three)         # (the last one is not record 0)

    def shorter_member():                                        # one member of a cluster with a shorter sequence line: unequal lengths
        other = seq_len.copy()
        c = next(c for c in ref.clusters_of(perm, head) if len(c) == 70)
        other[c[33]] -= 1
        return dict(seq_len=other)

    def fasta_like():                                            # a record that ends with its sequence line: the quality line would be that line
        other = size.copy()
        other[first_of_three] = int(seq_off[first_of_three] - start[first_of_three]) + int(seq_len[first_of_three]) + 1
        return dict(size=other)

    def a_single_fasta_like():                                   # the same in a cluster of one
        other = size.copy()
        single = next(c[0] for c in ref.clusters_of(perm, head) if len(c) == 1)
        other[single] = int(seq_len[single])
        return dict(size=other)

    def sequence_in_front():
        other = seq_off.copy()
        other[last_of_three] = start[last_of_three] - 1
        return dict(seq_off=other)

    def no_first_head():
        other = head.copy()
        other[0] = 0
        return dict(head=other)

    def record_outside():
        other = perm.copy()
        other[5] = n
        return dict(perm=other)

    with Engine() as e:
        def attempt(n_records=n, flags=0, info=True, **other):
            given = dict(perm=perm, head=head, start=start, size=size, seq_off=seq_off, seq_len=seq_len)
            given.update(other)
            d_text = dev(np.frombuffer(before, np.uint8).copy())
            with pytest.raises(FqdError) as refused:
                e.consensus(dev(given["perm"]), dev(given["head"]), n_records, d_text, dev(given["start"]), dev(given["size"]), dev(given["seq_off"]),
                            dev(given["seq_len"]), flags, None, info)
            assert refused.value.code == _lib.ERR_ARG
            e.sync()
            assert d_text.cpu().numpy().tobytes() == before      # nothing stored
        for make in (shorter_member, fasta_like, a_single_fasta_like, sequence_in_front, no_first_head, record_outside):
            for flags in (0, SMALL):
                attempt(flags=flags, **make())
        attempt(n_records=2 ** 31)
        attempt(n_records=2 ** 31 + 5, flags=SMALL)
        attempt(flags=2)
        attempt(info=None)
        check(e, rows, perm, head, SMALL, 0, gaps=1)                 # the engine is as good as before
