"""fqd_near_merge (csrc/fqd_near.hip) through the binding, exactly against the sequential statement (tests/near_reference.py:
exact clusters, all pairs compared, union-find): every merged owner, the counts of the info, nothing written behind the last
entry.  D = 1, 2, 3, single-end and paired.  Read lengths round the sixteen-byte chunk and the rounds of eight lanes, ragged
and uniform reads, every start alignment; differences exactly D and D + 1 at the segment bounds, all in one segment, one in
every segment but one; shapes; chains, stars and scattered copies; seed groups round the lane, wave and limit sizes and one
entry beyond the limit; weak seeds; the edge list's regrowth; random inputs; degenerate inputs and misuse; and the clusters of
fqd_sort_seqs + fqd_seq_heads(FQD_SEQ_HAMMING), which lie inside the merged ones."""
import random
from collections import Counter

import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, Reads, _lib
from fastq_dupaway_amd._lib import FqdError
import near_reference as ref
from near_cases import (GROUP_SIZES, chain_nodes, difference_pairs, every_short_read, group_records, lengths_for, mate2_length, random_records, scattered,
                        star_nodes, substituted, template)

pytestmark = pytest.mark.gpu
FILL = 0xEE
GUARD = 8                                                      # entries behind the last one of owner_out
NONE32 = 0xFFFFFFFF
DS = [1, 2, 3]


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def placed(records, uniform=False, align=0, rng=None, gap=b""):
    """The records' mates in device memory as Reads: ragged — back to back from byte `align` on, FILL (or `gap`) in between where
    rng says so — or uniform, every read at a stride of its length + 3.  Returns (segs, what must stay alive)."""
    n, segs, alive = len(records), [], []
    for s in range(len(records[0])):
        mates = [r[s] for r in records]
        lens = np.array([len(m) for m in mates], np.uint32)
        if uniform:
            assert len(set(lens.tolist())) == 1
            stride = int(lens[0]) + 3
            body = b"".join(m + bytes([FILL]) * 3 for m in mates)
            buf = dev(np.frombuffer(bytes([FILL]) * align + body, np.uint8).copy())
            segs.append(Reads(buf[align:], uniform_len=int(lens[0]), uniform_stride=stride))
            alive.append(buf)
            continue
        gaps = [gap + bytes([FILL]) * (rng.randrange(4) if rng else 0) for _ in mates]
        offs = np.zeros(n, np.uint64)
        at, parts = align, [bytes([FILL]) * align]
        for k, m in enumerate(mates):
            offs[k] = at
            parts += [m, gaps[k]]
            at += len(m) + len(gaps[k])
        buf, d_off, d_len = dev(np.frombuffer(b"".join(parts) + b"\0" * 16, np.uint8).copy()), dev(offs), dev(lens)
        segs.append(Reads(buf, d_off, d_len))
        alive += [buf, d_off, d_len]
    return segs, alive


def expected_pairs(records, D, weak):
    """The pairs of entries of two different nodes, over all seed groups."""
    total = 0
    for g in ref.seed_groups(records, D, weak).values():
        total += len(g) * (len(g) - 1) // 2 - sum(c * (c - 1) // 2 for c in Counter(g).values())
    return total


def merge(e, records, D, flags=0, **how):
    n = len(records)
    segs, alive = placed(records, **how)
    owner = dev(ref.exact_owners(records))
    out = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    info = e.near_merge(segs, owner, n, D, out, flags)
    e.sync()
    got = out.cpu().numpy().view(np.uint32)
    assert np.all(got[n:] == NONE32)                           # nothing behind the last entry
    return got[:n], info


def check(e, records, D, flags=0, counts=True, **how):
    """One call against the statement; returns the info."""
    got, info = merge(e, records, D, flags, **how)
    want, nodes, merged = ref.merged_owners(records, D)
    assert (info.nodes, info.entries, info.max_group, info.over_limit_first) == (nodes, nodes * (D + 1), ref.MAX_GROUP, ref.NO_RECORD)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (D, bad[:10], got[bad[:10]], want[bad[:10]], [records[i] for i in bad[:3]])
    assert info.merged == merged
    if counts:
        weak = bool(flags & _lib.NEAR_WEAK_SEEDS)
        groups = ref.seed_groups(records, D, weak)
        assert (info.groups, info.largest_group) == (len(groups), max(len(g) for g in groups.values()))
        assert info.largest_group <= ref.MAX_GROUP
        assert info.pairs == expected_pairs(records, D, weak)
        assert nodes - merged <= info.edges <= info.pairs      # a spanning forest at least; a pair once for every seed it shares
    return info


def flat(pairs):
    return [r for _, a, b, _ in pairs for r in (a, b)]


# ---- read lengths, alignments, where the differences fall ---------------------------------------------------------------------------

@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("D", DS)
def test_every_length_with_the_differences_at_the_segment_bounds(D, paired):
    rng = random.Random(100 + D)
    everything = []
    with Engine(segments=2 if paired else 1) as e:
        for length in lengths_for(D):
            pairs = difference_pairs(rng, length, D, paired)
            for name, a, b, want in pairs:
                assert ref.near(a, b, D) == want, (length, name)
            nodes = flat(pairs)
            if length <= 4:                                    # lengths round D + 1, where segments are empty: every read there is
                mate2 = template(rng, mate2_length(length))
                nodes += [(m, mate2) if paired else (m,) for m in every_short_read(length)]
            records = scattered(rng, nodes)
            check(e, records, D, rng=rng)                      # ragged
            check(e, records, D, uniform=True, align=length % 16)
            everything += records
        rng.shuffle(everything)
        check(e, everything, D, rng=rng)                       # all lengths in one input: shapes meet


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_reads_at_every_start_alignment(paired):
    rng = random.Random(200)
    D = 2
    records = scattered(rng, flat(difference_pairs(rng, 33, D, paired)))
    ragged = scattered(rng, flat(difference_pairs(rng, 33, D, paired) + difference_pairs(rng, 150, D, paired)))
    with Engine(segments=2 if paired else 1) as e:
        for align in range(16):
            check(e, records, D, uniform=True, align=align)
            check(e, ragged, D, align=align)


@pytest.mark.parametrize("D", DS)
def test_nodes_of_different_shape_are_never_merged(D):
    rng = random.Random(300 + D)
    t = template(rng, 60)
    with Engine(segments=1) as e:
        records = [(t[:k],) for k in (60, 59, 58, 57, 30, 1, 0)] * 2      # same bytes, different lengths
        got, info = merge(e, records, D)
        assert list(got) == list(range(7)) * 2 and info.merged == 7
        check(e, records, D)
    with Engine(segments=2) as e:
        records = [(b"ACG", b"T"), (b"AC", b"GT"), (b"A", b"CGT"), (b"ACGT", b""), (b"", b"ACGT"), (b"AC", b"GT")]      # one concatenation
        got, info = merge(e, records, D)
        assert list(got) == [0, 1, 2, 3, 4, 1] and info.merged == 5
        records = [(t[:40], t[40:]), (t[:41], t[41:]), (t[:40], t[40:59]), (t[:40], substituted(t[40:], [3], rng))]
        got, _ = merge(e, records, D)
        assert list(got) == [0, 1, 2, 0]
        check(e, records, D)


# ---- chains and components -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", DS)
def test_chains_stars_and_scattered_copies(D):
    rng = random.Random(400 + D)
    with Engine(segments=1) as e:
        chain = [(m,) for m in chain_nodes(rng, D)]
        assert not ref.near(chain[0], chain[2], D)
        for order in (chain, chain[::-1], chain[20:] + chain[:20], chain[20::-1] + chain[21:]):     # the lowest record at either end and in the middle
            got, info = merge(e, order, D)
            assert not got.any() and info.merged == 1 and 0 < info.sweeps < 39
            check(e, order, D)
            check(e, order[:5] + scattered(rng, order), D)
        star = [(m,) for m in star_nodes(rng, D)]
        for order in (star, star[::-1], star[1:16] + star[:1] + star[16:]):
            got, info = merge(e, order, D)
            assert not got.any() and info.merged == 1
            check(e, scattered(rng, order), D)
        both = scattered(rng, chain + star + [(m,) for m in chain_nodes(rng, D, links=7)])
        info = check(e, both, D)
        assert info.merged == 3
    with Engine(segments=2) as e:                                # a chain through mate 2, a star in mate 1
        mate = template(rng, 31)
        records = scattered(rng, [(mate, m) for m in chain_nodes(rng, D)] + [(m, mate) for m in star_nodes(rng, D)])
        assert check(e, records, D).merged == 2


# ---- seed groups -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", DS)
def test_seed_groups_round_the_lanes_the_wave_and_the_limit(D):
    rng = random.Random(500 + D)
    with Engine(segments=1) as e:
        for size in GROUP_SIZES:
            records = group_records(rng, D, size)
            info = check(e, records, D)                        # (asserts, through the statement, that the largest group is within the limit)
            assert info.largest_group == size
            assert info.merged == size - (1 if size >= 2 else 0)      # two components in one group and no edge between them; one near pair
        records = group_records(rng, D, 8)
        records += records[3:6]
        check(e, records, D)
    with Engine(segments=2) as e:
        for size in (9, 257):
            assert check(e, group_records(rng, D, size, paired=True), D).largest_group == size


@pytest.mark.parametrize("D", DS)
def test_a_group_beyond_the_limit_is_reported(D):
    rng = random.Random(600 + D)
    with Engine(segments=1) as e:
        records = group_records(rng, D, ref.MAX_GROUP + 1)
        lowest, entries = ref.over_limit(records, D)
        assert entries == ref.MAX_GROUP + 1
        _, info = merge(e, records, D)
        assert (info.over_limit_first, info.over_limit_nodes, info.largest_group) == (lowest, entries, entries)
        assert (info.merged, info.pairs, info.edges, info.sweeps) == (0, 0, 0, 0)
        # the lowest first record among the group's nodes, wherever it stands in the sorted group, and copies do not count
        records = records[7:] + records[:7]
        records = records[:100] + records[:50] + records[100:]
        assert ref.over_limit(records, D)[1] == ref.MAX_GROUP + 1
        _, info = merge(e, records, D)
        assert (info.over_limit_first, info.over_limit_nodes) == ref.over_limit(records, D)


# ---- weak seeds, the edge list's room, random inputs ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", DS)
def test_weak_seeds_change_nothing(D):
    rng = random.Random(700 + D)
    records = random_records(rng, D, nodes=2000, templates=200)
    with Engine(segments=1) as e:
        plain = check(e, records, D, rng=rng)
        got, _ = merge(e, records, D)
        weak = check(e, records, D, flags=_lib.NEAR_WEAK_SEEDS, rng=rng)
        got_weak, _ = merge(e, records, D, flags=_lib.NEAR_WEAK_SEEDS)
    assert np.array_equal(got, got_weak)
    assert weak.groups <= 16 and weak.pairs > plain.pairs and weak.merged == plain.merged
    same_node = sum(c * (c - 1) // 2 for g in ref.seed_groups(records, D, True).values() for c in Counter(g).values())
    assert same_node > 0                                        # entries of one node met in one group, and were skipped


@pytest.mark.parametrize("room", [1, 7, 1000000])
def test_the_edge_list_regrows(monkeypatch, room):
    rng = random.Random(800)
    D = 2
    records = scattered(rng, [(m,) for m in chain_nodes(rng, D) + star_nodes(rng, D)])
    with Engine(segments=1) as e:
        want = check(e, records, D)
        assert want.edges > 7
        monkeypatch.setenv("FQD_NEAR_EDGE_ROOM", str(room))
        info = check(e, records, D)
        assert (info.edges, info.pairs, info.sweeps, info.merged) == (want.edges, want.pairs, want.sweeps, want.merged)


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("D", DS)
def test_random_inputs(D, paired):
    rng = random.Random(900 + D + 10 * paired)
    records = random_records(rng, D, paired=paired)
    with Engine(segments=2 if paired else 1) as e:
        info = check(e, records, D, rng=rng)
    assert 0 < info.merged < info.nodes


# ---- degenerate inputs, misuse ---------------------------------------------------------------------------------------------------------------

def test_degenerate_inputs():
    rng = random.Random(1000)
    with Engine(segments=1) as e:
        for D in DS:
            info = e.near_merge(None, None, 0, D, None)
            assert (info.nodes, info.merged, info.over_limit_first, info.max_group) == (0, 0, ref.NO_RECORD, ref.MAX_GROUP)
            check(e, [(template(rng, 50),)], D)
            check(e, [(b"",)], D)
            singles = [(template(rng, 40),) for _ in range(300)]
            assert check(e, singles, D).merged == 300
            assert check(e, singles, D, uniform=True).edges == 0
            assert check(e, [singles[0]] * 300, D).nodes == 1
    with Engine(segments=2) as e:
        check(e, [(b"", b"")] * 3 + [(b"A", b"")], 1)


def test_misuse_is_refused():
    rng = random.Random(1100)
    records = [(template(rng, 20),) for _ in range(64)]
    n = len(records)
    segs, alive = placed(records)
    owner = dev(ref.exact_owners(records))
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    with Engine(segments=1) as e:
        e.near_merge(segs, owner, n, 1, out)
        e.sync()
        out.zero_()
        for distance in (0, 4, 0xFFFFFFFF):
            with pytest.raises(FqdError):
                e.near_merge(segs, owner, n, distance, out)
        bad = [lambda: e.near_merge(segs, owner, n, 1, out, flags=2),
               lambda: e.near_merge(segs, owner, n, 1, out, out=None),
               lambda: e.near_merge(segs, owner, n, 1, None),
               lambda: e.near_merge(segs, None, n, 1, out),
               lambda: e.near_merge(segs, owner, 1 << 31, 1, out),
               lambda: e.near_merge(segs, owner, n, 1, owner),                           # owner_out overlaps an input
               lambda: e.near_merge(segs, owner, n, 1, segs[0].lengths),
               lambda: e.near_merge(segs, owner, n - 8, 1, segs[0].offsets[8:].view(torch.int32)),
               lambda: e.near_merge([Reads(segs[0].bases, segs[0].offsets, None)], owner, n, 1, out),
               lambda: e.near_merge(segs, np.zeros(n, np.uint32), n, 1, out),               # host memory
               lambda: e.near_merge(segs, dev(np.arange(1, n + 1, dtype=np.uint32)), n, 1, out),      # owners above their records
               lambda: e.near_merge(segs, dev(np.maximum(np.arange(n, dtype=np.int64) - 1, 0).astype(np.uint32)), n, 1, out)]      # owners that are owned
        for k, call in enumerate(bad):
            with pytest.raises(FqdError):
                call()
            assert not out.cpu().numpy().any(), k                # nothing was written
        uniform, alive2 = placed(records, uniform=True)
        with pytest.raises(FqdError):
            e.near_merge(uniform, owner, n, 1, uniform[0].bases[4:4 + 4 * n].view(torch.int32))
        e.near_merge(segs, owner, n, 3, out)                      # the engine is as good as before
    del alive, alive2


# ---- against what is already here ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_tail_hamming_clusters_lie_inside_the_merged_ones(paired):
    rng = random.Random(1200 + paired)
    D = 2
    records = random_records(rng, D, nodes=1500, templates=150, paired=paired)
    n = len(records)
    with Engine(segments=2 if paired else 1) as e:
        segs, alive = placed(records, gap=b"\n")                # (the sequence sort reads the '\n' behind every read)
        out = torch.empty(n, dtype=torch.int32, device="cuda")
        info = e.near_merge(segs, dev(ref.exact_owners(records)), n, D, out)
        mates = [(s.bases, s.offsets, s.lengths, n) for s in segs]
        perm = torch.empty(n, dtype=torch.int32, device="cuda")
        head = torch.empty(n, dtype=torch.uint8, device="cuda")
        e.sort_seqs(mates[0], perm, mates[1] if paired else None)
        heads = e.seq_heads(mates[0], perm, _lib.SEQ_HAMMING, D, head, mates[1] if paired else None)
        e.sync()
    merged, perm, head = out.cpu().numpy().view(np.uint32), perm.cpu().numpy().view(np.uint32), head.cpu().numpy()
    assert info.merged <= heads
    at = -1
    for k in range(n):
        if head[k]:
            at = int(perm[k])
        else:
            assert ref.near(records[at], records[int(perm[k])], D)      # what tail-hamming joins to a head is near that head
        assert merged[perm[k]] == merged[at]


# ---- through the engine -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_submit_owners_merge_group(paired):
    rng = random.Random(1300 + paired)
    D = 3
    records = random_records(rng, D, nodes=1200, templates=100, paired=paired)
    n = len(records)
    want, nodes, merged = ref.merged_owners(records, D)
    with Engine(segments=2 if paired else 1) as e:
        segs, alive = placed(records, rng=rng)
        keep, link = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        owner, out, perm = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
        head = torch.empty(n, dtype=torch.uint8, device="cuda")
        e.submit_linked(segs, n, keep, link, last=True)
        e.owners(keep, link, n, owner)
        info = e.near_merge(segs, owner, n, D, out)
        e.owners_to_keep(out, n, keep)
        clusters = e.group_owners(out, n, perm, head)
        e.sync()
    assert np.array_equal(owner.cpu().numpy().view(np.uint32), ref.exact_owners(records))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    assert (info.nodes, info.merged, clusters, int(keep.sum())) == (nodes, merged, merged, merged)
