"""fqd_prefix_merge (csrc/fqd_prefix.hip) through the binding, exactly against the sequential statement
(tests/prefix_reference.py: exact clusters, every eligible node held against every other, the parent rule, the trees): every
merged owner, every count of the info, every span, and nothing written behind the last entry of either array.  Single-end and
paired.  Short-node lengths round the sixteen-byte chunk and the rounds of eight lanes with the long node 1, 16 and 129 bytes
longer, ragged reads at every start alignment and uniform reads; a difference at the overlap's last byte, at byte L, inside
the first L and in the first byte behind the overlap; mates of exactly L and of L - 1 bytes; same-sided and opposite-sided
pairs; stars, two maximal reads over one short one, chains and a child that owns its cluster; seed groups round the lane, wave
and limit sizes and one entry beyond the limit; weak seeds; random inputs; degenerate inputs and misuse."""
import random

import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, Reads, _lib
from fastq_dupaway_amd._lib import FqdError
import prefix_reference as ref
from prefix_cases import (EXTRA, GROUP_SIZES, as_records, chain, eligibility, group_records, pair_directions, random_records, scattered, short_lengths, star,
                          template, truncations, two_maximal)

pytestmark = pytest.mark.gpu
FILL = 0xEE
GUARD = 8                                                      # entries behind the last one of owner_out and span_out
NONE32 = 0xFFFFFFFF
LS = [1, 20, 32]


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def placed(records, uniform=False, align=0, rng=None):
    """The records' mates in device memory as Reads: ragged — back to back from byte `align` on, FILL in between where rng says
    so, and one byte behind the last read — or uniform, every read at a stride of its length + 3.  Returns (segs, what must
    stay alive)."""
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
        gaps = [bytes([FILL]) * (rng.randrange(4) if rng else 0) for _ in mates]
        offs = np.zeros(n, np.uint64)
        at, parts = align, [bytes([FILL]) * align]
        for k, m in enumerate(mates):
            offs[k] = at
            parts += [m, gaps[k]]
            at += len(m) + len(gaps[k])
        buf, d_off, d_len = dev(np.frombuffer(b"".join(parts) + b"\0", np.uint8).copy()), dev(offs), dev(lens)
        segs.append(Reads(buf, d_off, d_len))
        alive += [buf, d_off, d_len]
    return segs, alive


def merge(e, records, L, flags=0, span=True, **how):
    n = len(records)
    segs, alive = placed(records, **how)
    owner = dev(ref.exact_owners(records))
    out = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    spans = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda") if span else None
    info = e.prefix_merge(segs, owner, n, L, out, spans, flags)
    e.sync()
    got = out.cpu().numpy().view(np.uint32)
    assert np.all(got[n:] == NONE32)                           # nothing behind the last entry
    if span:
        got_spans = spans.cpu().numpy().view(np.uint32)
        assert np.all(got_spans[n:] == NONE32)
        if info.over_limit_first == ref.NO_RECORD:
            assert np.array_equal(got_spans[:n], ref.spans(records))
    return got[:n], info


def check(e, records, L, flags=0, **how):
    """One call against the statement; returns the info."""
    weak = bool(flags & _lib.PREFIX_WEAK_SEEDS)
    want, counts = ref.merged_owners(records, L)
    groups, largest, pairs, related = ref.group_counts(records, L, weak)
    assert largest <= ref.MAX_GROUP                            # before the GPU is asked
    got, info = merge(e, records, L, flags, **how)
    assert (info.max_group, info.over_limit_first, info.over_limit_nodes) == (ref.MAX_GROUP, ref.NO_RECORD, 0)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (L, bad[:10], got[bad[:10]], want[bad[:10]], [records[i] for i in bad[:3]])
    assert {k: getattr(info, k) for k in counts} == counts
    assert (info.groups, info.largest_group, info.pairs, info.related) == (groups, largest, pairs, related)
    return info


# ---- lengths, alignments, where the differences fall ---------------------------------------------------------------------------------

@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("L", LS)
def test_every_length_with_the_differences_where_they_matter(L, paired):
    rng = random.Random(100 + L)
    everything = []
    with Engine(segments=2 if paired else 1) as e:
        for short in short_lengths(L):
            cases = [c for extra in EXTRA for c in truncations(rng, L, short, extra)]
            for name, nodes, related in cases:
                fit = list(range(len(nodes)))
                assert len(ref.all_pairs([(m,) for m in nodes], fit)) == related, (short, name)
            for cut_mate in (0, 1) if paired else (0,):
                records = scattered(rng, as_records(rng, L, cases, paired, cut_mate))
                info = check(e, records, L, rng=rng)
                assert info.related >= sum(r for *_, r in cases) and info.merged < info.nodes      # (more: at L = 1 a read of one byte begins many)
                everything += records
        rng.shuffle(everything)
        check(e, everything, L, rng=rng)                       # all lengths in one input


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_reads_at_every_start_alignment(paired):
    rng = random.Random(200)
    L = 20
    cases = [c for short in (20, 33, 144) for c in truncations(rng, L, short, 16)]
    records = scattered(rng, as_records(rng, L, cases, paired))
    with Engine(segments=2 if paired else 1) as e:
        for align in range(16):
            check(e, records, L, align=align)


def test_uniform_reads_are_never_related():
    rng = random.Random(300)
    nodes = [(template(rng, 12) + template(rng, 38),) for _ in range(40)]
    records = scattered(rng, nodes + [(nodes[0][0][:49] + b"N",)])
    with Engine(segments=1) as e:
        for align in (0, 5):
            info = check(e, records, 12, uniform=True, align=align)
            assert info.merged == info.nodes == 41 and (info.pairs, info.related, info.children, info.deepest, info.jumps) == (0, 0, 0, 0, 0)
        same_start = [(nodes[0][0][:20] + template(rng, 30),) for _ in range(30)]
        info = check(e, same_start, 20, uniform=True)          # one group of one shape: nothing is compared
        assert (info.largest_group, info.pairs, info.merged) == (30, 0, 30)


@pytest.mark.parametrize("L", LS)
def test_mates_of_exactly_L_bytes_and_of_one_less(L):
    rng = random.Random(400 + L)
    for paired in (False, True):
        records, clusters = eligibility(rng, L, paired)
        with Engine(segments=2 if paired else 1) as e:
            assert check(e, records, L, rng=rng).merged == clusters
            assert check(e, records[::-1], L).merged == clusters


@pytest.mark.parametrize("L", LS)
def test_pairs_same_sided_and_opposite_sided(L):
    rng = random.Random(500 + L)
    records, clusters = pair_directions(rng, L)
    with Engine(segments=2) as e:
        assert check(e, records, L, rng=rng).merged == clusters
        assert check(e, scattered(rng, records), L, rng=rng).merged == clusters


# ---- structure -------------------------------------------------------------------------------------------------------------------------

def test_a_star_goes_to_the_least_span_and_the_lowest_record():
    rng = random.Random(600)
    L = 24
    records, short, parent = star(rng, L)
    with Engine(segments=1) as e:
        got, info = merge(e, records, L)
        assert list(got) == [0, 1, 2, 3, 4, parent] and (info.related, info.children, info.merged) == (5, 1, 5)
        check(e, records, L)
        turned = records[::-1]                                 # the short read first: it owns the cluster of its parent
        got, _ = merge(e, turned, L)
        assert list(got) == [0, 1, 2, 0, 4, 5]                 # (of the two shortest long reads the lower record: place 3)
        check(e, turned, L)
        check(e, scattered(rng, records), L, rng=rng)


def test_two_maximal_reads_over_one_short_read_stay_apart():
    rng = random.Random(700)
    L = 32
    records = two_maximal(rng, L)
    with Engine(segments=1) as e:
        got, info = merge(e, records, L)
        assert list(got) == [0, 0, 2] and (info.merged, info.related, info.children) == (2, 2, 1)
        check(e, records, L)
        got, _ = merge(e, [records[1], records[2], records[0]], L)
        assert list(got) == [0, 0, 2]                          # the short read first: with the first of the two, and it owns the cluster


@pytest.mark.parametrize("depth", list(range(1, 10)) + [64])
def test_chains(depth):
    rng = random.Random(800 + depth)
    L = 17
    with Engine(segments=1) as e:
        nodes = chain(rng, L, depth)
        for order in (nodes, nodes[::-1], scattered(rng, nodes)):
            info = check(e, order, L, rng=rng)
            assert (info.deepest, info.jumps, info.merged, info.children) == (depth, ref.jumps_for(depth), 1, depth)
            assert info.related == depth * (depth + 1) // 2    # every node is a prefix of every longer one
        both = scattered(rng, nodes + chain(rng, L, 3) + [(template(rng, L - 1),), (template(rng, 90),)])
        info = check(e, both, L, rng=rng)
        assert (info.deepest, info.merged) == (max(depth, 3), 4)
    with Engine(segments=2) as e:
        info = check(e, scattered(rng, chain(rng, L, depth, paired=True)), L, rng=rng)
        assert (info.deepest, info.merged) == (depth, 1)


# ---- seed groups -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", GROUP_SIZES)
def test_seed_groups_round_the_lanes_the_wave_and_the_limit(size):
    rng = random.Random(900 + size)
    L = 16
    with Engine(segments=1) as e:
        info = check(e, group_records(rng, L, size), L)
        assert (info.largest_group, info.groups, info.related, info.merged) == (size, 1, 1, size - 1)
    if size <= 65:
        with Engine(segments=2) as e:
            assert check(e, group_records(rng, L, size, paired=True), L).largest_group == size


def test_a_group_beyond_the_limit_is_reported():
    rng = random.Random(1000)
    L = 16
    with Engine(segments=1) as e:
        records = group_records(rng, L, ref.MAX_GROUP + 1)
        lowest, entries = ref.over_limit(records, L)
        assert entries == ref.MAX_GROUP + 1
        _, info = merge(e, records, L)
        assert (info.over_limit_first, info.over_limit_nodes, info.largest_group) == (lowest, entries, entries)
        assert (info.merged, info.pairs, info.related, info.children, info.deepest, info.jumps) == (0, 0, 0, 0, 0, 0)
        # the lowest first record among the group's nodes, wherever it stands in the sorted group, and copies do not count
        records = records[7:] + records[:7]
        records = records[:100] + records[:50] + records[100:]
        assert ref.over_limit(records, L)[1] == ref.MAX_GROUP + 1
        _, info = merge(e, records, L)
        assert (info.over_limit_first, info.over_limit_nodes) == ref.over_limit(records, L)


# ---- weak seeds, random inputs -----------------------------------------------------------------------------------------------------------

def test_weak_seeds_change_nothing():
    rng = random.Random(1100)
    L = 20
    records = random_records(rng, L, nodes=2000, templates=200)
    with Engine(segments=1) as e:
        plain = check(e, records, L, rng=rng)
        got, _ = merge(e, records, L)
        weak = check(e, records, L, flags=_lib.PREFIX_WEAK_SEEDS, rng=rng)
        got_weak, _ = merge(e, records, L, flags=_lib.PREFIX_WEAK_SEEDS)
    assert np.array_equal(got, got_weak)
    assert weak.groups <= 16 and weak.pairs > plain.pairs
    assert (weak.merged, weak.related, weak.children, weak.deepest, weak.jumps) == (plain.merged, plain.related, plain.children, plain.deepest, plain.jumps)


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("L", LS)
def test_random_inputs(L, paired):
    rng = random.Random(1200 + L + 100 * paired)
    records = random_records(rng, L, nodes=2000, templates=40 if L == 1 else 200, paired=paired)
    with Engine(segments=2 if paired else 1) as e:
        info = check(e, records, L, rng=rng)
        info_no_span = e.prefix_merge(*placed(records)[:1], dev(ref.exact_owners(records)), len(records), L,
                                      torch.empty(len(records), dtype=torch.int32, device="cuda"))      # span_out left out
    assert 0 < info.merged < info.nodes and info.deepest >= 2
    assert (info_no_span.merged, info_no_span.related) == (info.merged, info.related)


# ---- degenerate inputs, misuse ---------------------------------------------------------------------------------------------------------------

def test_degenerate_inputs():
    rng = random.Random(1300)
    with Engine(segments=1) as e:
        for L in LS:
            info = e.prefix_merge(None, None, 0, L, None)
            assert (info.nodes, info.merged, info.over_limit_first, info.max_group) == (0, 0, ref.NO_RECORD, ref.MAX_GROUP)
            assert check(e, [(template(rng, 50),)], L).merged == 1
            info = check(e, [(b"",)], L)                        # one record, not eligible: no entry at all
            assert (info.nodes, info.eligible, info.groups, info.merged) == (1, 0, 0, 1)
            assert check(e, [(template(rng, 40),)] * 300, L).nodes == 1
        info = check(e, [(template(rng, 9),) for _ in range(300)], 10)      # nobody is eligible
        assert (info.eligible, info.merged) == (0, info.nodes)
    with Engine(segments=2) as e:
        check(e, [(b"", b"")] * 3 + [(b"A", b"")] + [(b"A", b"C"), (b"AG", b"C"), (b"AG", b"CT")], 1)


def test_misuse_is_refused():
    rng = random.Random(1400)
    records = [(template(rng, 20),) for _ in range(64)]
    n = len(records)
    segs, alive = placed(records)
    owner = dev(ref.exact_owners(records))
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    spans = torch.zeros(n, dtype=torch.int32, device="cuda")
    with Engine(segments=1) as e:
        e.prefix_merge(segs, owner, n, 10, out, spans)
        e.sync()
        out.zero_(); spans.zero_()
        for L in (0, 65536, 0xFFFFFFFF):
            with pytest.raises(FqdError):
                e.prefix_merge(segs, owner, n, L, out, spans)
        bad = [lambda: e.prefix_merge(segs, owner, n, 10, out, spans, flags=2),           # a flag that does not exist
               lambda: e.prefix_merge(segs, owner, n, 10, out, spans, out=None),
               lambda: e.prefix_merge(segs, owner, n, 10, None, spans),
               lambda: e.prefix_merge(segs, None, n, 10, out, spans),
               lambda: e.prefix_merge(segs, owner, 1 << 31, 10, out, spans),
               lambda: e.prefix_merge(segs, owner, n, 10, owner, spans),                  # owner_out over an input
               lambda: e.prefix_merge(segs, owner, n, 10, segs[0].lengths, spans),
               lambda: e.prefix_merge(segs, owner, n, 10, out, owner),                    # span_out over an input
               lambda: e.prefix_merge(segs, owner, n, 10, out, out),                      # ... and over owner_out
               lambda: e.prefix_merge(segs, owner, n - 8, 10, segs[0].offsets[8:].view(torch.int32), spans),
               lambda: e.prefix_merge([Reads(segs[0].bases, segs[0].offsets, None)], owner, n, 10, out, spans),
               lambda: e.prefix_merge(segs, np.zeros(n, np.uint32), n, 10, out, spans),      # host memory
               lambda: e.prefix_merge(segs, owner, n, 10, out, np.zeros(n, np.uint32)),
               lambda: e.prefix_merge(segs, dev(np.arange(1, n + 1, dtype=np.uint32)), n, 10, out, spans),      # owners above their records
               lambda: e.prefix_merge(segs, dev(np.maximum(np.arange(n, dtype=np.int64) - 1, 0).astype(np.uint32)), n, 10, out, spans),      # owners that are owned
               lambda: e.prefix_merge([Reads(segs[0].bases, uniform_len=1 << 31, uniform_stride=1 << 31)], owner, n, 10, out, spans)]
        for k, call in enumerate(bad):
            with pytest.raises(FqdError):
                call()
            assert not out.cpu().numpy().any() and not spans.cpu().numpy().any(), k      # nothing was written
        uniform, alive2 = placed(records, uniform=True)
        with pytest.raises(FqdError):
            e.prefix_merge(uniform, owner, n, 10, uniform[0].bases[4:4 + 4 * n].view(torch.int32))
        assert e.prefix_merge(segs, owner, n, 20, out, spans).nodes == n      # the engine is as good as before
    del alive, alive2


# ---- through the engine -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_submit_owners_merge_group(paired):
    rng = random.Random(1500 + paired)
    L = 25
    records = random_records(rng, L, nodes=1200, templates=100, paired=paired)
    n = len(records)
    want, counts = ref.merged_owners(records, L)
    with Engine(segments=2 if paired else 1) as e:
        segs, alive = placed(records, rng=rng)
        keep, link = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        owner, out, perm = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
        head = torch.empty(n, dtype=torch.uint8, device="cuda")
        e.submit_linked(segs, n, keep, link, last=True)
        e.owners(keep, link, n, owner)
        info = e.prefix_merge(segs, owner, n, L, out)
        e.owners_to_keep(out, n, keep)
        clusters = e.group_owners(out, n, perm, head)
        e.sync()
    assert np.array_equal(owner.cpu().numpy().view(np.uint32), ref.exact_owners(records))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    assert (info.nodes, info.merged, clusters, int(keep.sum())) == (counts["nodes"], counts["merged"], counts["merged"], counts["merged"])
