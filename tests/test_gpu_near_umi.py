"""fqd_near_merge_umi (csrc/fqd_near.hip) through the binding, exactly against the sequential statement
(tests/near_umi_reference.py: exact clusters by tag and mates, all pairs of equal tag and shape compared, union-find, the links
joined): every owner, the counts of the info, nothing written behind the last entry.  A record is (U, mates).  The tag: every
UMI length round the eight-byte word, U at every offset in its line and at the line's end, tags that differ in one byte or in
a joiner's character only, one sequence under 5000 UMIs, a seed group at and one beyond the limit under one UMI.  The reads:
lengths round the segments, the sixteen-byte chunk and the rounds of eight lanes with exactly D and D + 1 differences, under
equal and unequal tags, single-end and paired, ragged and uniform.  Weak seeds.  The links: none, a molecule that exists only
through one, the edge list's regrowth, fqd_umi_merge's owners; misuse; random inputs."""
import random

import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, Reads, _lib
from fastq_dupaway_amd._lib import FqdError
import near_reference as near
import near_umi_reference as ref
import umi_merge_reference as umi_merge
import umi_reference as umi
from near_cases import chain_nodes, difference_pairs, group_records, mate2_length, random_records, scattered, star_nodes, substituted, template

pytestmark = pytest.mark.gpu
FILL = 0xEE
GUARD = 8                                                      # entries behind the last one of owner_out
NONE32 = 0xFFFFFFFF
DS = [1, 2, 3]
UMI_LENGTHS = [1, 7, 8, 9, 15, 16, 17, 63, 64]


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def placed(mates_of, uniform=False, align=0, rng=None):
    """The records' mates in device memory as Reads: ragged — back to back from byte `align` on, FILL in between where rng says
    so — or uniform, every read at a stride of its length + 3.  Returns (segs, what must stay alive)."""
    n, segs, alive = len(mates_of), [], []
    for s in range(len(mates_of[0])):
        mates = [r[s] for r in mates_of]
        lens = np.array([len(m) for m in mates], np.uint32)
        if uniform:
            assert len(set(lens.tolist())) == 1
            body = b"".join(m + bytes([FILL]) * 3 for m in mates)
            buf = dev(np.frombuffer(bytes([FILL]) * align + body, np.uint8).copy())
            segs.append(Reads(buf[align:], uniform_len=int(lens[0]), uniform_stride=int(lens[0]) + 3))
            alive.append(buf)
            continue
        offs = np.zeros(n, np.uint64)
        at, parts = align, [bytes([FILL]) * align]
        for k, m in enumerate(mates):
            gap = bytes([FILL]) * (rng.randrange(4) if rng else 0)
            offs[k] = at
            parts += [m, gap]
            at += len(m) + len(gap)
        buf, d_off, d_len = dev(np.frombuffer(b"".join(parts) + b"\0" * 16, np.uint8).copy()), dev(offs), dev(lens)
        segs.append(Reads(buf, d_off, d_len))
        alive += [buf, d_off, d_len]
    return segs, alive


def id_lines(records, rng, offset=None, at_line_end=None):
    """File 1's ID lines as fqd_umi_find leaves them: (text, id_start, umi_off).  Line i is '@', bytes that differ from record to
    record, U, and either '\\n' at once (U ends at the line's last byte in front of it) or a comment of its own: a load that
    leaves U reads something that two records of one tag do not share.  offset: where U starts in its line (0: the line is U)."""
    text, starts, offs = bytearray(), [], []
    for u, _ in records:
        off = rng.randrange(1, 24) if offset is None else offset
        front = (b"@" + bytes(rng.choice(b"abcdefgh0123456789:") for _ in range(off - 1))) if off else b""
        end = rng.random() < 0.5 if at_line_end is None else at_line_end
        back = b"\n" if end else b" " + bytes(rng.choice(b"ACGTN+-_:1") for _ in range(rng.randrange(1, 12))) + b"\n"
        starts.append(len(text))
        offs.append(off)
        text += front + u + back
    return dev(np.frombuffer(bytes(text), np.uint8).copy()), dev(np.array(starts, np.uint64)), dev(np.array(offs, np.uint32))


def info_of(umi_len, joiners):
    return _lib.UmiInfo(n_bases=umi_len - bin(joiners).count("1"), umi_len=umi_len, joiners=joiners, bad_record=ref.NO_RECORD, bad_reason=0, reserved=0)


def shape_of(records):
    lengths = {len(u) for u, _ in records}
    shapes = {ref.joiners_of(u) for u, _ in records}
    assert len(lengths) == 1 and len(shapes) == 1                # one shape a run
    return lengths.pop(), shapes.pop()


def merge(e, records, D, link=None, flags=0, rng=None, offset=None, at_line_end=None, **how):
    n = len(records)
    rng = rng or random.Random(n)
    umi_len, joiners = shape_of(records)
    segs, alive = placed([m for _, m in records], rng=None if how.get("uniform") else rng, **how)
    text, id_start, umi_off = id_lines(records, rng, offset, at_line_end)
    owner = dev(ref.exact_owners(records, joiners))
    out = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    info = e.near_merge_umi(segs, owner, dev(np.asarray(link, np.uint32)) if link is not None else None, n, D, text, id_start, umi_off,
                            info_of(umi_len, joiners), out, flags)
    e.sync()
    got = out.cpu().numpy().view(np.uint32)
    assert np.all(got[n:] == NONE32)                           # nothing behind the last entry
    return got[:n], info


def check(e, records, D, link=None, flags=0, **how):
    """One call against the statement; returns the info."""
    got, info = merge(e, records, D, link, flags, **how)
    _, joiners = shape_of(records)
    want, nodes, molecules, links = ref.molecules(records, D, joiners, link)
    assert (info.near.nodes, info.near.entries, info.near.max_group, info.near.over_limit_first) == (nodes, nodes * (D + 1), ref.MAX_GROUP, ref.NO_RECORD)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (D, bad[:10], got[bad[:10]], want[bad[:10]], [records[i] for i in bad[:3]])
    assert (info.near.merged, info.links) == (molecules, links)
    weak = bool(flags & _lib.NEAR_WEAK_SEEDS)
    groups = ref.seed_groups(records, D, joiners, weak)
    assert (info.near.groups, info.near.largest_group) == (len(groups), max(len(g) for g in groups.values()))
    assert info.near.pairs == ref.expected_pairs(records, D, joiners, weak)
    assert nodes - molecules - links <= info.near.edges <= info.near.pairs      # with the links a spanning forest at least
    return info


def random_umi(rng, length, joiners=0, alphabet=b"ACGT"):
    return bytes(rng.choice(b"+-_") if (joiners >> p) & 1 else rng.choice(alphabet) for p in range(length))


def joiner_shapes(length):
    """Joiner sets of a UMI of `length` bytes that leave a base: none, the first place, the last, round a word boundary."""
    sets = [0, 1, 1 << (length - 1)] + [(1 << (k - 1)) | (1 << k) for k in range(8, length, 8)]
    return sorted({j for j in sets if bin(j).count("1") < length})


# ---- the tag -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("umi_len", UMI_LENGTHS)
def test_tags_at_every_length(umi_len):
    rng = random.Random(100 + umi_len)
    D = 2
    s = template(rng, 40)
    s1, s2, far = substituted(s, [3], rng), substituted(s, [20, 39], rng), substituted(s, [10, 11, 12], rng)
    with Engine(segments=1) as e:
        for joiners in joiner_shapes(umi_len):
            u = random_umi(rng, umi_len, joiners)
            bases = [p for p in range(umi_len) if not (joiners >> p) & 1]
            others = []                                          # tags that differ from u's in one byte only
            for p in sorted({bases[0], bases[-1]} | {q for q in bases if q % 8 in (0, 7)}):
                others.append(bytes(c if k != p else (ord("A") if c != ord("A") else ord("C")) for k, c in enumerate(u)))
            same = bytes((ord("-") if c == ord("+") else ord("+")) if (joiners >> k) & 1 else c for k, c in enumerate(u))     # another joiner character
            records = [(u, (s,)), (same, (s1,)), (u, (s2,)), (u, (far,)), (same, (s,))]
            for o in others:
                records += [(o, (s,)), (o, (s1,))]
            records = scattered(rng, records)
            info = check(e, records, D, rng=rng)
            # u's four sequences are two molecules (s, s1, s2 hang together, far does not), every other tag's two are one
            assert info.near.merged == 2 + len(others), (umi_len, hex(joiners))
            assert info.near.nodes == 4 + 2 * len(others)


@pytest.mark.parametrize("umi_len", [8, 17, 64])
def test_the_umi_at_every_offset_and_at_the_line_end(umi_len):
    rng = random.Random(200 + umi_len)
    D = 1
    s = template(rng, 33)
    umis = [random_umi(rng, umi_len) for _ in range(6)]
    records = scattered(rng, [(u, (m,)) for u in umis for m in (s, substituted(s, [7], rng), substituted(s, [1, 30], rng))])
    with Engine(segments=1) as e:
        for offset in range(16):
            for at_line_end in (True, False):
                info = check(e, records, D, rng=rng, offset=offset, at_line_end=at_line_end)
                assert info.near.merged == 12


def test_one_sequence_under_5000_umis_is_5000_groups_of_one():
    rng = random.Random(300)
    umis = set()
    while len(umis) < 5000:
        umis.add(random_umi(rng, 10))
    s = template(rng, 100)
    records = [(u, (s,)) for u in sorted(umis)]
    rng.shuffle(records)
    records += records[:200]
    with Engine(segments=1) as e:
        for D in DS:
            got, info = merge(e, records, D, rng=rng)
            assert info.near.over_limit_first == ref.NO_RECORD                           # no refusal
            assert (info.near.nodes, info.near.merged, info.near.edges) == (5000, 5000, 0)      # no merge
            assert info.near.largest_group == 1 and info.near.pairs == 0
            assert np.array_equal(got, ref.exact_owners(records, 0))
        # the same records without their tags are ONE group, beyond the limit
        segs, alive = placed([m for _, m in records[:5000]])
        plain = e.near_merge(segs, dev(np.arange(5000, dtype=np.uint32)), 5000, 1, torch.empty(5000, dtype=torch.int32, device="cuda"))
        assert plain.nodes == 5000 and plain.over_limit_first != ref.NO_RECORD


def test_a_group_at_the_limit_is_taken_and_one_beyond_it_is_refused():
    rng = random.Random(400)
    D = 2
    u, other = b"ACGTTGCA", b"ACGTTGCC"
    with Engine(segments=1) as e:
        records = [(u, m) for m in group_records(rng, D, ref.MAX_GROUP)]
        info = check(e, records, D, rng=rng)
        assert info.near.largest_group == ref.MAX_GROUP and info.near.merged == ref.MAX_GROUP - 1
        # one more node under ANOTHER UMI is not in the group; under the same UMI it is
        records = [(u, m) for m in group_records(rng, D, ref.MAX_GROUP + 1)]
        split = [(other if k == 5 else w, m) for k, (w, m) in enumerate(records)]
        assert ref.over_limit(split, D, 0) is None
        _, info = merge(e, split, D, rng=rng)
        assert (info.near.over_limit_first, info.near.largest_group) == (ref.NO_RECORD, ref.MAX_GROUP)
        records = records[7:] + records[:7]
        records = records[:100] + records[:50] + records[100:]      # copies do not count
        lowest, entries = ref.over_limit(records, D, 0)
        assert entries == ref.MAX_GROUP + 1
        _, info = merge(e, records, D, rng=rng)
        assert (info.near.over_limit_first, info.near.over_limit_nodes, info.near.largest_group) == (lowest, entries, entries)
        assert (info.near.merged, info.near.pairs, info.near.edges, info.near.sweeps, info.links) == (0, 0, 0, 0, 0)


# ---- the reads ---------------------------------------------------------------------------------------------------------------------------

def read_lengths(D):
    return sorted({0, 1, D, D + 1, 15, 16, 17, 127, 128, 129})


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("D", DS)
def test_reads_with_d_and_d_plus_one_differences_under_equal_and_unequal_tags(D, paired):
    rng = random.Random(500 + D + 10 * paired)
    u, v = b"ACGTACGTA+TTGCA", b"ACGTACGTA+TTGCC"               # one shape, tags that differ in their last byte
    everything = []
    with Engine(segments=2 if paired else 1) as e:
        for length in read_lengths(D):
            pairs = difference_pairs(rng, length, D, paired)
            empty2 = template(rng, mate2_length(length))
            if length <= 1:                                      # too short for a difference set of D: every read of the length
                pairs += [("short", (a,) + ((empty2,) if paired else ()), (b,) + ((empty2,) if paired else ()), near.mismatches(a, b) <= D)
                          for a in ([b""] if not length else [b"A", b"C", b"N"]) for b in ([b""] if not length else [b"G"])]
            records = []
            for name, a, b, want in pairs:
                assert near.near(a, b, D) == want, (length, name)
                records += [(u, a), (u, b)]                      # under one tag: near where the statement says so
                records += [(v, b)]                              # the same sequence under another tag: never near (u, a)
            records = scattered(rng, records)
            info = check(e, records, D, rng=rng)                 # ragged
            got, _ = merge(e, records, D, rng=rng)
            tags = [ref.tag(w, 1 << 9) for w, _ in records]
            assert all(tags[i] == tags[int(got[i])] for i in range(len(records)))       # no molecule holds two tags
            check(e, records, D, uniform=True, align=length % 16)
            everything += records
        rng.shuffle(everything)
        info = check(e, everything, D, rng=rng)                  # all lengths in one input: shapes meet
        assert info.near.merged < info.near.nodes


@pytest.mark.parametrize("D", DS)
def test_chains_and_stars_under_several_umis(D):
    rng = random.Random(600 + D)
    umis = [random_umi(rng, 12) for _ in range(3)]
    chain, star = chain_nodes(rng, D), star_nodes(rng, D)
    records = scattered(rng, [(u, (m,)) for u in umis for m in chain + star])
    with Engine(segments=1) as e:
        info = check(e, records, D, rng=rng)
        assert info.near.merged == 6 and info.near.sweeps > 0   # a chain and a star under each UMI
    with Engine(segments=2) as e:                                # a chain through mate 2
        mate = template(rng, 31)
        records = scattered(rng, [(u, (mate, m)) for u in umis[:2] for m in chain])
        assert check(e, records, D, rng=rng).near.merged == 2


@pytest.mark.parametrize("D", DS)
def test_weak_seeds_make_unlike_tags_meet_and_change_nothing(D):
    rng = random.Random(700 + D)
    umis = [random_umi(rng, 9, 1 << 4) for _ in range(12)]
    records = [(rng.choice(umis), m) for m in random_records(rng, D, nodes=1500, templates=60)]
    with Engine(segments=1) as e:
        plain = check(e, records, D, rng=rng)
        got, _ = merge(e, records, D)
        weak = check(e, records, D, flags=_lib.NEAR_WEAK_SEEDS, rng=rng)
        got_weak, _ = merge(e, records, D, flags=_lib.NEAR_WEAK_SEEDS)
    assert np.array_equal(got, got_weak)
    assert weak.near.groups <= 16 and weak.near.pairs > plain.near.pairs and weak.near.merged == plain.near.merged
    # nodes of unlike tags and one sequence met in one group, and the tag compare kept them apart
    by_seq = {}
    for w, m in records:
        by_seq.setdefault(m, set()).add(ref.tag(w, 1 << 4))
    assert any(len(t) > 1 for t in by_seq.values())


# ---- the links -----------------------------------------------------------------------------------------------------------------------------

def links_of(records, distance=1):
    """fqd_umi_merge's owner_out over the records, by its statement."""
    out, info, *_ = umi_merge.merge([umi.bases(u) for u, _ in records], [m for _, m in records], distance, 4096)
    assert out is not None
    return out


@pytest.mark.parametrize("D", DS)
def test_no_link_is_the_identity(D):
    rng = random.Random(800 + D)
    umis = [random_umi(rng, 8) for _ in range(5)]
    records = [(rng.choice(umis), m) for m in random_records(rng, D, nodes=800, templates=40)]
    with Engine(segments=1) as e:
        a, none = merge(e, records, D)
        b, identity = merge(e, records, D, link=np.arange(len(records), dtype=np.uint32))
        c, owners = merge(e, records, D, link=ref.exact_owners(records, 0))
        check(e, records, D, link=np.arange(len(records), dtype=np.uint32), rng=rng)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert (none.links, identity.links, owners.links) == (0, 0, 0)
    assert (none.near.merged, none.near.edges, none.near.sweeps) == (identity.near.merged, identity.near.edges, identity.near.sweeps)


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_a_molecule_that_exists_only_through_a_link(paired):
    rng = random.Random(900 + paired)
    D = 1
    u, u1 = b"ACGTACGT", b"ACGTACGA"                             # one base apart
    s = template(rng, 60)
    s1 = substituted(s, [17], rng)
    mate2 = template(rng, 25)
    def rec(w, m):
        return (w, (m, mate2) if paired else (m,))
    records = [rec(u, s)] * 10 + [rec(u1, s), rec(u1, s1)]
    link = links_of(records)
    assert list(link) == [0] * 11 + [11]                         # (u', s) went into (u, s) by the directional rule; (u', s') stands alone
    with Engine(segments=2 if paired else 1) as e:
        got, info = merge(e, records, D, link=link)
        assert not got.any() and (info.near.merged, info.links, info.near.edges) == (1, 1, 1)
        check(e, records, D, link=link)
        got, info = merge(e, records, D)
        assert list(got) == [0] * 10 + [10, 10] and (info.near.merged, info.links) == (2, 0)
        # a copy with an error in the UMI AND in the read, and no intermediate: a molecule of its own, link or not
        records = [rec(u, s)] * 10 + [rec(u1, s1)]
        link = links_of(records)
        got, info = merge(e, records, D, link=link)
        assert list(got) == [0] * 10 + [10] and info.links == 0
        # ... and the other intermediate: (u, s') near (u, s), (u', s') linked to (u, s')
        records = [rec(u, s)] * 10 + [rec(u, s1)] * 3 + [rec(u1, s1)]
        link = links_of(records)
        assert int(link[13]) == 10
        got, info = merge(e, records, D, link=link)
        assert not got.any() and info.near.merged == 1
        check(e, records, D, link=link)


def linked_records(rng, D, nodes, templates, umis=30, paired=False):
    """Random reads under UMIs that stand one base apart in families, the counts skewed so that the directional rule links."""
    roots = [random_umi(rng, 8, 1 << 4) for _ in range(umis)]
    family = []
    for r in roots:
        family += [r] * 8 + [substituted(r, [rng.choice([0, 3, 5, 7])], rng)]
    return [(rng.choice(family), m) for m in random_records(rng, D, nodes=nodes, templates=templates, paired=paired, lengths=(30, 31, 48, 100))]


@pytest.mark.parametrize("room", [1, 7, 1000000])
def test_the_edge_list_regrows_with_links(monkeypatch, room):
    rng = random.Random(1000)
    D = 2
    records = linked_records(rng, D, nodes=1200, templates=15, umis=4)
    link = links_of(records)
    with Engine(segments=1) as e:
        want = check(e, records, D, link=link, rng=rng)
        assert want.links > 7 and want.near.edges > 7
        monkeypatch.setenv("FQD_NEAR_EDGE_ROOM", str(room))
        info = check(e, records, D, link=link, rng=rng)
        assert (info.near.edges, info.links, info.near.pairs, info.near.sweeps, info.near.merged) == \
               (want.near.edges, want.links, want.near.pairs, want.near.sweeps, want.near.merged)


def test_the_links_of_the_device_merge():
    """fqd_umi_merge's owner_out, as the device leaves it, is what the entry takes as link."""
    rng = random.Random(1100)
    D = 1
    records = linked_records(rng, D, nodes=1500, templates=20, umis=5)
    n = len(records)
    umi_len, joiners = shape_of(records)
    want_link, _, owner_exact, owner_seq, size = umi_merge.merge([umi.bases(u) for u, _ in records], [m for _, m in records], 1, 4096)
    assert np.array_equal(owner_exact, ref.exact_owners(records, joiners))
    with Engine(segments=1) as e:
        segs, alive = placed([m for _, m in records], rng=rng)
        text, id_start, umi_off = id_lines(records, rng)
        info = info_of(umi_len, joiners)
        link = torch.empty(n, dtype=torch.int32, device="cuda")
        out = torch.empty(n, dtype=torch.int32, device="cuda")
        e.umi_merge(text, id_start, umi_off, info, dev(owner_exact), dev(owner_seq), dev(size), n, 1, link)
        got = e.near_merge_umi(segs, dev(owner_exact), link, n, D, text, id_start, umi_off, info, out)
        e.sync()
    assert np.array_equal(link.cpu().numpy().view(np.uint32), want_link)
    want, nodes, molecules, links = ref.molecules(records, D, joiners, want_link)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    assert (got.near.nodes, got.near.merged, got.links) == (nodes, molecules, links) and links > 0
    assert molecules < len({int(x) for x in want_link})          # the near edges joined directional clusters


# ---- random inputs ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("D", DS)
def test_random_inputs(D, paired):
    rng = random.Random(1200 + D + 10 * paired)
    records = linked_records(rng, D, nodes=2500, templates=60, paired=paired)
    with Engine(segments=2 if paired else 1) as e:
        info = check(e, records, D, rng=rng)
        assert 0 < info.near.merged < info.near.nodes
        linked = check(e, records, D, link=links_of(records), rng=rng)
        assert linked.links > 0 and linked.near.merged < info.near.merged


def test_twenty_thousand_records():
    rng = random.Random(1300)
    D = 2
    records = linked_records(rng, D, nodes=13000, templates=400, umis=40)
    records = (records + records[:20000 - len(records)])[:20000]
    assert len(records) == 20000
    with Engine(segments=1) as e:
        info = check(e, records, D, link=links_of(records), rng=rng)
    assert info.links > 0 and 0 < info.near.merged < info.near.nodes


# ---- degenerate inputs, misuse ---------------------------------------------------------------------------------------------------------------

def test_degenerate_inputs():
    rng = random.Random(1400)
    with Engine(segments=1) as e:
        for D in DS:
            info = e.near_merge_umi(None, None, None, 0, D, None, None, None, info_of(8, 0), None)
            assert (info.near.nodes, info.near.merged, info.links, info.near.over_limit_first, info.near.max_group) == (0, 0, 0, ref.NO_RECORD, ref.MAX_GROUP)
            check(e, [(b"A", (template(rng, 50),))], D)
            check(e, [(b"ACGT", (b"",))], D)
            check(e, [(b"ACGT", (b"",)), (b"ACGA", (b"",)), (b"ACGT", (b"",))], D)
            assert check(e, [(b"AC-GT", (template(rng, 40),))] * 300, D).near.nodes == 1
    with Engine(segments=2) as e:
        check(e, [(b"AC", (b"", b""))] * 3 + [(b"AC", (b"A", b"")), (b"AG", (b"A", b""))], 1)


def test_misuse_is_refused():
    rng = random.Random(1500)
    records = [(b"ACGTACGT", (template(rng, 20),)) for _ in range(62)]
    records += [records[3], records[5]]                          # records 62 and 63 are no nodes
    n = len(records)
    segs, alive = placed([m for _, m in records])
    text, id_start, umi_off = id_lines(records, rng)
    owner = dev(ref.exact_owners(records, 0))
    good = info_of(8, 0)
    identity = np.arange(n, dtype=np.uint32)
    out = torch.zeros(n, dtype=torch.int32, device="cuda")

    def link_with(v, to):
        link = identity.copy()
        link[v] = to
        return dev(link)

    def info_with(**fields):
        info = info_of(8, 0)
        for name, value in fields.items():
            setattr(info, name, value)
        return info

    with Engine(segments=1) as e:
        def call(**changed):
            args = dict(segs=segs, owner=owner, link=None, n=n, distance=1, text=text, id_start=id_start, umi_off=umi_off, info=good, owner_out=out)
            args.update(changed)
            return e.near_merge_umi(**args)
        assert call().near.merged == 62
        assert call(link=link_with(63, 40)).links == 0            # a link at a record that is no node is not read
        assert call(link=link_with(40, 7)).links == 1
        e.sync()
        out.zero_()
        bad = [dict(distance=0), dict(distance=4), dict(flags=2), dict(out=None), dict(owner_out=None), dict(owner=None), dict(n=1 << 31),
               dict(info=None), dict(info=info_with(bad_record=0, bad_reason=1)), dict(info=info_with(umi_len=0)), dict(info=info_with(umi_len=65)),     # a refused info
               dict(text=None), dict(id_start=None), dict(umi_off=None),
               dict(link=link_with(7, 40)), dict(link=link_with(0, 1))]      # a link above its record
        for k, changed in enumerate(bad):
            with pytest.raises(FqdError):
                call(**changed)
            assert not out.cpu().numpy().any(), k                # nothing was written
        for changed in (dict(owner_out=owner), dict(owner_out=umi_off), dict(owner_out=id_start.view(torch.int32)[:n]), dict(owner_out=segs[0].lengths)):
            with pytest.raises(FqdError):
                call(**changed)
        link = dev(identity)
        with pytest.raises(FqdError):
            call(link=link, owner_out=link)                      # owner_out overlaps the links
        with pytest.raises(FqdError):
            call(link=identity)                                  # host memory
        with pytest.raises(FqdError):
            call(umi_off=np.zeros(n, np.uint32))
        assert call(distance=3).near.nodes == 62                 # the engine is as good as before
    # a link to a record that is no node
    records = [records[0], records[0], records[1], records[2]]
    segs2, alive2 = placed([m for _, m in records])
    text, id_start, umi_off = id_lines(records, rng)
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    with Engine(segments=1) as e:
        for link, fine in (([0, 0, 2, 3], True), ([0, 1, 0, 3], True), ([0, 0, 1, 3], False), ([0, 0, 2, 1], False)):
            args = (segs2, dev(np.array([0, 0, 2, 3], np.uint32)), dev(np.array(link, np.uint32)), 4, 1, text, id_start, umi_off, good, out)
            if fine:
                e.near_merge_umi(*args)
                e.sync()
                out.zero_()
            else:
                with pytest.raises(FqdError):
                    e.near_merge_umi(*args)
                assert not out.cpu().numpy().any()
    del alive, alive2
