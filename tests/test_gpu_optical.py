"""fqd_read_places and fqd_optical_split (csrc/fqd_optical.hip) through the binding, exactly against the sequential statement
(tests/optical_reference.py): every output array, every field of the two infos, nothing written behind the last entry.
Places: every reason and the lowest refused record; record counts round the tiles (64 lanes, 256 a block, 2048), 0 included;
ID lines of one byte and of several hundred.  Split: the edge list of tests/optical_cases.py; cluster sizes round the
kernels' classes (eight lanes up to 8 members, a wave up to 64, a workgroup up to the block limit, the large tier up to the
cap) with a chain in each, the cap itself and one member more, which is refused with owner_out untouched; a cluster that
straddles a scan tile; a 20 000-record random file.  End to end through the binding, single-end and paired: submit, owners,
group, split, group again give the statement's clusters.  Misuse: each case FQD_ERR_ARG."""
import random

import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, Reads, _lib
from fastq_dupaway_amd._lib import FqdError
import optical_reference as ref
from optical_cases import BIG, SURFACE, chain, cluster_cases, grid, id_line, parse_cases, random_clusters

pytestmark = pytest.mark.gpu
FILL = 0xEE
PAD = 64
GUARD = 8                                                      # entries behind the last one of every output array
SMALL, WAVE, BLOCK = 8, 64, 2048                               # csrc/fqd_optical_core.hpp: kSmall, kWave, kBlockLimit
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]
NONE32 = 0xFFFFFFFF


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


@pytest.fixture(scope="module")
def cap():
    with Engine(segments=1) as e:
        got = e.optical_split(None, None, None, None, None, None, None, None, 0, 1, None)
    assert got.max_cluster >= 65536
    return got.max_cluster


class IdLines:
    """ID lines back to back in device memory, FILL behind the last one."""
    def __init__(self, lines):
        lens = np.array([len(x) for x in lines], np.uint32)
        starts = np.zeros(max(len(lines), 1), np.uint64)
        if len(lines) > 1:
            starts[1:len(lines)] = np.cumsum(lens.astype(np.uint64))[:-1]
        self.n = len(lines)
        self.text = dev(np.concatenate([np.frombuffer(b"".join(lines), np.uint8), np.full(PAD, FILL, np.uint8)]))
        self.start, self.len = dev(starts), dev(lens if len(lines) else np.zeros(1, np.uint32))


def places_on_device(e, lines):
    """fqd_read_places over the lines, asserted against the statement; returns (ids, the four device arrays, surfaces)."""
    n = len(lines)
    ids = IdLines(lines)
    out = [torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda") for _ in range(4)]
    got = e.read_places(ids.text, ids.start, ids.len, n, *out)
    e.sync()
    tile, x, y, word, surfaces, info = ref.read_places(lines)
    assert dict(bad_record=got.bad_record, bad_reason=got.bad_reason, other_surface=got.other_surface) == info
    for t, want in zip(out, (tile, x, y, word)):
        a = host(t, np.uint32)
        assert np.all(a[n:] == NONE32)                         # nothing behind the last entry
        if info["bad_record"] == ref.NO_RECORD:
            bad = np.nonzero(a[:n] != want)[0]
            assert bad.size == 0, (bad[:10], a[bad[:10]], want[bad[:10]], [lines[i] for i in bad[:3]])
    return ids, out, surfaces


def random_lines(rng, n, long_every=0):
    lines = []
    for i in range(n):
        surface = rng.choice([SURFACE] * 6 + [b"M01:7:FC1:2", b"M01:7:FC1:10", b"N02:7:FC1:1"])
        if long_every and i % long_every == 0:
            surface = b"I" * rng.randrange(200, 500) + b":7:FC1:1"
        lines.append(id_line(surface, rng.randrange(1, 3000), rng.randrange(10 ** rng.randrange(1, 10)), rng.randrange(10 ** rng.randrange(1, 10)),
                             rng.choice([b"", b"", b"_ACGTAC", b":ACGT+TT", b"#0/1"]), rng.choice([b" 1:N:0:ACGT", b"", b"\tx", b" " + b"c" * 300])))
    return lines


def test_places_every_reason_and_the_lowest_refused_record():
    cases = parse_cases()
    fine = [line for _, line, reason in cases if reason == ref.OK]
    bad = [(name, line, reason) for name, line, reason in cases if reason != ref.OK]
    assert {reason for _, _, reason in bad} == {1, 2, 3, 4, 5}
    with Engine(segments=1) as e:
        places_on_device(e, fine)
        for k, (name, line, reason) in enumerate(bad):
            later = bad[(k + 1) % len(bad)][1]
            lines = fine * 3 + [line] + fine + [later] * 2 + fine
            ids = IdLines(lines)
            got = e.read_places(ids.text, ids.start, ids.len, len(lines), *[torch.zeros(len(lines), dtype=torch.int32, device="cuda") for _ in range(4)])
            assert (got.bad_record, got.bad_reason) == (3 * len(fine), reason), name
        places_on_device(e, [bad[0][1]] + fine)                # record 0 itself
        places_on_device(e, fine + [bad[3][1]])                # the last record


def test_places_record_counts_round_the_tiles():
    rng = random.Random(41)
    with Engine(segments=1) as e:
        for n in COUNTS:
            places_on_device(e, random_lines(rng, n, long_every=97))


def test_places_lines_of_one_byte_and_of_several_hundred():
    rng = random.Random(42)
    with Engine(segments=1) as e:
        places_on_device(e, random_lines(rng, 300, long_every=2))
        lines = random_lines(rng, 70)
        for at in (69, 64, 5, 0):
            lines[at] = b"@"
            places_on_device(e, lines)                         # (the statement names record `at`, the lowest so far)
        places_on_device(e, [b"@"])
        places_on_device(e, [b"@", b">"] * 40)


def test_places_misuse():
    lines = random_lines(random.Random(43), 10)
    ids = IdLines(lines)
    out = [torch.full((10,), -1, dtype=torch.int32, device="cuda") for _ in range(4)]
    with Engine(segments=1) as e:
        def refused(match, *, text=ids.text, start=ids.start, tile=out[0], surface=out[3], n=10, info=True):
            with pytest.raises(FqdError, match=match) as ei:
                e.read_places(text, start, ids.len, n, tile, out[1], out[2], surface, info=info)
            assert ei.value.code == _lib.ERR_ARG
        refused("device memory", text=ids.text.cpu().numpy())
        refused("device memory", start=ids.start.cpu().numpy())
        refused("device memory", tile=np.zeros(10, np.uint32))
        refused("fqd_read_places", surface=None)
        refused("fqd_read_places", info=None)
        refused("fqd_read_places", n=0xFFFFFFFF)
        e.sync()
        assert all(bool((t == -1).all()) for t in out)


# ---- the split ---------------------------------------------------------------------------------------------------------------

def info_dict(got):
    return {k: getattr(got, k) for k in ("clusters_in", "clusters_out", "split", "largest", "sweeps", "max_cluster", "over_limit_members", "over_limit_first")}


def file_of(clusters, seed=None):
    """clusters = [members, ...] -> (places per record, owner per record): the members of every cluster keep their order, the
    clusters are interleaved at random (seed None: one after another)."""
    tagged = [[(c, m) for m in members] for c, members in enumerate(clusters)]
    if seed is None:
        records = [r for t in tagged for r in t]
    else:
        rng = random.Random(seed)
        left = [list(reversed(t)) for t in tagged]
        alive = [c for c, t in enumerate(left) if t]
        records = []
        while alive:
            k = rng.randrange(len(alive))
            records.append(left[alive[k]].pop())
            if not left[alive[k]]:
                alive[k] = alive[-1]
                alive.pop()
    first = {}
    owner = np.array([first.setdefault(c, i) for i, (c, _) in enumerate(records)], np.uint32)
    return [m for _, m in records], owner


def grouping(owner):
    """What fqd_group_owners leaves: the records ordered by owner, members in input order, and the head flags."""
    perm = np.argsort(owner, kind="stable").astype(np.uint32)
    head = np.ones(len(owner), np.uint8)
    head[1:] = owner[perm[1:]] != owner[perm[:-1]]
    return perm, head


def split_on_device(e, clusters, D, cap, seed=None):
    """fqd_read_places and fqd_optical_split over a file of these clusters, owner_out and the info asserted; returns the
    statement's owner_out (None: refused)."""
    places, owner = file_of(clusters, seed)
    n = len(places)
    ids, arrays, _ = places_on_device(e, [id_line(*p) for p in places])
    exp_owner, exp_info = ref.split(owner, places, D, cap)
    perm, head = grouping(owner)
    inputs = [dev(perm if n else np.zeros(1, np.uint32)), dev(head if n else np.zeros(1, np.uint8))]
    before = [t.clone() for t in inputs + arrays]
    owner_out = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    got = e.optical_split(*inputs, ids.text, ids.start, *arrays, n, D, owner_out)
    e.sync()
    out = host(owner_out, np.uint32)
    assert info_dict(got) == exp_info
    assert np.all(out[n:] == NONE32)                           # nothing behind the last entry
    if exp_owner is None:
        assert np.all(out == NONE32)                           # refused: untouched
    else:
        bad = np.nonzero(out[:n] != exp_owner)[0]
        assert bad.size == 0, (bad[:10], out[bad[:10]], exp_owner[bad[:10]])
    for t, b in zip(inputs + arrays, before):
        assert torch.equal(t, b)
    return exp_owner


def test_split_edge_list(cap):
    cases = cluster_cases()
    with Engine(segments=1) as e:
        for name, D, members in cases:
            split_on_device(e, [members], D, cap)
        for D in sorted({D for _, D, _ in cases}):             # and all clusters of one D in one file, interleaved
            split_on_device(e, [m for _, d, m in cases if d == D], D, cap, seed=D)
        # no record on record 0's surface: the bytes decide every pair
        split_on_device(e, [[(b"X9:1:F:1", 1, 1, 1)]] + [m for _, d, m in cases if d == 50], 50, cap)


def test_split_n_of_zero(cap):
    with Engine(segments=1) as e:
        split_on_device(e, [], 5, cap)


def test_split_sizes_round_the_kernels_classes(cap):
    rng = random.Random(51)
    sizes = [1, 2, SMALL - 1, SMALL, SMALL + 1, WAVE - 1, WAVE, WAVE + 1] * 4 + [1] * 300 + [2] * 40
    clusters = [m for s in sizes for _, _, m in random_clusters(rng.randrange(1 << 30), 1, sizes=(s,))]
    clusters += [chain(s) for s in (SMALL, SMALL + 1, WAVE, WAVE + 1, 200)]
    with Engine(segments=1) as e:
        for D in (1, 10, 300):
            split_on_device(e, clusters, D, cap, seed=D)


@pytest.mark.parametrize("s", [BLOCK, BLOCK + 1])
def test_split_round_the_block_limit(cap, s):
    rng = random.Random(52)
    scattered = [(SURFACE, 5, rng.randrange(4000), rng.randrange(4000)) for _ in range(s)]
    with Engine(segments=1) as e:
        split_on_device(e, [chain(s), [(SURFACE, 3, 7, 7)] * 3, scattered, grid(50, 41, 4)[:s]], 10, cap, seed=s)
        split_on_device(e, [[(SURFACE, 9, 77, 88)] * s, [(SURFACE, 9, 100 * i, 5) for i in range(s)]], 3, cap)      # all identical; none a neighbour


def test_split_a_chain_at_the_cap(cap):
    with Engine(segments=1) as e:
        owner = split_on_device(e, [[(SURFACE, 1, 1, 1)] * 2, chain(cap), chain(BLOCK + 500, reverse=False)], 10, cap)
    assert owner is not None and len(set(owner.tolist())) == 3


def test_split_over_the_cap_is_refused_and_nothing_is_written(cap):
    with Engine(segments=1) as e:
        assert split_on_device(e, [chain(9), chain(cap + 1), chain(70), chain(cap + 40)], 10, cap) is None
        split_on_device(e, [chain(9), chain(70)], 10, cap)     # and the engine goes on


def test_split_a_cluster_that_straddles_a_scan_tile(cap):
    rng = random.Random(53)
    singles = [[(SURFACE, 1, rng.randrange(10 ** 6), rng.randrange(10 ** 6))] for _ in range(2030)]
    with Engine(segments=1) as e:
        owner = split_on_device(e, singles + [chain(40), grid(5, 5, 3)], 10, cap)     # places 2030 .. 2094 of the grouping
    assert set(owner[2030:2070].tolist()) == {2030}


def test_split_more_places_than_the_tile_scans_first_round(cap):
    """The one block that scans the head counts takes 1024 tiles of 2048 places a round: a grouping of 1024 tiles, one tile and
    three places more.  Clusters of one, a chain across the round's edge and a grid at the end; the records share the ID
    lines of one small file, which fqd_read_places has read."""
    tile, n = 2048, 1024 * 2048 + 2048 + 3
    rng = random.Random(56)
    base = chain(30) + grid(4, 4, 3) + [(SURFACE, 1101, rng.randrange(10 ** 6), rng.randrange(10 ** 6)) for _ in range(15)]
    pick = 46 + np.arange(n) % 15
    owner = np.arange(n, dtype=np.uint32)
    edge = 1024 * tile - 20
    pick[edge:edge + 30], owner[edge:edge + 30] = np.arange(30), edge
    pick[n - 16:], owner[n - 16:] = 30 + np.arange(16), n - 16
    with Engine(segments=1) as e:
        ids, arrays, _ = places_on_device(e, [id_line(*p) for p in base])
        at = torch.from_numpy(pick).cuda()
        big = [t[:len(base)][at].contiguous() for t in arrays]
        exp_owner, exp_info = ref.split(owner, [base[p] for p in pick.tolist()], 10, cap)
        perm, head = grouping(owner)
        owner_out = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
        got = e.optical_split(dev(perm), dev(head), ids.text, ids.start[:len(base)][at].contiguous(), *big, n, 10, owner_out)
        e.sync()
    out = host(owner_out, np.uint32)
    assert info_dict(got) == exp_info and exp_info["clusters_in"] == n - 29 - 15 and exp_info["split"] == 0
    assert np.all(out[n:] == NONE32)
    bad = np.nonzero(out[:n] != exp_owner)[0]
    assert bad.size == 0, (bad[:10], out[bad[:10]], exp_owner[bad[:10]])


def test_split_a_random_file_of_20000_records(cap):
    rng = random.Random(54)
    clusters = []
    while sum(len(c) for c in clusters) < 20000:
        s = rng.choice([1] * 16 + [2, 2, 3, 5, 9, 30, 70, 150])
        span = rng.choice([50, 500, 5000])
        clusters.append([(rng.choice([SURFACE] * 9 + [b"M01:7:FC1:2"]), rng.choice([1101, 1101, 1102]), rng.randrange(span), rng.randrange(span)) for _ in range(s)])
    with Engine(segments=1) as e:
        split_on_device(e, clusters, 40, cap, seed=1)
        split_on_device(e, clusters, BIG, cap, seed=2)


class Mate:
    def __init__(self, reads):
        lens = np.array([len(r) for r in reads], np.uint32)
        offs = np.zeros(len(reads), np.uint64)
        offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
        self.bases = dev(np.concatenate([np.frombuffer(b"".join(reads), np.uint8), np.full(PAD, FILL, np.uint8)]))
        self.offs, self.lens = dev(offs), dev(lens)
        self.desc = Reads(self.bases, offsets=self.offs, lengths=self.lens)


@pytest.mark.parametrize("paired", [False, True])
def test_end_to_end_through_the_binding(cap, paired):
    rng = random.Random(55 + paired)
    frags = [(bytes(rng.choice(b"ACGT") for _ in range(rng.choice([20, 21, 50]))), bytes(rng.choice(b"ACGT") for _ in range(30)) if paired else None)
             for _ in range(150)]
    n, D = 2000, 30
    seqs = [rng.choice(frags) for _ in range(n)]
    places = [(SURFACE, rng.choice([1101, 1102]), rng.randrange(200), rng.randrange(200)) for _ in range(n)]
    first = {}
    owner_in = np.array([first.setdefault(s, i) for i, s in enumerate(seqs)], np.uint32)
    exp_owner, exp_info = ref.split(owner_in, places, D, cap)
    assert exp_info["split"] > 50 and exp_info["clusters_out"] < n - 100
    ids = IdLines([id_line(*p) for p in places])
    mates = [Mate([s[m] for s in seqs]) for m in range(2 if paired else 1)]
    u32 = lambda: torch.full((n,), -1, dtype=torch.int32, device="cuda")
    owner, link, perm, owner_out, tile, x, y, surface = (u32() for _ in range(8))
    keep, head = (torch.full((n,), 7, dtype=torch.uint8, device="cuda") for _ in range(2))
    with Engine(segments=len(mates)) as e:
        assert e.read_places(ids.text, ids.start, ids.len, n, tile, x, y, surface).bad_record == ref.NO_RECORD
        e.submit_linked([m.desc for m in mates], n, keep, link, last=True)
        e.sync()
        e.owners(keep, link, n, owner)
        before = e.group_owners(owner, n, perm, head)
        got = e.optical_split(perm, head, ids.text, ids.start, tile, x, y, surface, n, D, owner_out)
        assert info_dict(got) == exp_info and got.clusters_in == before
        clusters = e.group_owners(owner_out, n, perm, head)
        e.owners_to_keep(owner_out, n, keep)
        e.sync()
    assert np.array_equal(host(owner, np.uint32), owner_in)
    assert np.array_equal(host(owner_out, np.uint32), exp_owner)
    assert clusters == exp_info["clusters_out"]
    p, h = host(perm, np.uint32), head.cpu().numpy()
    listing = []
    for k in range(n):
        if h[k]:
            listing.append([])
        listing[-1].append(int(p[k]))
    assert listing == ref.clusters_of(exp_owner)
    assert np.array_equal(keep.cpu().numpy(), (exp_owner == np.arange(n)).astype(np.uint8))


def test_split_misuse_is_refused_before_anything_is_written(cap):
    places, owner = file_of([chain(3), chain(9), chain(70)], seed=4)
    n = len(places)
    perm, head = grouping(owner)
    with Engine(segments=1) as e:
        ids, arrays, _ = places_on_device(e, [id_line(*p) for p in places])
        d_perm, d_head = dev(perm), dev(head)
        owner_out = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")

        def refused(match, *, p=d_perm, h=d_head, text=ids.text, tile=arrays[0], surface=arrays[3], D=10, out=owner_out, count=n, res=True):
            with pytest.raises(FqdError, match=match) as ei:
                e.optical_split(p, h, text, ids.start, tile, arrays[1], arrays[2], surface, count, D, out, out=res)
            assert ei.value.code == _lib.ERR_ARG

        refused("device memory", p=perm)
        refused("device memory", h=head)
        refused("device memory", text=ids.text.cpu().numpy())
        refused("device memory", tile=np.zeros(n, np.uint32))
        refused("device memory", surface=np.zeros(n, np.uint32))
        refused("device memory", out=np.zeros(n, np.uint32))
        refused("distance of 1", D=0)
        refused("distance of 1", D=0x80000000)
        refused("overlaps an input", out=d_perm)
        refused("overlaps an input", out=arrays[1])
        refused("overlaps an input", out=arrays[3][2:])
        refused("2\\^31-1 records", count=1 << 31)
        refused("fqd_optical_split", res=None)
        no_head = head.copy()
        no_head[0] = 0
        refused("head\\[0\\] is not set", h=dev(no_head))
        outside = perm.copy()
        outside[5] = n
        refused("outside 0 .. n-1", p=dev(outside))
        e.sync()
        assert bool((owner_out == -1).all())
        got = e.optical_split(d_perm, d_head, ids.text, ids.start, *arrays, n, 10, owner_out)      # and the engine goes on
        assert (got.clusters_in, got.clusters_out) == (3, 3)
