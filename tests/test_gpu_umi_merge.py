"""fqd_umi_merge (csrc/fqd_umi_merge.hip) through the binding, exactly against the sequential statement
(tests/umi_merge_reference.py): owner_out and every field of the info; nothing written behind the last entry.  Shapes: the
edge list of tests/umi_merge_cases.py; sequence groups of 1, 2 and every size round the kernels' classes (eight lanes a
group up to 8 nodes, a wave up to 64, a block up to the limit), the limit itself and one node more, which is refused with
owner_out untouched; record and node counts round the tiles (64 lanes, 256 a block, 2048 a block of the scan), 0 included; a
group that straddles a scan tile; a 20 000-record random file.  End to end through the binding, single-end and paired: the
exact pass, reset, the pass by sequence, the merge and fqd_group_owners give the statement's clusters.  Misuse: host memory,
a distance of 0 or 3, an info that names a refused record, size 0 at an owner — argument checks, each FQD_ERR_ARG."""
import random

import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, Reads, _lib
from fastq_dupaway_amd._lib import FqdError
import umi_merge_reference as ref
import umi_reference as umi
from umi_merge_cases import bases, edge_cases, seqkey

pytestmark = pytest.mark.gpu
FILL = 0xEE
PAD = 64
GUARD = 8                                                      # entries behind the last one of every output array
SMALL, WAVE = 8, 64                                            # csrc/fqd_umi_merge_core.hpp: kSmall, kWave
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


@pytest.fixture(scope="module")
def max_group():
    with Engine(segments=1) as e:
        got = e.umi_merge(None, None, None, _lib.UmiInfo(4, 4, 0, umi.NO_RECORD, 0, 0), None, None, None, 0, 1, None)
    assert got.max_group >= 4096
    return got.max_group


class IdLines:
    """`@r<i>:<field> c` lines back to back in device memory, FILL behind the last one."""
    def __init__(self, fields):
        lines = [b"@r%d:%s c\n" % (i, f) for i, f in enumerate(fields)]
        lens = np.array([len(x) for x in lines], np.uint32)
        starts = np.zeros(max(len(lines), 1), np.uint64)
        if len(lines) > 1:
            starts[1:len(lines)] = np.cumsum(lens.astype(np.uint64))[:-1]
        self.n = len(lines)
        self.text = dev(np.concatenate([np.frombuffer(b"".join(lines), np.uint8), np.full(PAD, FILL, np.uint8)]))
        self.start, self.len = dev(starts), dev(lens if len(lines) else np.zeros(1, np.uint32))


def info_dict(got):
    return {k: getattr(got, k) for k in ("nodes", "groups", "merged", "largest", "sweeps", "max_group", "over_limit_nodes", "over_limit_first")}


def merge_on_device(e, fields, keys, D, max_group):
    """Runs fqd_umi_find and fqd_umi_merge over the statement's owners and sizes and asserts owner_out and the info; returns
    the statement's owner_out (None: refused)."""
    n = len(fields)
    exp_owner, exp_info, owner_exact, owner_seq, size = ref.merge([bases(f) for f in fields], keys, D, max_group)
    ids = IdLines(fields)
    umi_off = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    info = e.umi_find(ids.text, ids.start, ids.len, n, ":", umi_off)
    assert info.bad_record == umi.NO_RECORD
    if n == 0:
        info = _lib.UmiInfo(4, 4, 0, umi.NO_RECORD, 0, 0)
    owner_out = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    inputs = [dev(owner_exact if n else np.zeros(1, np.uint32)), dev(owner_seq if n else np.zeros(1, np.uint32)), dev(size if n else np.zeros(1, np.uint32))]
    before = [t.clone() for t in inputs]
    got = e.umi_merge(ids.text, ids.start, umi_off, info, *inputs, n, D, owner_out)
    e.sync()
    out = host(owner_out, np.uint32)
    if n == 0:
        exp_info.update(largest=0)
    assert info_dict(got) == exp_info
    assert np.all(out[n:] == 0xFFFFFFFF)                       # nothing behind the last entry
    if exp_owner is None:
        assert np.all(out == 0xFFFFFFFF)                       # refused: untouched
    else:
        bad = np.nonzero(out[:n] != exp_owner)[0]
        assert bad.size == 0, (bad[:10], out[bad[:10]], exp_owner[bad[:10]])
    for t, b in zip(inputs, before):
        assert torch.equal(t, b)
    return exp_owner


def case_arrays(records, both=False):
    return [f for f, _ in records], [seqkey(s, both) for _, s in records]


def distinct_umis(rng, m, L, alphabet=b"ACGT"):
    seen, out = set(), []
    while len(out) < m:
        u = bytes(rng.choice(alphabet) for _ in range(L))
        if u not in seen:
            seen.add(u)
            out.append(u)
    return out


def groups_file(rng, sizes, L=7, copies=(1, 1, 1, 2, 5, 12)):
    """One sequence group of m distinct UMIs per entry of `sizes`, every UMI 1 .. 12 times, the records shuffled."""
    fields, keys = [], []
    for g, m in enumerate(sizes):
        for u in distinct_umis(rng, m, L):
            c = rng.choice(copies)
            fields += [u] * c
            keys += [g] * c
    order = list(range(len(fields)))
    rng.shuffle(order)
    return [fields[i] for i in order], [keys[i] for i in order]


def test_edge_list(max_group):
    with Engine(segments=1) as e:
        for name, D, records in edge_cases():
            for both in (False, True):
                merge_on_device(e, *case_arrays(records, both), D, max_group)


def test_group_sizes_round_the_kernels_classes(max_group):
    rng = random.Random(91)
    sizes = [1, 2, SMALL - 1, SMALL, SMALL + 1, WAVE - 1, WAVE, WAVE + 1] * 6 + [1] * 40 + [2] * 40
    fields, keys = groups_file(rng, sizes)
    with Engine(segments=1) as e:
        for D in (1, 2):
            merge_on_device(e, fields, keys, D, max_group)


@pytest.mark.parametrize("m", ["limit - 1", "limit"])
def test_a_group_at_the_limit(max_group, m):
    rng = random.Random(92)
    fields, keys = groups_file(rng, [3, max_group - 1 if m == "limit - 1" else max_group, 70], copies=(1, 1, 1, 2, 5))
    with Engine(segments=1) as e:
        assert merge_on_device(e, fields, keys, 1, max_group) is not None


def test_a_group_over_the_limit_is_refused_and_nothing_is_written(max_group):
    rng = random.Random(93)
    fields, keys = groups_file(rng, [5, max_group + 1, 9, max_group + 40], copies=(1, 1, 2))
    with Engine(segments=1) as e:
        assert merge_on_device(e, fields, keys, 1, max_group) is None
        merge_on_device(e, *groups_file(rng, [5, 9, 70]), 1, max_group)       # and the engine goes on


@pytest.mark.parametrize("distinct", [False, True])
def test_record_and_node_counts_round_the_tiles(max_group, distinct):
    rng = random.Random(94)
    with Engine(segments=1) as e:
        for n in COUNTS:
            if distinct:                                        # every record a node of its own: n nodes, groups of 30 that straddle every tile
                pool = distinct_umis(rng, 30, 4, b"ACG")
                fields, keys = [pool[i % 30] for i in range(n)], [i // 30 for i in range(n)]
            else:
                fields = [bytes(rng.choice(b"ACG") for _ in range(4)) for _ in range(n)]
                keys = [rng.randrange(1 + n // 20) for _ in range(n)]
            merge_on_device(e, fields, keys, 1 + n % 2, max_group)


def test_a_group_that_straddles_a_scan_tile(max_group):
    # the records of one group lie round record 2048, its nodes round node 2048 of the compacted and of the sorted order
    rng = random.Random(95)
    nodes = [u + b"AAAA" for u in distinct_umis(rng, 20, 4, b"ACG")]
    fields = distinct_umis(rng, 2040, 8) + nodes + nodes[:10] + nodes[:5] * 3          # counts 5, 2 and 1
    keys = list(range(2040)) + ["g"] * 45
    with Engine(segments=1) as e:
        owner = merge_on_device(e, fields, keys, 1, max_group)
    assert len(set(owner[2040:])) < 20 and all(int(o) >= 2040 for o in owner[2040:])


def test_more_records_than_the_tile_scans_first_round(max_group):
    """The one block that scans the node counts takes 1024 tiles of 2048 records a round: 1024 tiles, one tile and three
    records more.  Most records repeat the UMI of their sequence group of 700, so that the statement has few nodes to walk; the
    groups round the round's edge and the last one hold eight UMIs each, one and two bases apart."""
    n = 1024 * 2048 + 2048 + 3
    umis = [b"AAAA", b"AAAC", b"AACC", b"ACCC", b"CCCC", b"GGGG", b"GGGT", b"TTTT"]
    fields, keys = [b"AAAA"] * n, [i // 700 for i in range(n)]
    for g in (1024 * 2048 // 700 - 1, 1024 * 2048 // 700, 1024 * 2048 // 700 + 1, (n - 1) // 700):
        for i in range(g * 700, min(n, g * 700 + 700)):
            fields[i] = umis[(i * 7 // 50) % 8 if i % 3 else 0]
    with Engine(segments=1) as e:
        owner = merge_on_device(e, fields, keys, 1, max_group)
    assert owner is not None and len(set(owner[1024 * 2048 - 700:1024 * 2048 + 700].tolist())) > 4


def test_a_random_file_of_20000_records(max_group):
    rng = random.Random(97)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(10)) for _ in range(900)]
    fields, keys = [], []
    for _ in range(20000):
        fields.append(bytes(rng.choice(b"ACGTN" if rng.random() < 0.1 else b"ACG") for _ in range(6)))
        keys.append(rng.choice(seqs) if rng.random() < 0.9 else seqs[0])
    with Engine(segments=1) as e:
        merge_on_device(e, fields, keys, 1, max_group)
        merge_on_device(e, fields, keys, 2, max_group)


class Mate:
    def __init__(self, reads):
        lens = np.array([len(r) for r in reads], np.uint32)
        offs = np.zeros(len(reads), np.uint64)
        offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
        self.bases = dev(np.concatenate([np.frombuffer(b"".join(reads), np.uint8), np.full(PAD, FILL, np.uint8)]))
        self.offs, self.lens = dev(offs), dev(lens)
        self.desc = Reads(self.bases, offsets=self.offs, lengths=self.lens)


@pytest.mark.parametrize("paired", [False, True])
def test_end_to_end_through_the_binding(max_group, paired):
    rng = random.Random(98 + paired)
    frags = [(bytes(rng.choice(b"ACGT") for _ in range(rng.choice([20, 21, 50]))), bytes(rng.choice(b"ACGT") for _ in range(30)) if paired else None)
             for _ in range(60)]
    if paired:
        frags += [(a, bytes(rng.choice(b"ACGT") for _ in range(30))) for a, _ in frags[:20]]      # the same mate 1 under another mate 2
    n = 5000
    fields = [bytes(rng.choice(b"ACG") for _ in range(3)) + b"+" + bytes(rng.choice(b"ACGN") for _ in range(2)) for _ in range(n)]
    seqs = [rng.choice(frags) for _ in range(n)]
    exp_owner, exp_info, *_ = ref.merge([bases(f) for f in fields], seqs, 1, max_group)
    assert exp_info["merged"] > 100 and exp_info["groups"] > 50
    ids = IdLines(fields)
    mates = [Mate([s[m] for s in seqs]) for m in range(2 if paired else 1)]
    u32 = lambda: torch.full((n,), -1, dtype=torch.int32, device="cuda")
    umi_off, owner_exact, owner_seq, size, link, perm, owner_out = (u32() for _ in range(7))
    keep, head = (torch.full((n,), 7, dtype=torch.uint8, device="cuda") for _ in range(2))
    total = sum(len(bases(f)) + len(s[0]) for f, s in zip(fields, seqs))
    out = torch.full((total + PAD,), FILL, dtype=torch.uint8, device="cuda")
    off, ln = torch.full((n,), -1, dtype=torch.int64, device="cuda"), u32()
    with Engine(segments=len(mates)) as e:
        info = e.umi_find(ids.text, ids.start, ids.len, n, ":", umi_off)
        e.umi_reads(ids.text, ids.start, umi_off, info, mates[0].desc, n, out, off, ln, out_capacity=total)
        e.submit_linked([Reads(out, offsets=off, lengths=ln)] + [m.desc for m in mates[1:]], n, keep, link, last=True)
        e.sync()
        e.owners(keep, link, n, owner_exact)
        exact = e.group_owners(owner_exact, n, perm, head)
        e.cluster_sizes(perm, head, n, size, levels=False)
        e.reset()
        e.submit_linked([m.desc for m in mates], n, keep, link, last=True)
        e.sync()
        e.owners(keep, link, n, owner_seq)
        got = e.umi_merge(ids.text, ids.start, umi_off, info, owner_exact, owner_seq, size, n, 1, owner_out)
        assert info_dict(got) == exp_info and got.nodes == exact
        clusters = e.group_owners(owner_out, n, perm, head)
        e.owners_to_keep(owner_out, n, keep)
        e.sync()
    assert np.array_equal(host(owner_out, np.uint32), exp_owner)
    assert clusters == exp_info["nodes"] - exp_info["merged"]
    p, h = host(perm, np.uint32), head.cpu().numpy()
    listing = []
    for k in range(n):
        if h[k]:
            listing.append([])
        listing[-1].append(int(p[k]))
    assert listing == ref.clusters_of(exp_owner)
    assert np.array_equal(keep.cpu().numpy(), (exp_owner == np.arange(n)).astype(np.uint8))


def test_misuse_is_refused_before_anything_is_written(max_group):
    rng = random.Random(99)
    fields, keys = groups_file(rng, [1, 2, 9, 70])
    n = len(fields)
    _, _, owner_exact, owner_seq, size = ref.merge(fields, keys, 1, max_group)
    ids = IdLines(fields)
    umi_off = torch.zeros(n, dtype=torch.int32, device="cuda")
    owner_out = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    d_exact, d_seq, d_size = dev(owner_exact), dev(owner_seq), dev(size)
    with Engine(segments=1) as e:
        info = e.umi_find(ids.text, ids.start, ids.len, n, ":", umi_off)

        def refused(match, *, text=ids.text, exact=d_exact, seq=d_seq, sz=d_size, D=1, out=owner_out, info=info, res=True):
            with pytest.raises(FqdError, match=match) as ei:
                e.umi_merge(text, ids.start, umi_off, info, exact, seq, sz, n, D, out, out=res)
            assert ei.value.code == _lib.ERR_ARG

        refused("device memory", text=ids.text.cpu().numpy())
        refused("device memory", exact=owner_exact)
        refused("device memory", seq=owner_seq)
        refused("device memory", sz=size)
        refused("device memory", out=np.zeros(n, np.uint32))
        refused("distance of 1 or 2", D=0)
        refused("distance of 1 or 2", D=3)
        refused("fqd_umi_merge", res=None)
        refused("fqd_umi_merge", info=None)
        for change in (dict(bad_record=3, bad_reason=umi.SHAPE_DIFFERS), dict(n_bases=5), dict(umi_len=65), dict(umi_len=0, n_bases=0)):
            wrong = _lib.UmiInfo(info.n_bases, info.umi_len, info.joiners, info.bad_record, info.bad_reason, 0)
            for k, v in change.items():
                setattr(wrong, k, v)
            refused("fqd_umi_find leaves", info=wrong)
        owner_at = int(np.nonzero(owner_exact == np.arange(n))[0][5])
        no_size = size.copy()
        no_size[owner_at] = 0
        refused("size 0", sz=dev(no_size))
        behind = owner_exact.copy()
        behind[3] = n - 1
        refused("behind its record", exact=dev(behind))
        e.sync()
        assert bool((owner_out == -1).all())
        got = e.umi_merge(ids.text, ids.start, umi_off, info, d_exact, d_seq, d_size, n, 1, owner_out)      # and the engine goes on
        assert got.nodes == int((owner_exact == np.arange(n)).sum())
