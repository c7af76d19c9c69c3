"""GPU checks of FQD_FAST_KEEP / FQD_FAST_CLUSTERS' primitives (fqd_submit_linked in csrc/fqd_engine.hip; fqd_owners,
fqd_group_owners, fqd_heads_to_keep in csrc/fqd_owner.hip) through ctypes, against a dict of first indices.

Every case asserts: keep equals a plain fqd_submit run's and the dict's; every cleared flag's link names an EARLIER
record of the IDENTICAL key and kept records' entries are untouched; the owners are the first index of every key; the
order groups the records by owner (exactly: clusters by first member, members in input order, one head per cluster).
Cases: uniform 150 bp and ragged 1-200 bp, pairs whose mate 1 is equal and mate 2 differs, 1/63/64/65/20 000 records,
three unequal batches with duplicates across them, both insert paths, the weak hash, a heavy bucket, the final batch
declared or not; the pick on hand-made scores (ties, a maximum that stands last, saturated scores); bad arguments."""
import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, Reads, _lib
from fastq_dupaway_amd._lib import FqdError
import fast_keep_reference as fast

pytestmark = pytest.mark.gpu
UNWRITTEN = 0xFFFFFFFF


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


class Mate:
    """One mate's reads on the device: uniform (no offsets) when all lengths are equal, ragged otherwise."""
    def __init__(self, reads):
        lens = np.array([len(r) for r in reads], dtype=np.uint32)
        self.uniform = int(lens[0]) if len(set(lens.tolist())) == 1 and lens[0] > 0 else None
        offs = np.zeros(len(reads), np.uint64)
        offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        self.bases = dev(np.frombuffer(b"".join(reads) + b"\0" * 64, dtype=np.uint8).copy())
        self.offs, self.lens = dev(offs), dev(lens)

    def batch(self, a):
        if self.uniform is not None:
            return Reads(self.bases[a * self.uniform:], uniform_len=self.uniform, uniform_stride=self.uniform)
        return Reads(self.bases, offsets=self.offs[a:], lengths=self.lens[a:])


def first_index(keys):
    seen = {}
    return np.array([seen.setdefault(k, i) for i, k in enumerate(keys)], dtype=np.uint32)


def check_run(mates, cuts, weak_hash=False, declare_last=True, profile=False):
    """mates: per mate the list of reads (bytes); cuts: batch boundaries [0, ..., n].  Returns (owner, perm, head) on the
    device and the engine they came from is closed; everything listed in the module's docstring is asserted here."""
    S, n = len(mates), len(mates[0])
    keys = list(zip(*mates))
    first = first_index(keys)
    exp_keep = (first == np.arange(n)).astype(np.uint8)
    m = [Mate(r) for r in mates]

    plain = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    with Engine(segments=S, weak_hash=weak_hash) as e:
        for a, b in zip(cuts[:-1], cuts[1:]):
            e.submit([x.batch(a) for x in m], b - a, keep=plain[a:])
        e.sync()
        plain_dups = e.stats()["duplicates"]

    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    link = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    owner = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    perm = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    head = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    with Engine(segments=S, weak_hash=weak_hash, profile=profile) as e:
        for a, b in zip(cuts[:-1], cuts[1:]):
            e.submit_linked([x.batch(a) for x in m], b - a, keep[a:], link[a:], last=declare_last and b == n)
        e.sync()
        assert e.stats()["duplicates"] == plain_dups == n - int(exp_keep.sum())
        prof = e.profile() if profile else None
        e.owners(keep, link, n, owner)                       # after the final batch: nothing here uses the table
        clusters = e.group_owners(owner, n, perm, head)
    got_keep, got_link = keep.cpu().numpy(), host_u32(link)
    assert np.array_equal(got_keep, plain.cpu().numpy())
    assert np.array_equal(got_keep, exp_keep)
    dup = np.flatnonzero(got_keep == 0)
    assert np.all(got_link[got_keep == 1] == UNWRITTEN)      # entries of kept records are not written
    assert np.all(got_link[dup] < dup)                       # earlier ...
    assert all(keys[int(got_link[i])] == keys[int(i)] for i in dup)   # ... and the identical key
    assert np.array_equal(host_u32(owner), first)
    got_perm, got_head = host_u32(perm), head.cpu().numpy()
    assert np.array_equal(np.sort(got_perm), np.arange(n, dtype=np.uint32))            # a permutation
    exp_perm = np.argsort(first, kind="stable").astype(np.uint32)                       # ascending owners, members in input order
    assert np.array_equal(got_perm, exp_perm)
    exp_head = np.ones(n, np.uint8)
    exp_head[1:] = first[exp_perm[1:]] != first[exp_perm[:-1]]
    assert np.array_equal(got_head, exp_head)
    assert clusters == len(set(keys)) == int(exp_head.sum())
    return keys, first, prof


def reads_uniform(rng, n, L=150, dup=0.2):
    pool = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=(max(1, int(n * (1 - dup))), L), p=[.245, .245, .245, .245, .02])
    pick = rng.integers(0, len(pool), n)
    return [pool[k].tobytes() for k in pick]


def reads_ragged(rng, n, dup=0.2):
    pool = [rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=int(rng.integers(1, 201))).tobytes() for _ in range(max(1, int(n * (1 - dup))))]
    return [pool[k] for k in rng.integers(0, len(pool), n)]


@pytest.mark.parametrize("bulk_min", ["0", "-1"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 20_000])
@pytest.mark.parametrize("shape", ["uniform", "ragged"])
def test_single_end(monkeypatch, shape, n, bulk_min):
    monkeypatch.setenv("FQD_BULK_MIN", bulk_min)
    rng = np.random.default_rng(n + (shape == "ragged"))
    reads = reads_uniform(rng, n) if shape == "uniform" else reads_ragged(rng, n)
    check_run([reads], [0, n])


@pytest.mark.parametrize("bulk_min", ["0", "-1"])
@pytest.mark.parametrize("n", [65, 20_000])
def test_pairs_whose_mate_1_is_equal_and_mate_2_differs(monkeypatch, n, bulk_min):
    monkeypatch.setenv("FQD_BULK_MIN", bulk_min)
    rng = np.random.default_rng(3)
    one = reads_uniform(rng, n, L=100, dup=0.9)              # few distinct mates 1 ...
    two = reads_uniform(rng, n, L=75, dup=0.9)               # ... under a few distinct mates 2: equal pairs and half-equal ones
    assert len(set(one)) < len(set(zip(one, two))) < n       # equal mates 1 under different mates 2, and equal pairs
    check_run([one, two], [0, n])


@pytest.mark.parametrize("declare_last", [True, False])
@pytest.mark.parametrize("bulk_min", ["0", "-1"])
@pytest.mark.parametrize("shape", ["uniform", "ragged"])
def test_three_unequal_batches_with_duplicates_across_them(monkeypatch, shape, bulk_min, declare_last):
    monkeypatch.setenv("FQD_BULK_MIN", bulk_min)
    rng = np.random.default_rng(5)
    n = 20_000
    reads = reads_uniform(rng, n, dup=0.5) if shape == "uniform" else reads_ragged(rng, n, dup=0.5)
    check_run([reads], [0, 11_000, 11_065, n], declare_last=declare_last)


@pytest.mark.parametrize("bulk_min", ["0", "-1"])
def test_weak_hash_unequal_keys_share_slots(monkeypatch, bulk_min):
    monkeypatch.setenv("FQD_BULK_MIN", bulk_min)
    rng = np.random.default_rng(6)
    n = 20_000
    check_run([reads_uniform(rng, n, L=75, dup=0.3)], [0, 9_000, n], weak_hash=True)


def test_heavy_bucket_path(monkeypatch):
    # one key about 20 000 times among 40 000 records: its bucket (segments of 4096 slots) goes to heavy_bucket_insert_kernel
    monkeypatch.setenv("FQD_BULK_MIN", "0")
    monkeypatch.setenv("FQD_SEG_BITS", "12")
    monkeypatch.setenv("FQD_HEAVY_ABOVE", "8000")
    rng = np.random.default_rng(7)
    n = 40_000
    reads = reads_uniform(rng, n, L=60, dup=0.0)
    hot = reads[17]
    for i in np.flatnonzero(rng.random(n) < 0.5):
        if i > 17:
            reads[int(i)] = hot
    # That heavy_bucket_insert_kernel takes them: equal keys have equal hashes, so all copies of `hot` land in ONE bucket
    # whatever the table's geometry; about 20 000 (12 500 in the first batch of the second run) is above FQD_HEAVY_ABOVE,
    # so bucket_dedup_kernel skips that bucket and lists it for the heavy kernel — the only other way its records are
    # inserted on the bulk path.  That the bulk path ran is asserted from the profile (the dedup bracket is its alone).
    assert sum(r == hot for r in reads) > 16_000
    for cuts in ([0, n], [0, 25_000, n]):
        assert sum(r == hot for r in reads[:cuts[1]]) > 8000
        _, _, prof = check_run([reads], cuts, profile=True)
        assert prof["dedup_launches"] >= 1 and prof["partition_launches"] >= 1


# ---------------------------------------------------------------- the pick on top of the grouping

@pytest.mark.parametrize("case", ["ties", "maximum last", "saturated", "random"])
def test_heads_to_keep_after_the_pick(case):
    rng = np.random.default_rng(8)
    n = 5000
    keys = rng.integers(0, 1200, n).tolist()
    first = first_index(keys)
    if case == "ties":
        scores = rng.integers(0, 3, n).astype(np.uint32)
    elif case == "maximum last":
        scores = np.arange(n, dtype=np.uint32)               # the best member of every cluster is its last
    elif case == "saturated":
        scores = rng.choice(np.array([2 ** 32 - 1, 2 ** 32 - 2, 0], dtype=np.uint32), n)
    else:
        scores = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    head = torch.empty(n, dtype=torch.uint8, device="cuda")
    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        clusters = e.group_owners(dev(first), n, perm, head)
        before = host_u32(perm).tolist()
        moved = e.seq_pick_best(dev(scores), head, n, perm)
        e.heads_to_keep(perm, head, n, keep)
    exp_perm, exp_moved = fast.restate_pick(before, head.cpu().numpy().tolist(), scores.tolist())
    assert host_u32(perm).tolist() == exp_perm and moved == exp_moved
    assert moved > 0
    groups = fast.clusters_of(keys)
    assert clusters == len(groups)
    exp_keep = np.zeros(n, np.uint8)
    for g in groups:
        exp_keep[fast.pick(g, scores.tolist())] = 1
    assert np.array_equal(keep.cpu().numpy(), exp_keep)


# ---------------------------------------------------------------- arguments

def test_bad_arguments_are_refused():
    d8 = torch.zeros(8, dtype=torch.uint8, device="cuda")
    d32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    h8, h32 = np.zeros(8, np.uint8), np.zeros(8, np.uint32)
    bases = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        with pytest.raises(FqdError, match="fqd_submit_linked") as ei:
            e.submit_linked([Reads(bases, uniform_len=4, uniform_stride=4)], 8, d8, d32, memory=_lib.MEM_HOST)
        assert ei.value.code == _lib.ERR_ARG
        with pytest.raises(FqdError, match="fqd_submit_linked"):
            e.submit_linked([Reads(bases, uniform_len=4, uniform_stride=4)], 8, d8, None)
        for args in ((h8, d32, 8, d32), (d8, h32, 8, d32), (d8, d32, 8, h32)):
            with pytest.raises(FqdError, match="fqd_owners") as ei:
                e.owners(*args)
            assert ei.value.code == _lib.ERR_ARG
        for args in ((h32, 8, d32, d8), (d32, 8, h32, d8), (d32, 8, d32, h8)):
            with pytest.raises(FqdError, match="fqd_group_owners") as ei:
                e.group_owners(*args)
            assert ei.value.code == _lib.ERR_ARG
        for n in (2 ** 31, 2 ** 32 + 5):                     # the argument alone: nothing is allocated or launched
            with pytest.raises(FqdError, match="fqd_group_owners") as ei:
                e.group_owners(d32, n, d32, d8)
            assert ei.value.code == _lib.ERR_ARG
        for args in ((h32, d8, 8, d8), (d32, h8, 8, d8), (d32, d8, 8, h8)):
            with pytest.raises(FqdError, match="fqd_heads_to_keep") as ei:
                e.heads_to_keep(*args)
            assert ei.value.code == _lib.ERR_ARG
        assert e.group_owners(d32, 0, d32, d8) == 0
