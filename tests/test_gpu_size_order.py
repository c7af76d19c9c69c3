"""GPU checks of FQD_FAST_SORT=size / FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE's primitives (fqd_size_filter, fqd_size_order,
fqd_size_order_ex, fqd_take_u32 in csrc/fqd_size_order.hip) through ctypes, against the plain-Python statement (tests/size_order_reference.py).

fqd_size_order: W and n around the wave and block sizes, the compaction's tile (2048 places) and the radix pass's tile (4096
entries); all sizes equal, all distinct, sizes at both sides of 255 / 256, every cluster above 255, exactly one above 255, the
largest at tier 2's pass edges; ties over a tile edge, tiles without a kept head, kept and unkept heads alternating, nothing
kept, an order that a restated pick has taken out of ascending order; entries behind the W written ones and guard entries
behind the array stay as they were; misuse is refused with nothing written.  fqd_size_filter: counts and flags at both sides
of both bounds, through the 16-byte path and the byte path.  fqd_take_u32 at the same n.  End to end: the chain from
fqd_submit_linked to fqd_copy_labelled through the order gives the statement's output text."""
import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, Reads, _lib
from fastq_dupaway_amd._lib import FqdError
import fast_keep_reference as fast
import size_order_reference as ref

pytestmark = pytest.mark.gpu
GUARD = 7
FILL32 = 0x5A5A5A5A
FILL8 = 0xEE
PLACE_TILE = 2048                                            # places a block of the compaction (csrc/fqd_record_scan.hpp, kOffTile)
SORT_TILE = 4096                                             # entries a block of a radix pass (csrc/fqd_join.hip, kSortTile)
NS = [0, 1, 63, 64, 65, 255, 256, 257, PLACE_TILE - 1, PLACE_TILE, PLACE_TILE + 1, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE + 1]


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def guarded_u32(n):
    return torch.full((n + GUARD,), FILL32, dtype=torch.int32, device="cuda")


@pytest.fixture(scope="module")
def e():
    with Engine(segments=1) as engine:
        yield engine


def grouping(rng, runs, shuffled=True):
    """(perm, head, size, keep) of clusters with the given member counts, in that order: the flags of fqd_group_owners'
    grouping, every written record kept."""
    runs = np.asarray(runs, np.int64)
    n = int(runs.sum())
    perm = (rng.permutation(n) if shuffled else np.arange(n)).astype(np.uint32)
    starts = np.concatenate([[0], np.cumsum(runs)[:-1]]).astype(np.int64) if len(runs) else np.zeros(0, np.int64)
    head = np.zeros(n, np.uint8)
    head[starts] = 1
    size = np.zeros(n, np.uint32)
    size[perm[starts]] = runs
    keep = np.zeros(n, np.uint8)
    keep[perm[starts]] = 1
    return perm, head, size, keep


def expected_order(perm, head, size, keep):
    """The statement by numpy for the large cases: the kept head places in place order, a STABLE sort by size descending."""
    places = np.flatnonzero(head)
    ok = perm[places] < len(perm)
    places = places[ok]
    places = places[keep[perm[places]] != 0]
    recs = perm[places]
    return recs[np.argsort(-size[recs].astype(np.int64), kind="stable")].tolist()


def check_order(e, perm, head, size, keep):
    n = len(perm)
    expect = expected_order(perm, head, size, keep)
    if n <= 20000:
        assert expect == ref.written_order(perm.tolist(), head.tolist(), size.tolist(), keep.tolist())
    order = guarded_u32(n)
    args = [dev(perm), dev(head), dev(size), dev(keep)]
    torch.cuda.synchronize()
    w, info = e.size_order_info(*args, n, order)
    got = host_u32(order)
    assert w == len(expect)
    # what the call says it counted and launched: W, the L pairs of tier 2, the largest size, tier 2's passes
    sizes = size[np.asarray(expect, np.int64)] if expect else np.zeros(0, np.uint32)
    large, largest = int((sizes > 255).sum()), int(sizes.max()) if expect else 0
    passes = ((largest - 256).bit_length() + 7) // 8 if large > 1 else 0
    assert (info.written, info.large, info.largest, info.tier2_passes) == (w, large, largest, passes)
    assert got[:w].tolist() == expect
    assert np.all(got[w:] == FILL32)                         # entries at W and beyond, and the guard behind the n, are untouched
    return expect


# ---------------------------------------------------------------- fqd_size_order

@pytest.mark.parametrize("n", NS)
def test_equal_sizes_keep_the_place_order(e, n):
    rng = np.random.default_rng(n)
    if n == 0:
        assert e.size_order(None, None, None, None, 0, None) == 0
        return
    perm, head, size, keep = grouping(rng, [1] * n)          # W = n singletons under a shuffled perm
    assert check_order(e, perm, head, size, keep) == perm.tolist()
    perm, head, size, keep = grouping(rng, [3] * n)          # W = n clusters of three: the heads every third place
    assert check_order(e, perm, head, size, keep) == perm[::3].tolist()
    perm, head, size, keep = grouping(rng, [300] * min(n, 65))      # ties in bucket 0, over the compaction's tile edges
    assert check_order(e, perm, head, size, keep) == perm[::300].tolist()


@pytest.mark.parametrize("w", NS[1:])
def test_w_at_the_edges_with_kept_and_unkept_heads_alternating(e, w):
    rng = np.random.default_rng(100 + w)
    runs = rng.choice([1, 1, 2, 5, 255, 256], 2 * w)
    perm, head, size, keep = grouping(rng, runs)
    starts = np.flatnonzero(head)
    keep[perm[starts[1::2]]] = 0                              # every second cluster is not written
    assert len(check_order(e, perm, head, size, keep)) == w


@pytest.mark.parametrize("w", [1, 63, 64, 65, 255, 256, 257, 600])
def test_all_sizes_distinct(e, w):
    rng = np.random.default_rng(200 + w)
    runs = rng.permutation(np.arange(1, w + 1))
    perm, head, size, keep = grouping(rng, runs)
    got = check_order(e, perm, head, size, keep)
    assert size[got].tolist() == list(range(w, 0, -1))


@pytest.mark.parametrize("pool,count", [([254, 255, 256, 257, 258], 60), (list(range(256, 400)), 40), ([256], 9), ([1, 2, 3, 255], 500)],
                         ids=["straddling", "all-above-255", "all-256", "none-above-255"])
def test_sizes_around_255(e, pool, count):
    rng = np.random.default_rng(len(pool) + count)
    runs = rng.choice(pool, count)
    perm, head, size, keep = grouping(rng, runs)
    got = check_order(e, perm, head, size, keep)
    assert sorted(size[got].tolist(), reverse=True) == size[got].tolist() and len(got) == count


@pytest.mark.parametrize("big", [256, 257, 300, 5000])
def test_exactly_one_cluster_above_255(e, big):
    rng = np.random.default_rng(big)
    runs = rng.choice([1, 1, 1, 2, 7, 255], 700)
    runs[rng.integers(0, 700)] = big
    perm, head, size, keep = grouping(rng, runs)
    got = check_order(e, perm, head, size, keep)
    assert size[got[0]] == big and size[got[1]] <= 255


@pytest.mark.parametrize("largest", [65535, 65536, 65537, 65791, 65792])
def test_the_largest_at_tier_twos_pass_edges(e, largest):
    """largest - 256 = 65535 takes two passes, 65536 three (65791 / 65792); 65535 .. 65537 stand around the 16-bit size."""
    rng = np.random.default_rng(largest)
    runs = np.array([1] * 40 + [2] * 10 + [256, 256, 300, 300, 300, 511, 512, 513, 40000, 40000, 65535 if largest > 65535 else 65000, largest])
    rng.shuffle(runs)
    perm, head, size, keep = grouping(rng, runs)
    assert 180_000 <= len(perm) <= 260_000
    got = check_order(e, perm, head, size, keep)
    assert size[got[0]] == largest and size[got].tolist() == sorted(runs.tolist(), reverse=True)
    order = guarded_u32(len(perm))
    args = [dev(perm), dev(head), dev(size), dev(keep)]
    torch.cuda.synchronize()
    w, info = e.size_order_info(*args, len(perm), order)
    assert info.large == 12 and info.tier2_passes == (2 if largest <= 65791 else 3)      # twelve pairs alone went through tier 2
    assert e.size_order(*args, len(perm), order) == w                                    # the plain entry is the same call


def test_tiles_without_a_kept_head(e):
    rng = np.random.default_rng(5)
    long_run = 3 * PLACE_TILE + 5                             # one head, then whole tiles without any
    runs = [1] * 100 + [long_run] + [2] * 50 + [1] * (2 * PLACE_TILE + 3) + [4] * 10
    perm, head, size, keep = grouping(rng, runs)
    assert any(not head[t * PLACE_TILE:(t + 1) * PLACE_TILE].any() for t in range(len(head) // PLACE_TILE))
    got = check_order(e, perm, head, size, keep)
    assert size[got[0]] == long_run
    starts = np.flatnonzero(head)
    unkept = starts[(starts >= 4 * PLACE_TILE) & (starts < 6 * PLACE_TILE)]      # heads, none of them kept, over a whole tile
    keep[perm[unkept]] = 0
    assert len(unkept) >= PLACE_TILE
    check_order(e, perm, head, size, keep)
    keep[perm[starts[:-1]]] = 0                               # the last head alone
    keep[perm[starts[-1]]] = 1
    assert check_order(e, perm, head, size, keep) == [int(perm[starts[-1]])]


def test_more_places_than_the_tile_scans_first_round(e):
    """The one block that scans the tile counts takes 1024 tiles a round: 1024 tiles of places, one tile and three places more."""
    n = 1024 * PLACE_TILE + PLACE_TILE + 3
    rng = np.random.default_rng(7)
    runs = rng.choice([1, 2, 3], n)
    runs = runs[:int(np.searchsorted(np.cumsum(runs), n))]    # the longest prefix below n places, and one cluster for the rest
    runs = np.append(runs, n - runs.sum())
    perm, head, size, keep = grouping(rng, runs)
    assert len(perm) == n and head[1024 * PLACE_TILE:].sum() > PLACE_TILE // 3
    assert len(check_order(e, perm, head, size, keep)) == len(runs)


def test_nothing_kept_leaves_the_order_untouched(e):
    rng = np.random.default_rng(6)
    perm, head, size, keep = grouping(rng, rng.choice([1, 2, 300], 500))
    assert check_order(e, perm, head, size, np.zeros_like(keep)) == []


def test_an_order_that_is_not_ascending_after_a_restated_pick(e):
    rng = np.random.default_rng(7)
    n = 5000
    keys = rng.integers(0, 900, n).tolist()
    keys[::7] = [0] * len(keys[::7])                          # one cluster above 255
    seen = {}
    first = np.array([seen.setdefault(k, i) for i, k in enumerate(keys)], dtype=np.uint32)
    scores = rng.integers(0, 50, n).tolist()
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    head = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_first = dev(first)
    torch.cuda.synchronize()
    e.group_owners(d_first, n, perm, head)
    h = head.cpu().numpy()
    picked, moved = fast.restate_pick(host_u32(perm).tolist(), h.tolist(), scores)
    assert moved > 0 and picked != sorted(picked)
    picked = np.array(picked, np.uint32)
    starts = np.flatnonzero(h)
    size, keep = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    size[picked[starts]] = np.diff(np.append(starts, n))
    keep[picked[starts]] = 1
    got = check_order(e, picked, h, size, keep)
    groups = fast.clusters_of(keys)                           # by first member: the tie rule speaks of the FIRST member's place
    want = [fast.pick(g, scores) for g in sorted(groups, key=lambda g: (-len(g), g[0]))]
    assert got == want and size[got[0]] > 255


def test_misuse_is_refused_and_nothing_is_written(e):
    rng = np.random.default_rng(8)
    perm, head, size, keep = grouping(rng, rng.choice([1, 2, 300], 300))
    n = len(perm)
    order = guarded_u32(n)
    d = [dev(perm), dev(head), dev(size), dev(keep)]
    bad_head = head.copy(); bad_head[0] = 0
    d_bad_head = dev(bad_head)
    no_size = size.copy(); no_size[perm[np.flatnonzero(head)[5]]] = 0
    d_no_size = dev(no_size)
    torch.cuda.synchronize()
    with pytest.raises(FqdError, match="fqd_size_order.*head\\[0\\]") as ei:
        e.size_order(d[0], d_bad_head, d[2], d[3], n, order)
    assert ei.value.code == _lib.ERR_ARG
    with pytest.raises(FqdError, match="fqd_size_order.*size 0") as ei:      # a kept place without a size
        e.size_order(d[0], d[1], d_no_size, d[3], n, order)
    assert ei.value.code == _lib.ERR_ARG
    for big in (2 ** 31, 2 ** 32 + 5):                       # the argument alone: nothing is allocated or launched
        with pytest.raises(FqdError, match="fqd_size_order") as ei:
            e.size_order(*d, big, order)
        assert ei.value.code == _lib.ERR_ARG
    for args in ((perm, d[1], d[2], d[3], n, order), (d[0], head, d[2], d[3], n, order), (d[0], d[1], d[2], d[3], n, np.zeros(n, np.uint32)),
                 (d[0], d[1], None, d[3], n, order), (d[0], d[1], d[2], d[3], n, None)):
        with pytest.raises(FqdError, match="fqd_size_order") as ei:
            e.size_order(*args)
        assert ei.value.code == _lib.ERR_ARG
    e.sync()
    assert np.all(host_u32(order) == FILL32)                 # none of the refusals wrote to order


def test_an_order_that_is_no_permutation_stays_inside(e):
    """W <= the head places <= n whatever perm holds, and a perm entry outside 0 .. n-1 is no kept place: read the bounds in
    csrc/fqd_size_order_core.hpp.  The statement is applied to the same arrays."""
    n = 3000
    rng = np.random.default_rng(9)
    head = (rng.random(n) < 0.5).astype(np.uint8); head[0] = 1
    size = rng.choice([1, 2, 3, 300], n).astype(np.uint32)
    keep = (rng.random(n) < 0.7).astype(np.uint8)
    same = np.full(n, 17, np.uint32)                          # every place names record 17
    keep[17] = 1
    assert check_order(e, same, head, size, keep) == [17] * int(head.sum())
    outside = rng.integers(0, n, n).astype(np.uint32)         # repeats, and entries at n and far beyond it
    outside[::5] = n
    outside[1::5] = 0xFFFFFFFF
    got = check_order(e, outside, head, size, keep)
    assert 0 < len(got) < int(head.sum()) and max(got) < n


# ---------------------------------------------------------------- fqd_size_filter

def check_filter(e, size, keep, lo, hi, offset=0):
    """offset: the arrays start that many entries into their allocations (1: neither 16-byte nor 4-byte aligned)."""
    n = len(size)
    d_size = torch.full((offset + n + GUARD,), FILL32, dtype=torch.int32, device="cuda")
    d_keep = torch.full((offset + n + GUARD,), FILL8, dtype=torch.uint8, device="cuda")
    d_size[offset:offset + n] = dev(size)
    d_keep[offset:offset + n] = dev(keep)
    torch.cuda.synchronize()
    clusters, records = e.size_filter(d_size[offset:], n, lo, hi, d_keep[offset:])
    want, want_clusters, want_records = ref.filtered(size.tolist(), keep.tolist(), lo, hi)
    got = d_keep.cpu().numpy()
    assert (clusters, records) == (want_clusters, want_records)
    assert got[offset:offset + n].tolist() == want
    assert np.all(got[:offset] == FILL8) and np.all(got[offset + n:] == FILL8)
    assert host_u32(d_size)[offset:offset + n].tolist() == size.tolist()      # the sizes are read only
    return clusters, records


@pytest.mark.parametrize("n", NS[1:])
def test_the_filter_at_both_sides_of_both_bounds(e, n):
    rng = np.random.default_rng(300 + n)
    keep = (rng.random(n) < 0.6).astype(np.uint8)
    size = rng.choice([1, 2, 3, 4, 5, 6, 255, 256, 257, 2 ** 31 - 1], n).astype(np.uint32)
    size[(keep == 0) & (rng.random(n) < 0.7)] = 0             # a record that is not written carries no size
    for lo, hi in ((1, 0), (2, 0), (1, 1), (3, 5), (4, 4), (256, 256), (257, 0), (2 ** 31 - 1, 0), (1, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        check_filter(e, size, keep, lo, hi, offset=(lo + hi + n) % 2)
    assert check_filter(e, size, keep, 1, 0) == (0, 0)         # today's run: no flag changes


def test_the_filter_refuses_misuse(e):
    n = 1000
    rng = np.random.default_rng(10)
    keep = np.ones(n, np.uint8)
    size = rng.choice([1, 2, 3], n).astype(np.uint32)
    d_size, d_keep = dev(size), dev(keep)
    torch.cuda.synchronize()
    for lo, hi in ((0, 0), (2, 1), (2 ** 31, 0), (1, 2 ** 31), (5, 4)):
        with pytest.raises(FqdError, match="fqd_size_filter") as ei:
            e.size_filter(d_size, n, lo, hi, d_keep)
        assert ei.value.code == _lib.ERR_ARG
    for args in ((size, n, 1, 0, d_keep), (d_size, n, 1, 0, keep), (None, n, 1, 0, d_keep), (d_size, 2 ** 31, 1, 0, d_keep)):
        with pytest.raises(FqdError, match="fqd_size_filter") as ei:
            e.size_filter(*args)
        assert ei.value.code == _lib.ERR_ARG
    e.sync()
    assert d_keep.cpu().numpy().tolist() == keep.tolist()    # none of the refusals touched a flag
    for at in (0, 63, 64, n - 1):                            # flags and sizes that do not belong together, wherever
        wrong = size.copy(); wrong[at] = 0
        d_wrong, d_flags = dev(wrong), dev(keep)
        torch.cuda.synchronize()
        with pytest.raises(FqdError, match="fqd_size_filter.*size 0") as ei:
            e.size_filter(d_wrong, n, 1, 0, d_flags)
        assert ei.value.code == _lib.ERR_ARG
    assert e.size_filter(None, 0, 1, 0, None) == (0, 0)


# ---------------------------------------------------------------- fqd_take_u32

@pytest.mark.parametrize("n", NS)
def test_take_u32(e, n):
    rng = np.random.default_rng(400 + n)
    m = max(1, 3 * n)
    values = rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32)
    if n == 0:
        e.take_u32(None, None, 0, None)
        return
    idx = rng.integers(0, m, n).astype(np.uint32)
    idx[0], idx[-1] = m - 1, 0
    out = guarded_u32(n)
    d_values, d_idx = dev(values), dev(idx)
    torch.cuda.synchronize()
    e.take_u32(d_values, d_idx, n, out)
    e.sync()
    got = host_u32(out)
    assert got[:n].tolist() == values[idx].tolist() and np.all(got[n:] == FILL32)
    with pytest.raises(FqdError, match="fqd_take_u32") as ei:
        e.take_u32(values, d_idx, n, out)
    assert ei.value.code == _lib.ERR_ARG


# ---------------------------------------------------------------- the chain

def test_end_to_end_through_the_binding(e):
    rng = np.random.default_rng(11)
    n = 5000
    pool = ["".join(rng.choice(list("ACGT"), int(rng.integers(30, 80)))) for _ in range(1500)]
    seqs = [pool[int(k)] for k in rng.integers(0, len(pool), n)]
    for i in rng.choice(n, 600, replace=False):              # clusters above 255 members
        seqs[int(i)] = pool[int(i) % 2]
    recs, start, id_len, seq_off, seq_len, rec_size, at = [], [], [], [], [], [], 0
    for i, s in enumerate(seqs):
        line = f"@read{i}" + ("" if i % 5 == 0 else f"{' ' if i % 2 else chr(9)}{i % 3 + 1}:N:0:ATCACG") + "\n"
        r = f"{line}{s}\n+\n{'I' * len(s)}\n".encode()
        start.append(at); id_len.append(len(line)); seq_off.append(at + len(line)); seq_len.append(len(s)); rec_size.append(len(r))
        recs.append(r); at += len(r)
    text = b"".join(recs)
    lo, hi = 2, 400
    exp_out, gone, gone_records, written = ref.dedup_ordered([text], by_size=True, lo=lo, hi=hi, sizeout=True)
    assert gone > 100 and written[0] > 255 and len(set(written)) < len(written) and 1 not in written
    d_text = dev(np.frombuffer(text, np.uint8))
    d_start, d_idl, d_size = dev(np.array(start, np.uint64)), dev(np.array(id_len, np.uint32)), dev(np.array(rec_size, np.uint32))
    d_soff, d_slen = dev(np.array(seq_off, np.uint64)), dev(np.array(seq_len, np.uint32))
    keep = torch.zeros(n, dtype=torch.uint8, device="cuda")
    link, owner, perm, size, label_at, out_size, order = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(7))
    head = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with Engine(segments=1) as own:                          # (an engine of its own: this one takes reads)
        own.submit_linked([Reads(d_text, offsets=d_soff, lengths=d_slen)], n, keep, link, last=True)
        own.sync()
        own.owners(keep, link, n, owner)
        clusters = own.group_owners(owner, n, perm, head)
        own.cluster_sizes(perm, head, n, size)
        assert own.size_filter(size, n, lo, hi, keep) == (gone, gone_records)
        w = own.size_order(perm, head, size, keep, n, order)
        assert w == clusters - gone == len(written)
        own.size_labels(d_text, d_start, d_idl, d_size, keep, size, n, label_at, out_size)
        ones = torch.ones(w, dtype=torch.uint8, device="cuda")
        lens, at_w, size_w = (torch.zeros(w, dtype=torch.int32, device="cuda") for _ in range(3))
        src_off, dst_off = (torch.zeros(w + 1, dtype=torch.int64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        out_bytes = own.output_plan(ones, order, w, d_start, out_size, src_off, lens, dst_off)
        assert out_bytes == len(exp_out[0])
        own.take_u32(label_at, order, w, at_w)
        own.take_u32(size, order, w, size_w)
        dst = torch.full((out_bytes + 64,), FILL8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        own.copy_labelled(d_text, src_off, lens, at_w, size_w, w, dst, dst_off)
        own.sync()
    got = dst.cpu().numpy().tobytes()
    assert got[:out_bytes] == exp_out[0] and got[out_bytes:] == bytes([FILL8]) * 64
    assert host_u32(size_w).tolist() == written
