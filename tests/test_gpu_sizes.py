"""GPU checks of FQD_FAST_SIZEOUT / FQD_FAST_LEVELS' primitives (fqd_cluster_sizes, fqd_size_labels, fqd_copy_labelled in
csrc/fqd_size.hip) through ctypes, against the plain-Python statement (tests/size_reference.py).

fqd_cluster_sizes: the sizes and the level table at n around the wave, block and tile sizes, for singletons, one run of n,
runs that begin on a tile's last and first place, a run over tiles without a head, every level edge, and an order that a
restated pick has taken out of ascending order; guard entries behind every output stay as they were; misuse is refused.
fqd_size_labels: ID lines of 1 .. 600 bytes at every start modulo 16, the word's end at the chunk and round edges and by each
of the four end bytes.  fqd_copy_labelled: byte for byte around part lengths 1, 15, 16, 17, with spans that are not written
in between, through a window, with the fill before and behind the destination unchanged and the source ending with its
allocation.  End to end: the chain from fqd_submit_linked to fqd_copy_labelled gives the statement's output text."""
import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, Reads, _lib
from fastq_dupaway_amd._lib import FqdError
import fast_keep_reference as fast
import size_reference as ref

pytestmark = pytest.mark.gpu
GUARD = 7
FILL32 = 0x5A5A5A5A
FILL8 = 0xEE
TILE = 2048


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


def split_guard(t, n):
    got = host_u32(t)
    assert np.all(got[n:] == FILL32)                         # nothing behind the n entries was touched
    return got[:n]


# ---------------------------------------------------------------- fqd_cluster_sizes

def check_sizes(e, perm, head, levels=True):
    perm, head = np.asarray(perm, np.uint32), np.asarray(head, np.uint8)
    n = len(perm)
    size = guarded_u32(n)
    got = e.cluster_sizes(dev(perm), dev(head), n, size, levels)
    sizes = split_guard(size, n)
    expect = ref.sizes_from(perm.tolist(), head.tolist())
    assert sizes.tolist() == expect                          # (the fill is no size: every entry was written)
    if levels:
        clusters, records, largest = ref.levels_of(expect)
        assert list(got.clusters) == clusters and list(got.records) == records and got.largest == largest and got.reserved == 0
        assert sum(records) == n and sum(clusters) == int(head.sum())
    else:
        assert got is None
    return sizes


NS = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]


@pytest.mark.parametrize("n", NS)
def test_sizes_at_the_wave_block_and_tile_edges(n):
    rng = np.random.default_rng(n)
    ident = np.arange(n, dtype=np.uint32)
    shuffled = rng.permutation(n).astype(np.uint32)
    with Engine(segments=1) as e:
        if n == 0:
            got = e.cluster_sizes(None, None, 0, None)
            assert list(got.clusters) == [0] * 16 and list(got.records) == [0] * 16 and got.largest == 0
            assert e.cluster_sizes(None, None, 0, None, levels=False) is None
            return
        check_sizes(e, ident, np.ones(n, np.uint8))                                   # all singletons
        check_sizes(e, shuffled, np.ones(n, np.uint8))
        one = np.zeros(n, np.uint8); one[0] = 1
        check_sizes(e, ident, one)                                                    # one run of n
        check_sizes(e, shuffled, one, levels=False)
        for p in (0.5, 0.1, 0.01):
            head = (rng.random(n) < p).astype(np.uint8); head[0] = 1
            check_sizes(e, shuffled, head)
        last = np.zeros(n, np.uint8); last[0] = 1; last[n - 1] = 1                    # a singleton on the last place
        check_sizes(e, shuffled, last)


def test_runs_that_begin_on_a_tiles_last_place_and_on_its_first():
    n = 3 * TILE + 10
    rng = np.random.default_rng(1)
    perm = rng.permutation(n).astype(np.uint32)
    with Engine(segments=1) as e:
        for places in ([TILE - 1], [TILE], [TILE - 1, TILE], [TILE - 1, 2 * TILE], [TILE, 2 * TILE - 1, 3 * TILE], [3 * TILE - 1, 3 * TILE, n - 1]):
            head = np.zeros(n, np.uint8); head[0] = 1; head[places] = 1
            check_sizes(e, perm, head)


def test_a_run_over_tiles_without_a_head_between_singletons():
    run = 3 * TILE + 5                                       # 6149
    for front in (100, TILE - 1, TILE):
        head = np.concatenate([np.ones(front, np.uint8), [1], np.zeros(run - 1, np.uint8), np.ones(100, np.uint8)])
        n = len(head)
        assert any(not head[t * TILE:(t + 1) * TILE].any() for t in range(n // TILE))      # a whole tile without a head
        perm = np.random.default_rng(front).permutation(n).astype(np.uint32)
        with Engine(segments=1) as e:
            sizes = check_sizes(e, perm, head)
        assert sizes[perm[front]] == run


def test_every_level_edge_and_the_largest():
    cluster = [9, 10, 49, 50, 99, 100, 499, 500, 999, 1000, 4999, 5000, 9999, 10000]
    rng = np.random.default_rng(2)
    runs = cluster + [1] * 700 + [2] * 20 + [8] * 3
    rng.shuffle(runs)
    head = np.concatenate([[1] + [0] * (r - 1) for r in runs]).astype(np.uint8)
    n = len(head)
    assert 34_000 <= n <= 35_000
    with Engine(segments=1) as e:
        sizes = check_sizes(e, rng.permutation(n).astype(np.uint32), head)
    clusters, records, largest = ref.levels_of(sizes.tolist())
    assert largest == 10000 and clusters[9:] == [2, 2, 2, 2, 2, 2, 1] and clusters[8] == 1 and records[15] == 10000


def test_an_order_that_is_not_ascending_after_a_restated_pick():
    rng = np.random.default_rng(3)
    n = 5000
    keys = rng.integers(0, 1200, n).tolist()
    seen = {}
    first = np.array([seen.setdefault(k, i) for i, k in enumerate(keys)], dtype=np.uint32)
    scores = rng.integers(0, 50, n).tolist()
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    head = torch.empty(n, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        e.group_owners(dev(first), n, perm, head)
        h = head.cpu().numpy()
        picked, moved = fast.restate_pick(host_u32(perm).tolist(), h.tolist(), scores)
        assert moved > 0 and picked != sorted(picked)
        sizes = check_sizes(e, picked, h)
    groups = fast.clusters_of(keys)
    for g in groups:                                         # the size stands at the member that is written
        w = fast.pick(g, scores)
        assert sizes[w] == len(g) and all(sizes[i] == 0 for i in g if i != w)


def test_misuse_is_refused():
    n = 300
    perm = dev(np.arange(n, dtype=np.uint32))
    head = np.ones(n, np.uint8); head[0] = 0
    size = guarded_u32(n)
    h32, h8 = np.zeros(n, np.uint32), np.ones(n, np.uint8)
    with Engine(segments=1) as e:
        with pytest.raises(FqdError, match="fqd_cluster_sizes.*head\\[0\\]") as ei:
            e.cluster_sizes(perm, dev(head), n, size)
        assert ei.value.code == _lib.ERR_ARG
        e.sync()
        assert np.all(host_u32(size) == FILL32)              # nothing was written to size
        for big in (2 ** 31, 2 ** 32 + 5):                   # the argument alone: nothing is allocated or launched
            with pytest.raises(FqdError, match="fqd_cluster_sizes") as ei:
                e.cluster_sizes(perm, dev(h8), big, size)
            assert ei.value.code == _lib.ERR_ARG
        for args in ((h32, dev(h8), n, size), (perm, h8, n, size), (perm, dev(h8), n, h32), (None, dev(h8), n, size)):
            with pytest.raises(FqdError, match="fqd_cluster_sizes") as ei:
                e.cluster_sizes(*args)
            assert ei.value.code == _lib.ERR_ARG
        assert np.all(host_u32(size) == FILL32)
        assert e.cluster_sizes(perm, dev(h8), n, size, levels=False) is None      # levels = NULL is accepted
        assert split_guard(size, n).tolist() == [1] * n


# ---------------------------------------------------------------- fqd_size_labels

ENDS = b" \t\r\n"


def id_lines():
    """ID lines of 1 .. 600 bytes: the first word's end at the chunk (16) and round (256) edges, by each end byte, at the
    line's own newline, and nowhere."""
    rng = np.random.default_rng(4)
    alphabet = np.frombuffer(b"abcXYZ:;=_0189/#", np.uint8)

    def filler(k):
        return rng.choice(alphabet, k).tobytes()

    lines = []
    for L in range(1, 601):
        if L == 1:
            lines.append(b"@")
            continue
        want = [15, 16, 17, 255, 256, 257, L - 1, 1, int(rng.integers(1, L))][L % 9]
        p = min(want, L - 1)
        end = bytes([ENDS[L % 4]]) if p < L - 1 else b"\n"
        line = b"@" + filler(p - 1) + end
        if len(line) < L:
            line += filler(L - len(line) - 1).replace(b"#", b" ") + b"\n"          # blanks in the comment as well
        assert len(line) == L
        lines.append(line)
    for L in (2, 5, 15, 16, 17, 40, 256, 257, 300):           # no word end at all: the lengths say where the line ends
        lines.append(b">" + filler(L - 1))
    return lines


def layout(lines, bodies):
    """Records (line + body) at starts that are i mod 16; returns (text bytes, start, id_len, rec_size)."""
    text = bytearray()
    start = []
    for i, (line, body) in enumerate(zip(lines, bodies)):
        while len(text) % 16 != i % 16:
            text += b"\n"                                    # (a word end in front of a record's '@': position 0 is not looked at)
        start.append(len(text))
        text += line + body
    return bytes(text), np.array(start, np.uint64), np.array([len(x) for x in lines], np.uint32), \
        np.array([len(a) + len(b) for a, b in zip(lines, bodies)], np.uint32)


def test_label_places_and_grown_sizes():
    rng = np.random.default_rng(5)
    lines = id_lines()
    n = len(lines)
    bodies = [b"ACGT\n+\nIIII\n" if i % 3 else b"" for i in range(n)]
    text, start, id_len, rec_size = layout(lines, bodies)
    assert sorted(set((start % 16).tolist())) == list(range(16))
    keep = (rng.random(n) < 0.6).astype(np.uint8)
    size = np.array([10 ** int(rng.integers(0, 10)) + int(rng.integers(0, 9)) for _ in range(n)], np.uint32)      # 1 .. 10 digits
    size[-1] = 4294967295
    size[(keep == 0) & (rng.random(n) < 0.5)] = 0            # a record that is not written carries no size
    assert {len(str(s)) for s in size[keep == 1].tolist()} == set(range(1, 11))
    label_at, out_size = guarded_u32(n), guarded_u32(n)
    with Engine(segments=1) as e:
        e.size_labels(dev(np.frombuffer(text, np.uint8)), dev(start), dev(id_len), dev(rec_size), dev(keep), dev(size), n, label_at, out_size)
        got_at, got_size = split_guard(label_at, n), split_guard(out_size, n)
        assert got_at.tolist() == [ref.first_word_end(x) for x in lines]
        assert got_size.tolist() == [int(rec_size[i]) + (len(ref.label(int(size[i]))) if keep[i] else 0) for i in range(n)]
        # a kept record whose size is 0 is refused, wherever it stands
        for at in (0, 63, 64, n - 1):
            bad_keep, bad_size = keep.copy(), size.copy()
            bad_keep[at], bad_size[at] = 1, 0
            with pytest.raises(FqdError, match="fqd_size_labels.*size 0") as ei:
                e.size_labels(dev(np.frombuffer(text, np.uint8)), dev(start), dev(id_len), dev(rec_size), dev(bad_keep), dev(bad_size), n, label_at, out_size)
            assert ei.value.code == _lib.ERR_ARG
        with pytest.raises(FqdError, match="fqd_size_labels") as ei:      # a host pointer
            e.size_labels(dev(np.frombuffer(text, np.uint8)), start, dev(id_len), dev(rec_size), dev(keep), dev(size), n, label_at, out_size)
        assert ei.value.code == _lib.ERR_ARG
        e.size_labels(None, None, None, None, None, None, 0, None, None)              # no record: nothing to do


# ---------------------------------------------------------------- fqd_copy_labelled

PAD = 64


def spans():
    """[(record bytes or None for a span that is not written, label_at, size)]."""
    rng = np.random.default_rng(6)
    out, digit = [], 0

    def rec(k):
        return rng.integers(33, 127, k, dtype=np.uint8).tobytes()

    def next_size():
        nonlocal digit
        digit = digit % 10 + 1
        return 4294967295 if digit == 10 else 10 ** (digit - 1) + int(rng.integers(0, 9 * 10 ** (digit - 1)))

    for at, tail in ((1, 1), (1, 4), (2, 3), (3, 12), (14, 1), (1, 14), (7, 8)):      # whole records shorter than sixteen bytes
        out.append((rec(at + tail), at, next_size()))
    out.append((None, 5, 77))
    for at in (1, 15, 16, 17, 33):
        for tail in (1, 15, 16, 17, 300):
            out.append((rec(at + tail), at, next_size()))
            if (at + tail) % 2:
                out.append((None, 0, 0))                      # spans that are not written in between
    for at, tail in ((128, 128), (129, 127), (300, 1), (40, 0), (5, 0)):              # the label as the record's last bytes
        out.append((rec(at + tail), at, next_size()))
    out.append((rec(16 + 300), 16, 123))                     # the last source byte ends with its allocation
    return out


def span_arrays(sp):
    src = b"".join(r for r, _, _ in sp if r is not None)
    src_off, lens, label_at, size, parts, at = [], [], [], [], [], 0
    for r, a, s in sp:
        src_off.append(at if r is not None else len(src) - 1)
        label_at.append(a); size.append(s)
        if r is None:
            lens.append(0); parts.append(b"")
            continue
        parts.append(r[:a] + ref.label(s) + r[a:])
        lens.append(len(parts[-1]))
        at += len(r)
    lens = np.array(lens, np.uint32)
    dst_off = np.zeros(len(sp), np.uint64)
    dst_off[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
    return src, np.array(src_off, np.uint64), lens, np.array(label_at, np.uint32), np.array(size, np.uint32), dst_off, parts


def test_the_labelled_copy_byte_for_byte():
    sp = spans()
    src, src_off, lens, label_at, size, dst_off, parts = span_arrays(sp)
    expect = b"".join(parts)
    n = len(sp)
    d_src = dev(np.frombuffer(src, np.uint8))                # exactly as long as the records
    dst = torch.full((PAD + len(expect) + PAD,), FILL8, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        e.copy_labelled(d_src, dev(src_off), dev(lens), dev(label_at), dev(size), n, dst.data_ptr() + PAD, dev(dst_off))
        e.sync()
        got = dst.cpu().numpy().tobytes()
        assert got[PAD:PAD + len(expect)] == expect
        assert got[:PAD] == bytes([FILL8]) * PAD and got[PAD + len(expect):] == bytes([FILL8]) * PAD
        e.copy_labelled(None, None, None, None, None, 0, None, None)
        with pytest.raises(FqdError, match="fqd_copy_labelled") as ei:
            e.copy_labelled(d_src, dev(src_off), dev(lens), None, dev(size), n, dst.data_ptr() + PAD, dev(dst_off))
        assert ei.value.code == _lib.ERR_ARG


@pytest.mark.parametrize("a,b", [(0, 9), (9, 21), (21, None), (8, 9)])
def test_a_window_with_advanced_pointers(a, b):
    sp = spans()
    src, src_off, lens, label_at, size, dst_off, parts = span_arrays(sp)
    b = len(sp) if b is None else b
    lo = int(dst_off[a])
    want = b"".join(parts[a:b])
    win = torch.full((PAD + len(want) + PAD,), FILL8, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        e.copy_labelled(dev(np.frombuffer(src, np.uint8)), dev(src_off)[a:], dev(lens)[a:], dev(label_at)[a:], dev(size)[a:], b - a,
                        win.data_ptr() + PAD - lo, dev(dst_off)[a:])
        e.sync()
    got = win.cpu().numpy().tobytes()
    assert got[PAD:PAD + len(want)] == want
    assert got[:PAD] == bytes([FILL8]) * PAD and got[PAD + len(want):] == bytes([FILL8]) * PAD


# ---------------------------------------------------------------- the chain

def test_end_to_end_through_the_binding():
    rng = np.random.default_rng(7)
    n = 5000
    pool = ["".join(rng.choice(list("ACGT"), int(rng.integers(30, 80)))) for _ in range(1900)]
    seqs = [pool[int(k)] for k in rng.integers(0, len(pool), n)]
    for i in rng.choice(n, 2300, replace=False):             # one cluster of more than 2048 members
        seqs[int(i)] = pool[0]
    recs, start, id_len, seq_off, seq_len, rec_size, at = [], [], [], [], [], [], 0
    for i, s in enumerate(seqs):
        line = f"@read{i}" + ("" if i % 5 == 0 else f"{' ' if i % 2 else chr(9)}{i % 3 + 1}:N:0:ATCACG") + "\n"
        r = f"{line}{s}\n+\n{'I' * len(s)}\n".encode()
        start.append(at); id_len.append(len(line)); seq_off.append(at + len(line)); seq_len.append(len(s)); rec_size.append(len(r))
        recs.append(r); at += len(r)
    text = b"".join(recs)
    exp_out, exp_levels, total, dups, plain, _ = ref.dedup_sized([text])
    assert total == n and n // 4 < dups and max(ref.levels_of([seqs.count(pool[0])])[2], 0) > 2048
    d_text = dev(np.frombuffer(text, np.uint8))
    d_start, d_idl, d_size = dev(np.array(start, np.uint64)), dev(np.array(id_len, np.uint32)), dev(np.array(rec_size, np.uint32))
    d_soff, d_slen = dev(np.array(seq_off, np.uint64)), dev(np.array(seq_len, np.uint32))
    keep = torch.zeros(n, dtype=torch.uint8, device="cuda")
    link, owner, perm, size, label_at, out_size, lens = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(7))
    head = torch.zeros(n, dtype=torch.uint8, device="cuda")
    src_off, dst_off = (torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    with Engine(segments=1) as e:
        e.submit_linked([Reads(d_text, offsets=d_soff, lengths=d_slen)], n, keep, link, last=True)
        e.sync()
        e.owners(keep, link, n, owner)
        clusters = e.group_owners(owner, n, perm, head)
        levels = e.cluster_sizes(perm, head, n, size)
        e.size_labels(d_text, d_start, d_idl, d_size, keep, size, n, label_at, out_size)
        out_bytes = e.output_plan(keep, None, n, d_start, out_size, src_off, lens, dst_off)
        assert out_bytes == len(exp_out[0])                  # out_size sums to the output's size
        dst = torch.full((out_bytes + PAD,), FILL8, dtype=torch.uint8, device="cuda")
        e.copy_labelled(d_text, src_off, lens, label_at, size, n, dst, dst_off)
        e.sync()
    got = dst.cpu().numpy().tobytes()
    assert got[:out_bytes] == exp_out[0] and got[out_bytes:] == bytes([FILL8]) * PAD
    assert clusters == n - dups == sum(levels.clusters) and sum(levels.records) == n
    assert ref.duplevels_text([s for s in host_u32(size).tolist() if s]) == exp_levels
    assert levels.largest > 2048
