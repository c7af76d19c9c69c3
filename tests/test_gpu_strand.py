"""fqd_canonical_reads (csrc/fqd_strand.hip) through the binding, byte for byte against the plain-Python statement
(tests/strand_reference.py): the packed buffer, both offset arrays, both length arrays, flipped and its count; nothing
written behind the last byte.  Shapes: the edge list of tests/strand_cases.py; ragged descriptors at every alignment mod
16 with gaps, uniform descriptors with a stride above the length; record counts round the kernel's tiles (64 records a
wave, 256 a block, 2048 a block of the offset scan); 300 000 x 150.  End to end: the canonical descriptors go into
fqd_submit_final and the flags are the first occurrences of the canonical keys.  Misuse: a capacity one byte short, mate-2
arrays on a single-end engine."""
import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, Reads, _lib
from fastq_dupaway_amd._lib import FqdError
import strand_reference as ref
from strand_cases import paired_cases, random_read, single_end_cases

pytestmark = pytest.mark.gpu
FILL = 0xEE
PAD = 64
WAVE_TILE, BLOCK_TILE, SCAN_TILE = 64, 256, 2048              # csrc/fqd_strand.hip: kWaveTile, kTile, kOffTile


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


class Layout:
    """One mate's reads in device memory.  packed: back to back; gaps: read i starts at an offset that is i mod 16, with
    at least one byte of FILL between reads; uniform: reads of ONE length at a stride of length + 7."""
    def __init__(self, reads, kind, pad=PAD):
        n = len(reads)
        lens = np.array([len(r) for r in reads], dtype=np.uint32)
        if kind == "uniform":
            L = int(lens[0]) if n else 0
            assert np.all(lens == L)
            stride = L + 7
            buf = np.full(n * stride + PAD, FILL, np.uint8)
            if n and L:
                buf[:n * stride].reshape(n, stride)[:, :L] = np.frombuffer(b"".join(reads), np.uint8).reshape(n, L)
            self.bases = dev(buf)
            self.desc = Reads(self.bases, uniform_len=L, uniform_stride=stride)
            return
        offs = np.zeros(n, np.uint64)
        at = 0
        for i in range(n):
            if kind == "gaps":
                at += 1 + (i - at - 1) % 16                   # the next offset that is i mod 16, at least one byte on
            offs[i] = at
            at += int(lens[i])
        buf = np.full(at + pad, FILL, np.uint8)
        for i, r in enumerate(reads):
            buf[int(offs[i]):int(offs[i]) + len(r)] = np.frombuffer(r, np.uint8)
        if kind == "gaps" and n:
            assert np.array_equal(offs % 16, np.arange(n, dtype=np.uint64) % 16)
        self.bases, self.offs, self.lens = dev(buf), dev(offs), dev(lens)
        self.desc = Reads(self.bases, offsets=self.offs, lengths=self.lens)


def canonical(mates, kind="packed", engine=None, pad=PAD):
    """Runs fqd_canonical_reads over the mates (lists of bytes) and asserts everything against the statement.  Returns the
    device arrays (out, offs, lens) for a submit."""
    S, n = len(mates), len(mates[0])
    exp_buf, exp_off, exp_len, exp_flip = ref.expected_layout(mates)
    lay = [Layout(m, kind, pad) for m in mates]
    out = torch.full((len(exp_buf) + PAD,), FILL, dtype=torch.uint8, device="cuda")
    offs = [torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda") for _ in range(S)]
    lens = [torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda") for _ in range(S)]
    flipped = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda")
    e = engine or Engine(segments=S)
    try:
        turned = e.canonical_reads([l.desc for l in lay], n, out, offs[0], lens[0], flipped, offs[1] if S == 2 else None,
                                   lens[1] if S == 2 else None, out_capacity=len(exp_buf), count=True)
        e.sync()
    finally:
        if engine is None:
            e.close()
    got = out.cpu().numpy()
    assert got[:len(exp_buf)].tobytes() == exp_buf
    assert np.all(got[len(exp_buf):] == FILL)                  # nothing behind the last byte
    for s in range(S):
        assert np.array_equal(host(offs[s], np.uint64)[:n], exp_off[s])
        assert np.array_equal(host(lens[s], np.uint32)[:n], exp_len[s])
    assert np.array_equal(flipped.cpu().numpy()[:n], exp_flip)
    assert turned == int(exp_flip.sum())
    return out, offs, lens


# ---------------------------------------------------------------- single-end shapes

@pytest.mark.parametrize("kind", ["packed", "gaps"])
def test_single_end_edge_list(kind):
    reads = [s for _, s in single_end_cases()]
    assert {ref.canon_se(s)[1] for s in reads} == {True, False}
    canonical([reads], kind)


@pytest.mark.parametrize("L", [0, 1, 15, 16, 17, 31, 32, 33, 150, 151, 257])
def test_uniform_descriptors_with_a_stride_above_the_length(L):
    rng = np.random.default_rng(L)
    n = 300
    reads = [rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=L).tobytes() for _ in range(n)]
    canonical([reads], "uniform")


@pytest.mark.parametrize("n", [0, 1, WAVE_TILE - 1, WAVE_TILE, WAVE_TILE + 1, BLOCK_TILE - 1, BLOCK_TILE, BLOCK_TILE + 1,
                               SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_record_counts_round_the_tiles(n, paired):
    import random
    rng = random.Random(n)
    lengths = [0, 1, 5, 16, 31, 32, 40, 75, 150]
    mates = [[random_read(rng, rng.choice(lengths)) for _ in range(n)] for _ in range(2 if paired else 1)]
    canonical(mates, "gaps")


def uniform_single_end_reads(n, L, seed):
    """n reads of L bases back to back through fqd_canonical_reads, against the statement by numpy (ref.canon_se_rows)."""
    rng = np.random.default_rng(seed)
    a = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=(n, L), p=[.245, .245, .245, .245, .02])
    a[::7, L // 2:] = ref.rc_rows(a[::7, :L // 2])           # reads that are their own reverse complement among them
    rows, flip = ref.canon_se_rows(a)
    assert 0 < int(flip.sum()) < n
    bases = dev(np.concatenate([a.reshape(-1), np.full(PAD, FILL, np.uint8)]))
    out = torch.full((n * L + PAD,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    ln = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    flipped = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        turned = e.canonical_reads([Reads(bases, uniform_len=L, uniform_stride=L)], n, out, off, ln, flipped, out_capacity=n * L, count=True)
    got = out.cpu().numpy()
    assert np.array_equal(got[:n * L].reshape(n, L), rows)
    assert np.all(got[n * L:] == FILL)
    assert np.array_equal(host(off, np.uint64), np.arange(n, dtype=np.uint64) * np.uint64(L))
    assert np.all(host(ln, np.uint32) == L)
    assert np.array_equal(flipped.cpu().numpy(), flip)
    assert turned == int(flip.sum())


def test_three_hundred_thousand_reads_of_150():
    uniform_single_end_reads(300_000, 150, 5)


def test_more_reads_than_the_tile_scans_first_round():
    # the one block that scans the records' byte counts takes 1024 tiles of SCAN_TILE records a round: one tile and three reads more
    uniform_single_end_reads(1024 * SCAN_TILE + SCAN_TILE + 3, 6, 6)


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("last", [1, 15, 16, 17, 31, 32, 33, 150, 600])
def test_the_last_read_ends_with_its_allocation(paired, last):
    # no byte behind the last read belongs to the caller; 70 records: the last wave's tile holds 6, the rest lie beyond n
    import random
    rng = random.Random(last)
    mates = [[random_read(rng, rng.choice([0, 3, 16, 40, 150])) for _ in range(69)] + [random_read(rng, last)] for _ in range(2 if paired else 1)]
    canonical(mates, "gaps", pad=0)


# ---------------------------------------------------------------- pairs

@pytest.mark.parametrize("kind", ["packed", "gaps"])
def test_paired_edge_list(kind):
    cases = paired_cases()
    a, b = [c[1] for c in cases], [c[2] for c in cases]
    flips = [ref.canon_pe(x, y)[1] for x, y in zip(a, b)]
    assert True in flips and False in flips
    assert any(len(x) != len(y) and f for x, y, f in zip(a, b, flips))       # lengths change places with the bytes
    canonical([a, b], kind)


def test_paired_uniform_descriptors():
    rng = np.random.default_rng(9)
    n = 500
    a = [rng.choice(np.frombuffer(b"ACGT", np.uint8), size=150).tobytes() for _ in range(n)]
    b = [rng.choice(np.frombuffer(b"ACGT", np.uint8), size=100).tobytes() for _ in range(n)]
    b[10:20] = [x[:100] for x in a[10:20]]                    # mate 2 a prefix of mate 1
    canonical([a, b], "uniform")


# ---------------------------------------------------------------- end to end through the binding

def copies(rng, n, turned_share):
    """origin[i] = the fresh record that record i repeats (itself for four in five), turn[i] = it is turned."""
    origin = np.arange(n)
    is_copy = rng.random(n) < 0.2
    is_copy[0] = False
    idx = np.flatnonzero(is_copy)
    origin[idx] = (rng.random(len(idx)) * idx).astype(np.int64)          # an earlier record, a copy itself or not
    for _ in range(64):                                                   # copies of copies: down to the fresh record
        nxt = origin[origin]
        if np.array_equal(nxt, origin):
            break
        origin = nxt
    turn = is_copy & (rng.random(n) < turned_share)
    return origin, turn


def submit_flags(descs, n, S):
    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    with Engine(segments=S) as e:
        e.submit(descs, n, keep=keep, final=True)
        e.sync()
    return keep.cpu().numpy()


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(17)
    n, L = 300_000, 150
    fresh = [rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=(n, L), p=[.245, .245, .245, .245, .02]) for _ in range(2)]
    return n, L, fresh


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("turned_share", [0.5, 0.0], ids=["half the copies turned", "no copy turned"])
def test_flags_of_canonical_reads_are_the_first_occurrences(big, paired, turned_share):
    n, L, fresh = big
    rng = np.random.default_rng(int(paired) * 2 + int(turned_share > 0))
    origin, turn = copies(rng, n, turned_share)
    S = 2 if paired else 1
    if paired:
        a = np.where(turn[:, None], fresh[1][origin], fresh[0][origin])  # a turned pair: the mates change places
        b = np.where(turn[:, None], fresh[0][origin], fresh[1][origin])
        (c0, c1), flip = ref.canon_pe_rows(a, b)
        exp_keep = ref.first_occurrence_rows(c0, c1)
        given = [a, b]
    else:
        a = fresh[0][origin]
        a = np.where(turn[:, None], ref.rc_rows(a), a)
        c0, flip = ref.canon_se_rows(a)
        exp_keep = ref.first_occurrence_rows(c0)
        given = [a]
    assert int((exp_keep == 0).sum()) >= int((origin != np.arange(n)).sum()) > n // 10
    bases = [dev(np.concatenate([x.reshape(-1), np.full(PAD, FILL, np.uint8)])) for x in given]
    descs = [Reads(x, uniform_len=L, uniform_stride=L) for x in bases]
    out = torch.full((S * n * L + PAD,), FILL, dtype=torch.uint8, device="cuda")
    offs = [torch.empty((n,), dtype=torch.int64, device="cuda") for _ in range(S)]
    lens = [torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(S)]
    flipped = torch.empty((n,), dtype=torch.uint8, device="cuda")
    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    with Engine(segments=S) as e:
        e.canonical_reads(descs, n, out, offs[0], lens[0], flipped, offs[1] if paired else None, lens[1] if paired else None,
                          out_capacity=S * n * L)
        e.submit([Reads(out, offsets=offs[s], lengths=lens[s]) for s in range(S)], n, keep=keep, final=True)
        e.sync()
        assert e.stats()["duplicates"] == int((exp_keep == 0).sum())
    assert np.array_equal(flipped.cpu().numpy(), flip)
    assert np.array_equal(keep.cpu().numpy(), exp_keep)
    plain = submit_flags(descs, n, S)
    if turned_share == 0.0:
        assert np.array_equal(plain, exp_keep)                # nothing turned: what a plain submit says
    else:
        assert int(plain.sum()) > int(exp_keep.sum())         # the plain submit keeps the turned copies


# ---------------------------------------------------------------- misuse

@pytest.mark.parametrize("kind", ["packed", "uniform"])
def test_a_capacity_one_byte_short_is_refused_and_nothing_is_written(kind):
    rng = np.random.default_rng(1)
    reads = [rng.choice(np.frombuffer(b"ACGT", np.uint8), size=40).tobytes() for _ in range(100)]
    lay = Layout(reads, kind)
    total = 40 * 100
    out = torch.full((total + PAD,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((100,), -1, dtype=torch.int64, device="cuda")
    ln = torch.full((100,), -1, dtype=torch.int32, device="cuda")
    flipped = torch.full((100,), 9, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        with pytest.raises(FqdError, match="out_capacity") as ei:
            e.canonical_reads([lay.desc], 100, out, off, ln, flipped, out_capacity=total - 1)
        assert ei.value.code == _lib.ERR_ARG
        e.sync()
        assert bool((out == FILL).all()) and bool((off == -1).all()) and bool((ln == -1).all()) and bool((flipped == 9).all())
        e.canonical_reads([lay.desc], 100, out, off, ln, flipped, out_capacity=total)      # the exact size is enough
        e.sync()
    assert out.cpu().numpy()[:total].tobytes() == ref.expected_layout([reads])[0]


def test_a_single_end_engine_given_mate_two_arrays_is_refused():
    reads = [b"ACGTACGTAC"] * 4
    lay = Layout(reads, "packed")
    out = torch.full((40 + PAD,), FILL, dtype=torch.uint8, device="cuda")
    off = [torch.full((4,), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
    ln = [torch.full((4,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    flipped = torch.full((4,), 9, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        with pytest.raises(FqdError, match="single-end") as ei:
            e.canonical_reads([lay.desc], 4, out, off[0], ln[0], flipped, off[1], ln[1])
        assert ei.value.code == _lib.ERR_ARG
    with Engine(segments=2) as e:
        with pytest.raises(FqdError, match="paired") as ei:
            e.canonical_reads([lay.desc, lay.desc], 4, out, off[0], ln[0], flipped)
        assert ei.value.code == _lib.ERR_ARG
    assert bool((out == FILL).all()) and bool((flipped == 9).all())


def test_host_memory_is_refused():
    reads = np.frombuffer(b"ACGTACGTAC" * 4, np.uint8).copy()
    out = torch.full((40 + PAD,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    ln = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    flipped = torch.full((4,), 9, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        with pytest.raises(FqdError, match="device memory") as ei:
            e.canonical_reads([Reads(reads, uniform_len=10, uniform_stride=10)], 4, out, off, ln, flipped)
        assert ei.value.code == _lib.ERR_ARG
    assert bool((out == FILL).all())
