"""fqd_umi_find and fqd_umi_reads (csrc/fqd_umi.hip) through the binding, byte for byte against the plain-Python statement
(tests/umi_reference.py): umi_off, info, the packed buffer, its offsets and lengths; nothing written behind the last byte or
the last entry.  Shapes: the edge list of tests/umi_cases.py (ID lines of 0 .. 600 and more bytes, the word's end round the
16-byte chunk and the 256-byte round, every way to be refused, files that differ from record 0's shape); record counts
round the kernels' tiles (64 records a wave, 256 a block, 2048 a block of the offset scan); UMIs of 1 .. 64 bases with and
without joiners; sequences ragged at every offset mod 16 and uniform with a stride above the length; the last ID line and
the last read ending with their allocations.  End to end: the packed descriptors go into fqd_submit_final (single-end and
paired, mate 2 untouched) and the flags are the first occurrences of (UMI bases, sequences).  Misuse: a capacity one byte
short, host memory, a null info, an info that names a refused record."""
import random

import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, Reads, _lib
from fastq_dupaway_amd._lib import FqdError
import umi_reference as ref
from umi_cases import COLON, UNDERSCORE, id_line, random_umi, refused_cases, shape_files, taken_cases

pytestmark = pytest.mark.gpu
FILL = 0xEE
PAD = 64
GUARD = 8                                                      # entries behind the last one of every output array
WAVE_TILE, BLOCK_TILE, SCAN_TILE = 64, 256, 2048              # csrc/fqd_umi.hip: kWaveTile, kTile; fqd_record_scan.hpp: kOffTile
COUNTS = [0, 1, WAVE_TILE - 1, WAVE_TILE, WAVE_TILE + 1, BLOCK_TILE - 1, BLOCK_TILE, BLOCK_TILE + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1]


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def sep_char(sep):
    return sep.decode()


class IdLines:
    """ID lines in device memory: line i at a start that is i mod 16 with at least one byte of FILL in front (`gaps`), or
    back to back; pad bytes of FILL behind the last one (0: it ends with the allocation)."""
    def __init__(self, lines, gaps=True, pad=PAD):
        n = len(lines)
        lens = np.array([len(x) for x in lines], dtype=np.uint32)
        starts = np.zeros(n, np.uint64)
        at = 0
        for i in range(n):
            if gaps:
                at += 1 + (i - at - 1) % 16
            starts[i] = at
            at += int(lens[i])
        buf = np.full(max(at + pad, 1), FILL, np.uint8)
        for i, x in enumerate(lines):
            buf[int(starts[i]):int(starts[i]) + len(x)] = np.frombuffer(x, np.uint8)
        self.n, self.size = n, at + pad
        self.text, self.start, self.len = dev(buf), dev(starts if n else np.zeros(1, np.uint64)), dev(lens if n else np.zeros(1, np.uint32))


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
                at += 1 + (i - at - 1) % 16
            offs[i] = at
            at += int(lens[i])
        buf = np.full(max(at + pad, 1), FILL, np.uint8)
        for i, r in enumerate(reads):
            buf[int(offs[i]):int(offs[i]) + len(r)] = np.frombuffer(r, np.uint8)
        self.bases, self.offs, self.lens = dev(buf), dev(offs if n else np.zeros(1, np.uint64)), dev(lens if n else np.zeros(1, np.uint32))
        self.desc = Reads(self.bases, offsets=self.offs, lengths=self.lens)


def info_tuple(info):
    return (info.n_bases, info.umi_len, info.joiners, info.bad_record, info.bad_reason)


def find(e, lines, sep, gaps=True, pad=PAD):
    """Runs fqd_umi_find and asserts umi_off and info against the statement; returns (IdLines, umi_off, info)."""
    ids = IdLines(lines, gaps, pad)
    n = len(lines)
    umi_off = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    before = ids.text.clone()
    info = e.umi_find(ids.text, ids.start, ids.len, n, sep_char(sep), umi_off)
    e.sync()
    exp_off, exp = ref.find(lines, sep)
    assert info_tuple(info) == (exp["n_bases"], exp["umi_len"], exp["joiners"], exp["bad_record"], exp["bad_reason"])
    got = host(umi_off, np.uint32)
    assert np.array_equal(got[:n], exp_off)
    assert np.all(got[n:] == 0xFFFFFFFF)                       # nothing behind the last entry
    assert torch.equal(ids.text, before)
    return ids, umi_off, info


def find_and_pack(lines, seqs, sep, kind="gaps", pad=PAD, engine=None):
    """find, then fqd_umi_reads over the sequences; asserts everything against the statement.  Returns the device arrays
    (out, off, len) for a submit."""
    n = len(lines)
    exp_buf, exp_off, exp_len = ref.expected_layout(lines, seqs, sep)
    lay = Layout(seqs, kind, pad)
    out = torch.full((len(exp_buf) + PAD,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((n + GUARD,), -1, dtype=torch.int64, device="cuda")
    ln = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    e = engine or Engine(segments=1)
    try:
        ids, umi_off, info = find(e, lines, sep, pad=pad)
        assert info.bad_record == ref.NO_RECORD
        e.umi_reads(ids.text, ids.start, umi_off, info, lay.desc, n, out, off, ln, out_capacity=len(exp_buf))
        e.sync()
    finally:
        if engine is None:
            e.close()
    got = out.cpu().numpy()
    assert got[:len(exp_buf)].tobytes() == exp_buf
    assert np.all(got[len(exp_buf):] == FILL)                  # nothing behind the last byte
    assert np.array_equal(host(off, np.uint64)[:n], exp_off) and np.all(host(off, np.uint64)[n:] == 0xFFFFFFFFFFFFFFFF)
    assert np.array_equal(host(ln, np.uint32)[:n], exp_len) and np.all(host(ln, np.uint32)[n:] == 0xFFFFFFFF)
    return out, off, ln


def lines_of_one_shape(rng, n, sep, umi_len=8, joiner_at=(), ends=(15, 16, 17, 30, 47, 255, 256, 257, 600)):
    """n ID lines whose UMIs have one shape; the word's end drawn from `ends` where the UMI fits."""
    out = []
    for _ in range(n):
        u = bytearray(random_umi(rng, umi_len))
        for k, p in enumerate(joiner_at):
            u[p] = b"+-"[k % 2] if sep == UNDERSCORE else b"+-_"[k % 3]
        fits = [x for x in ends if x >= umi_len + 2]
        ending = rng.choice([b" 1:N:0:AC_GT\n", b"\n", b"\tx:y\n", b"\r\n"])
        out.append(id_line(rng, rng.choice(fits) if fits else umi_len + 2, bytes(u), sep, ending, lead=rng.choice([b"@", b">"])))
    return out


def random_seqs(rng, n, lengths=(0, 1, 15, 16, 17, 40, 150, 255, 256, 257)):
    return [random_umi(rng, rng.choice(lengths)) for _ in range(n)]


# ---------------------------------------------------------------- the find alone

def test_every_line_the_rule_takes():
    # the edge list, one file per shape: every case both alone-shaped and among 64-record tiles of its like
    groups = {}
    for name, line, sep in taken_cases():
        groups.setdefault((sep, ref.shape(ref.umi_of(line, sep)[1])), []).append(line)
    assert len(groups) > 30
    with Engine(segments=1) as e:
        for (sep, _), lines in groups.items():
            _, _, info = find(e, lines, sep)
            assert info.bad_record == ref.NO_RECORD and info.n_bases > 0


def test_every_line_the_rule_refuses():
    rng = random.Random(61)
    seen = set()
    with Engine(segments=1) as e:
        for name, line, sep, reason in refused_cases():
            _, _, info = find(e, [line], sep)                   # as record 0
            assert (info.bad_record, info.bad_reason, info.n_bases, info.umi_len, info.joiners) == (0, reason, 0, 0, 0), name
            good = lines_of_one_shape(rng, 140, sep)
            lines = good[:67] + [line] + good[67:] + [line]     # as record 67 and once more far behind: the lowest is reported
            _, _, info = find(e, lines, sep)
            assert (info.bad_record, info.bad_reason, info.n_bases, info.umi_len) == (67, reason, 8, 8), name
            seen.add(reason)
    assert seen == {ref.NO_SEPARATOR, ref.EMPTY, ref.TOO_LONG, ref.BAD_BYTE, ref.NO_BASE}


def test_files_are_held_against_record_zero():
    seen = set()
    with Engine(segments=1) as e:
        for name, lines, sep in shape_files():
            _, _, info = find(e, lines, sep)
            seen.add((info.bad_record, info.bad_reason))
    assert {(ref.NO_RECORD, ref.OK), (1, ref.SHAPE_DIFFERS), (69, ref.SHAPE_DIFFERS), (13, ref.SHAPE_DIFFERS), (0, ref.NO_SEPARATOR), (20, ref.BAD_BYTE)} <= seen


@pytest.mark.parametrize("where", ["record 1", "the last record", "two places"])
@pytest.mark.parametrize("n", [2049, 300])
def test_a_differing_shape_is_reported_at_its_lowest_record(n, where):
    rng = random.Random(n)
    lines = lines_of_one_shape(rng, n, COLON, umi_len=9, joiner_at=(4,))
    other = id_line(rng, 40, b"ACG+TACGT", COLON)
    at = {"record 1": [1], "the last record": [n - 1], "two places": [n - 2, 257]}[where]
    for a in at:
        lines[a] = other
    with Engine(segments=1) as e:
        _, _, info = find(e, lines, COLON)
    assert (info.bad_record, info.bad_reason) == (min(at), ref.SHAPE_DIFFERS)


@pytest.mark.parametrize("end_at", [2, 15, 16, 17, 255, 256, 257, 600])
@pytest.mark.parametrize("pad", [0, PAD], ids=["ends with its allocation", "padded"])
def test_the_last_id_line(end_at, pad):
    # no byte behind the last ID line belongs to the caller; 70 records: the last wave's tile holds 6, the rest lie beyond n
    rng = random.Random(end_at)
    lines = lines_of_one_shape(rng, 69, COLON, umi_len=1)
    for ending in (b"\n", b" x\n", b""):
        last = id_line(rng, end_at, b"T", COLON, ending) if end_at > 2 else b"@\n"
        with Engine(segments=1) as e:
            ids, _, info = find(e, lines + [last], COLON, gaps=False, pad=pad)
        assert ids.size == sum(map(len, lines)) + len(last) + pad
        assert info.bad_record == (69 if end_at == 2 else ref.NO_RECORD)


# ---------------------------------------------------------------- find and pack

@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("sep", [COLON, UNDERSCORE], ids=["colon", "underscore"])
def test_record_counts_round_the_tiles(n, sep):
    rng = random.Random(n)
    find_and_pack(lines_of_one_shape(rng, n, sep, umi_len=9, joiner_at=(4,)), random_seqs(rng, n), sep)


@pytest.mark.parametrize("bases", [1, 15, 16, 17, 64])
@pytest.mark.parametrize("joiners", [0, 1, 2])
def test_umi_lengths_and_joiners(bases, joiners):
    if bases + joiners > 64:
        bases -= joiners
    rng = random.Random(bases * 3 + joiners)
    umi_len = bases + joiners
    at = sorted(rng.sample(range(umi_len), joiners))
    # the word's end so that U lies across a 16-byte boundary of the line, across the 256-byte round, and flush with the line's start
    lines = lines_of_one_shape(rng, 200, COLON, umi_len, at, ends=(umi_len + 2, umi_len + 9, 256 + umi_len // 2 + 1, 300))
    _, info = ref.find(lines, COLON)
    assert info["n_bases"] == bases
    find_and_pack(lines, random_seqs(rng, 200), COLON)


@pytest.mark.parametrize("L", [0, 1, 15, 16, 17, 255, 256, 257])
@pytest.mark.parametrize("kind", ["gaps", "uniform"])
def test_sequence_lengths(L, kind):
    # gaps: the sources at every offset mod 16; the destinations take every alignment as Lb + L runs on
    rng = random.Random(L)
    n = 150
    lines = lines_of_one_shape(rng, n, UNDERSCORE, umi_len=7)
    find_and_pack(lines, [random_umi(rng, L) for _ in range(n)], UNDERSCORE, kind)


@pytest.mark.parametrize("last", [0, 1, 15, 16, 17, 150, 600])
def test_the_last_read_ends_with_its_allocation(last):
    rng = random.Random(last)
    lines = lines_of_one_shape(rng, 70, COLON, umi_len=12, joiner_at=(6,))
    seqs = random_seqs(rng, 69, (0, 3, 16, 40, 150)) + [random_umi(rng, last)]
    find_and_pack(lines, seqs, COLON, "gaps", pad=0)


# ---------------------------------------------------------------- end to end through the binding

def submit_flags(descs, n, S):
    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    with Engine(segments=S) as e:
        e.submit(descs, n, keep=keep, final=True)
        e.sync()
    return keep.cpu().numpy()


def test_a_paired_engine_takes_mate_two_untouched():
    rng = random.Random(71)
    n = 3000
    pool = [(random_umi(rng, 8), random_umi(rng, rng.choice([30, 150]), "ACGT"), random_umi(rng, rng.choice([20, 150]), "ACGT")) for _ in range(n // 3)]
    recs = []
    for _ in range(n):
        u, a, b = rng.choice(pool)
        roll = rng.random()
        if roll < 0.2:
            u = random_umi(rng, 8)                              # the same pair from another molecule
        elif roll < 0.3:
            b = random_umi(rng, len(b), "ACGT")
        recs.append((u, a, b))
    lines = [id_line(rng, rng.choice([20, 40]), u, COLON) for u, _, _ in recs]
    exp_keep = ref.expected_keep([ref.key_of(l, COLON, a, b) for l, (_, a, b) in zip(lines, recs)])
    plain = ref.expected_keep([(a, b) for _, a, b in recs])
    assert int(exp_keep.sum()) > int(plain.sum())
    mate2 = Layout([b for _, _, b in recs], "gaps")
    before = (mate2.bases.clone(), mate2.offs.clone(), mate2.lens.clone())
    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    with Engine(segments=2) as e:
        out, off, ln = find_and_pack(lines, [a for _, a, _ in recs], COLON, "gaps", engine=e)
        e.submit([Reads(out, offsets=off, lengths=ln), mate2.desc], n, keep=keep, final=True)
        e.sync()
        assert e.stats()["duplicates"] == int((exp_keep == 0).sum())
    assert np.array_equal(keep.cpu().numpy(), exp_keep)
    assert all(torch.equal(x, y) for x, y in zip(before, (mate2.bases, mate2.offs, mate2.lens)))


def test_three_hundred_thousand_reads_keyed_by_umi_and_sequence():
    rng = np.random.default_rng(19)
    n, L, U = 300_000, 150, 8
    seq = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=(n, L), p=[.245, .245, .245, .245, .02])
    umi = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=(n, U))
    origin = np.arange(n)
    is_copy = rng.random(n) < 0.2
    is_copy[0] = False
    idx = np.flatnonzero(is_copy)
    origin[idx] = (rng.random(len(idx)) * idx).astype(np.int64)
    for _ in range(64):                                         # copies of copies: down to the fresh record
        nxt = origin[origin]
        if np.array_equal(nxt, origin):
            break
        origin = nxt
    other = is_copy & (rng.random(n) < 0.5)                     # half the copies come from another molecule
    seq = seq[origin]
    umi = np.where(other[:, None], umi, umi[origin])
    # "@A00:7:<7 digits>:<UMI> 1:N:0\n": one length, so numpy lays the lines out
    digits = np.frombuffer(b"".join(b"%07d" % i for i in range(n)), np.uint8).reshape(n, 7)
    head, tail = np.frombuffer(b"@A00:7:", np.uint8), np.frombuffer(b" 1:N:0\n", np.uint8)
    lines = np.concatenate([np.broadcast_to(head, (n, len(head))), digits, np.full((n, 1), ord(":"), np.uint8), umi,
                            np.broadcast_to(tail, (n, len(tail)))], axis=1)
    W = lines.shape[1]
    umi_at = len(head) + 7 + 1
    assert ref.umi_of(lines[n - 1].tobytes(), COLON) == (umi_at, umi[n - 1].tobytes())
    exp_keep = ref.first_occurrence_rows(umi, seq)
    plain_keep = ref.first_occurrence_rows(seq)
    assert int(plain_keep.sum()) < int(exp_keep.sum()) < n

    text = dev(np.concatenate([lines.reshape(-1), np.full(PAD, FILL, np.uint8)]))
    start = dev(np.arange(n, dtype=np.uint64) * np.uint64(W))
    id_len = dev(np.full(n, W, np.uint32))
    bases = dev(np.concatenate([seq.reshape(-1), np.full(PAD, FILL, np.uint8)]))
    given = Reads(bases, uniform_len=L, uniform_stride=L)
    umi_off = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    out = torch.full((n * (U + L) + PAD,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    ln = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        info = e.umi_find(text, start, id_len, n, ":", umi_off)
        assert info_tuple(info) == (U, U, 0, ref.NO_RECORD, ref.OK)
        e.umi_reads(text, start, umi_off, info, given, n, out, off, ln, out_capacity=n * (U + L))
        e.submit([Reads(out, offsets=off, lengths=ln)], n, keep=keep, final=True)
        e.sync()
        assert e.stats()["duplicates"] == int((exp_keep == 0).sum())
    assert bool((umi_off == umi_at).all())
    got = out.cpu().numpy()
    assert np.array_equal(got[:n * (U + L)].reshape(n, U + L), np.concatenate([umi, seq], axis=1))
    assert np.all(got[n * (U + L):] == FILL)
    assert np.array_equal(host(off, np.uint64), np.arange(n, dtype=np.uint64) * np.uint64(U + L))
    assert np.all(host(ln, np.uint32) == U + L)
    assert np.array_equal(keep.cpu().numpy(), exp_keep)
    plain = submit_flags([given], n, 1)
    assert np.array_equal(plain, plain_keep)
    assert int(plain.sum()) < int(exp_keep.sum())             # a plain submit of the same reads keeps strictly fewer


def test_more_reads_than_the_tile_scans_first_round():
    """The one block that scans the records' byte counts takes 1024 tiles of 2048 records a round: 1024 tiles, one tile and
    three records more, of the shortest lines and reads that numpy lays out (`@<7 digits>:<4 bases>`, reads of two bases)."""
    rng = np.random.default_rng(20)
    n, L, U = 1024 * SCAN_TILE + SCAN_TILE + 3, 2, 4
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seq, umi = rng.choice(acgt, size=(n, L)), rng.choice(acgt, size=(n, U))
    digits = (ord("0") + (np.arange(n)[:, None] // 10 ** np.arange(6, -1, -1)) % 10).astype(np.uint8)
    lines = np.concatenate([np.full((n, 1), ord("@"), np.uint8), digits, np.full((n, 1), ord(":"), np.uint8), umi, np.full((n, 1), ord("\n"), np.uint8)], axis=1)
    W, umi_at = lines.shape[1], 9
    assert lines[n - 1].tobytes() == b"@%07d:" % (n - 1) + umi[n - 1].tobytes() + b"\n"
    assert ref.umi_of(lines[n - 1].tobytes(), COLON) == (umi_at, umi[n - 1].tobytes())
    text = dev(np.concatenate([lines.reshape(-1), np.full(PAD, FILL, np.uint8)]))
    start, id_len = dev(np.arange(n, dtype=np.uint64) * np.uint64(W)), dev(np.full(n, W, np.uint32))
    bases = dev(np.concatenate([seq.reshape(-1), np.full(PAD, FILL, np.uint8)]))
    umi_off = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    out = torch.full((n * (U + L) + PAD,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    ln = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    with Engine(segments=1) as e:
        info = e.umi_find(text, start, id_len, n, ":", umi_off)
        assert info_tuple(info) == (U, U, 0, ref.NO_RECORD, ref.OK)
        e.umi_reads(text, start, umi_off, info, Reads(bases, uniform_len=L, uniform_stride=L), n, out, off, ln, out_capacity=n * (U + L))
        e.sync()
    assert bool((umi_off == umi_at).all())
    got = out.cpu().numpy()
    assert np.array_equal(got[:n * (U + L)].reshape(n, U + L), np.concatenate([umi, seq], axis=1))
    assert np.all(got[n * (U + L):] == FILL)
    assert np.array_equal(host(off, np.uint64), np.arange(n, dtype=np.uint64) * np.uint64(U + L))
    assert np.all(host(ln, np.uint32) == U + L)


# ---------------------------------------------------------------- misuse

def small_run():
    rng = random.Random(81)
    lines = lines_of_one_shape(rng, 100, COLON, umi_len=6)
    seqs = [random_umi(rng, 40, "ACGT") for _ in range(100)]
    return lines, seqs, 100 * 46


@pytest.mark.parametrize("kind", ["packed", "uniform"])
def test_a_capacity_one_byte_short_is_refused_and_nothing_is_written(kind):
    lines, seqs, total = small_run()
    lay = Layout(seqs, kind)
    out = torch.full((total + PAD,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((100,), -1, dtype=torch.int64, device="cuda")
    ln = torch.full((100,), -1, dtype=torch.int32, device="cuda")
    with Engine(segments=1) as e:
        ids, umi_off, info = find(e, lines, COLON)
        with pytest.raises(FqdError, match="out_capacity") as ei:
            e.umi_reads(ids.text, ids.start, umi_off, info, lay.desc, 100, out, off, ln, out_capacity=total - 1)
        assert ei.value.code == _lib.ERR_ARG
        e.sync()
        assert bool((out == FILL).all()) and bool((off == -1).all()) and bool((ln == -1).all())
        e.umi_reads(ids.text, ids.start, umi_off, info, lay.desc, 100, out, off, ln, out_capacity=total)      # the exact size is enough
        e.sync()
    assert out.cpu().numpy()[:total].tobytes() == ref.expected_layout(lines, seqs, COLON)[0]


def test_host_memory_is_refused():
    lines, seqs, total = small_run()
    lay = Layout(seqs, "packed")
    out = torch.full((total + PAD,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((100,), -1, dtype=torch.int64, device="cuda")
    ln = torch.full((100,), -1, dtype=torch.int32, device="cuda")
    with Engine(segments=1) as e:
        ids, umi_off, info = find(e, lines, COLON)
        host_text = ids.text.cpu().numpy()
        with pytest.raises(FqdError, match="device memory") as ei:
            e.umi_find(host_text, ids.start, ids.len, 100, ":", umi_off)
        assert ei.value.code == _lib.ERR_ARG
        with pytest.raises(FqdError, match="device memory") as ei:
            e.umi_find(ids.text, ids.start, ids.len, 100, ":", np.zeros(100, np.uint32))
        assert ei.value.code == _lib.ERR_ARG
        with pytest.raises(FqdError, match="device memory") as ei:
            e.umi_reads(host_text, ids.start, umi_off, info, lay.desc, 100, out, off, ln)
        assert ei.value.code == _lib.ERR_ARG
        host_reads = Reads(np.frombuffer(b"".join(seqs), np.uint8).copy(), uniform_len=40, uniform_stride=40)
        with pytest.raises(FqdError, match="device memory") as ei:
            e.umi_reads(ids.text, ids.start, umi_off, info, host_reads, 100, out, off, ln)
        assert ei.value.code == _lib.ERR_ARG
        with pytest.raises(FqdError, match="device memory") as ei:
            e.umi_reads(ids.text, ids.start, umi_off, info, lay.desc, 100, np.zeros(total, np.uint8), off, ln, out_capacity=total)
        assert ei.value.code == _lib.ERR_ARG
        e.sync()
    assert bool((out == FILL).all()) and bool((off == -1).all()) and bool((ln == -1).all())


def test_a_null_info_an_unknown_separator_and_a_refused_info_are_refused():
    lines, seqs, total = small_run()
    lay = Layout(seqs, "packed")
    out = torch.full((total + PAD,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((100,), -1, dtype=torch.int64, device="cuda")
    ln = torch.full((100,), -1, dtype=torch.int32, device="cuda")
    with Engine(segments=1) as e:
        ids, umi_off, info = find(e, lines, COLON)
        kept = umi_off.clone()
        with pytest.raises(FqdError, match="fqd_umi_find") as ei:
            e.umi_find(ids.text, ids.start, ids.len, 100, ":", umi_off, info=None)
        assert ei.value.code == _lib.ERR_ARG
        with pytest.raises(FqdError, match="separator") as ei:
            e.umi_find(ids.text, ids.start, ids.len, 100, "+", umi_off)
        assert ei.value.code == _lib.ERR_ARG
        with pytest.raises(FqdError, match="fqd_umi_reads") as ei:
            e.umi_reads(ids.text, ids.start, umi_off, None, lay.desc, 100, out, off, ln)
        assert ei.value.code == _lib.ERR_ARG
        for change in (dict(bad_record=3, bad_reason=ref.SHAPE_DIFFERS), dict(n_bases=5), dict(umi_len=65), dict(joiners=1 << 6), dict(umi_len=0, n_bases=0)):
            wrong = _lib.UmiInfo(info.n_bases, info.umi_len, info.joiners, info.bad_record, info.bad_reason, 0)
            for k, v in change.items():
                setattr(wrong, k, v)
            with pytest.raises(FqdError, match="fqd_umi_find leaves") as ei:
                e.umi_reads(ids.text, ids.start, umi_off, wrong, lay.desc, 100, out, off, ln)
            assert ei.value.code == _lib.ERR_ARG
        e.sync()
        assert torch.equal(umi_off, kept)
    assert bool((out == FILL).all()) and bool((off == -1).all()) and bool((ln == -1).all())
