"""Encoder output, bit for bit: every key word (and hash, where the entry point hands one out) that the device's
encoders write equals the plain statement of the layout in tests/key_layout.py.

The other GPU tests judge the encoders by keep flags on reads of which any two differ in most bases, or by holding
one encoder against another (all share pack_mate): a dropped N bit, a lost last base of a tile's last record or a
key word parked over bytes another lane has yet to read would leave them green.  Here the words are read back.

Which kernel and branch a case takes is read off choose_staged / launch_encode (csrc/fqd_engine.hip):
  uniform input, not FQD_FLAG_NO_STAGE: the largest tile R in 256/192/128/64 (pairs: R/2 pairs) with
      round16(R * stride + 32) [+ the same for mate 2] <= 64 KiB -> encode_staged_kernel / encode_staged_pe_kernel;
      <LDS_OUT = true> iff the key slots are contiguous, rw = W0 + lead > 1 and stride_m >= 8 * row_m + 15
      (row_0 = lead + W_0, row_1 = W_1); magic == 0 (16 bytes per lane stream-out) iff LDS_OUT and rw is a power of
      two >= 2 (pairs: and lead + W_0 even), else the division form.  No R fits: encode_general_kernel.
  ragged descriptors, not NO_STAGE: encode_span_kernel<S>, tile by tile LDS-staged or straight from HBM.
  NO_STAGE: encode_general_kernel<S>.
  fqd_encode_slabs[_hashed], one pass: encode_chunks_kernel / encode_chunks_pe_kernel.
Engines run without weak_hash: the flag masks the hashes they write.
"""
import numpy as np
import pytest
import torch

import key_layout as kl
from fastq_dupaway_amd import Engine, Reads
from test_shard import _Words          # raw device memory as something torch can alias

pytestmark = pytest.mark.gpu

N_SE = 3 * 256 + 77          # whole tiles and a short one, more than one workgroup
N_PE = 3 * 128 + 77
SE_LENGTHS = [1, 17, 31, 32, 33, 63, 64, 65, 100, 128, 149, 150, 151, 250, 256]
PE_LENGTHS = [(150, 150), (150, 101), (100, 150), (33, 33), (1, 64)]
ACGTN = np.frombuffer(b"ACGTN", np.uint8)
JUNK = np.frombuffer(b"@+#!IF\n~", np.uint8)           # what lies between the sequences: must never reach a key


def make_rows(seed, n, L):
    """n reads of L random ACGTN; rows of all N, all G, all A and one with N at 0, 31, 32, 63, 64, L-1 lead the
    batch, and the same four close it (the last records of the short tile)."""
    rng = np.random.default_rng(seed)
    rows = rng.choice(ACGTN, size=(n, L), p=[.23, .23, .23, .23, .08])
    for at in (0, n - 4):
        rows[at, :] = ord("N"); rows[at + 1, :] = ord("G"); rows[at + 2, :] = ord("A")
        for p in (0, 31, 32, 63, 64, L - 1):
            if p < L:
                rows[at + 3, p] = ord("N")
    return rows


def lay_out(rows, stride, offset, seed=0):
    """The rows `stride` bytes apart, the first `offset` bytes into a device buffer of junk; returns the view that
    starts at the first sequence (so its address is offset (mod 4) when offset < 4)."""
    n, L = rows.shape
    rng = np.random.default_rng(seed + stride)
    flat = rng.choice(JUNK, size=offset + n * stride + 64)
    body = flat[offset: offset + n * stride].reshape(n, stride)
    body[:, :L] = rows
    return torch.from_numpy(flat).cuda()[offset:]


def strides_for(L):
    """(stride, offset): back to back, one byte apart, and a FASTQ-like record (150 bases: 319 bytes) whose sequence
    starts 1, 2 and 3 bytes (mod 4) into the buffer."""
    fastq = 2 * L + 19
    return [(L, 0), (L + 1, 0), (fastq, 41), (fastq, 42), (fastq, 43)]


def check(got, exp, what, col0=0):
    """got, exp: (n, k) uint64.  A mismatch names the encoder and shape (what), the record and the word."""
    assert got.shape == exp.shape, f"{what}: shape {got.shape} against {exp.shape}"
    bad = np.argwhere(got != exp)
    if len(bad):
        i, k = (int(x) for x in bad[0])
        name = "hash" if k + col0 < 0 else f"word {k + col0}"
        raise AssertionError(f"{what}: record {i}, {name}: got {int(got[i, k]):#018x}, expected {int(exp[i, k]):#018x} "
                             f"({len(bad)} words of {len(set(bad[:, 0].tolist()))} records differ)")


def read_store(e, n, L0, L1):
    """The engine's uniform key store (lead 0, stride W0: key j at keys + j * W0): fqd_reserve_keys(0, ...) names its tail."""
    W = e.key_words(L0, L1)
    tail = e.reserve_keys(0, L0, L1)
    return torch.as_tensor(_Words(tail - n * W * 8, n * W), device="cuda").cpu().numpy().view(np.uint64).reshape(n, W)


# ---------------------------------------------------------------------------------------------------------
# fqd_submit, single-end, uniform: encode_staged_kernel into the key store (lead 0, rw = W0)
#   L:   1   17  31  32  33  63  64  65  100  128  149  150  151  250  256
#   rw:  2   2   2   2   3   3   3   5   6    6    8    8    8    12   12
#   rw 2, 8: magic 0 (16 bytes per lane) where LDS_OUT; rw 3, 5, 6, 12: the division form.
#   LDS_OUT needs stride >= 8 * rw + 15: off for L = 1 (strides 1, 2), L = 17 (17, 18: needs 31), L = 31 / 32 / 33
#   back to back or a byte apart (need 31 / 31 / 39), 63 / 64 at stride L (need 39: on), 65 (needs 55: on) ...; the
#   FASTQ-like stride turns it on for every length but L = 1 (21 < 31).  All strides here give R = 256.
@pytest.mark.parametrize("L", SE_LENGTHS)
def test_submit_se_key_store(L):
    rows_a, rows_b = make_rows(L, N_SE, L), make_rows(1000 + L, N_SE, L)
    exp = np.concatenate([kl.words_of_rows(rows_a), kl.words_of_rows(rows_b)])
    assert [int(x) for x in exp[3]] == kl.expected_words(bytes(rows_a[3]))        # the batch form against the scalar statement
    for stride, offset in strides_for(L):
        what = f"encode_staged_kernel via submit, L={L} stride={stride} offset={offset}"
        with Engine(segments=1) as e:
            keep = torch.zeros(2 * N_SE, dtype=torch.uint8, device="cuda")
            e.submit([Reads(lay_out(rows_a, stride, offset), uniform_len=L, uniform_stride=stride)], N_SE, keep)
            e.sync()
            check(read_store(e, N_SE, L, 0), exp[:N_SE], what + ", first batch")
            e.submit([Reads(lay_out(rows_b, stride, offset), uniform_len=L, uniform_stride=stride)], N_SE, keep[N_SE:])   # first_idx != 0
            e.sync()
            check(read_store(e, 2 * N_SE, L, 0), exp, what + ", both batches")


# Tile tiers (L = 150, rw 8, LDS_OUT, magic 0): stride 150 -> R 256 (38 447 B), 304 -> R 192 (256 * 304 > 64 KiB),
# 500 -> R 128, 1000 -> R 64, 1100 -> no tile fits: encode_general_kernel<1>.
@pytest.mark.parametrize("stride", [150, 304, 500, 1000, 1100])
def test_submit_se_tile_tiers(stride):
    L = 150
    rows = make_rows(stride, N_SE, L)
    exp = kl.words_of_rows(rows)
    for offset in (0, 3):
        with Engine(segments=1) as e:
            keep = torch.zeros(N_SE, dtype=torch.uint8, device="cuda")
            e.submit([Reads(lay_out(rows, stride, offset), uniform_len=L, uniform_stride=stride)], N_SE, keep)
            e.sync()
            check(read_store(e, N_SE, L, 0), exp, f"submit (tile tier), L={L} stride={stride} offset={offset}")


# ---------------------------------------------------------------------------------------------------------
# fqd_submit, paired, uniform: encode_staged_pe_kernel (R = 256: 128 pairs per tile at all these strides)
#   (150, 150): rw 16, split 8 even -> magic 0;  (150, 101): rw 14, (100, 150): rw 14, (33, 33): rw 6 (split 3),
#   (1, 64): rw 5 -> the division form.  LDS_OUT needs stride_m >= 8 * W_m + 15 for both mates: off back to back
#   for (33, 33) (39 > 33/34) and (1, 64); on with the FASTQ-like strides except for the 1-base mate (21 < 31).
def pe_strides(L0, L1):
    return [((L0, 0), (L1, 0)), ((L0 + 1, 0), (L1 + 1, 0)), ((2 * L0 + 19, 41), (2 * L1 + 19, 43)), ((2 * L0 + 19, 42), (2 * L1 + 23, 40))]


@pytest.mark.parametrize("L0,L1", PE_LENGTHS)
def test_submit_pe_key_store(L0, L1):
    batches = [(make_rows(7 * L0 + L1 + 100 * b, N_PE, L0), make_rows(11 * L0 + L1 + 100 * b, N_PE, L1)) for b in range(2)]
    exp = np.concatenate([np.concatenate([kl.words_of_rows(r0), kl.words_of_rows(r1)], axis=1) for r0, r1 in batches])
    assert [int(x) for x in exp[3]] == kl.expected_pair_words(bytes(batches[0][0][3]), bytes(batches[0][1][3]))
    for (s0, o0), (s1, o1) in pe_strides(L0, L1):
        what = f"encode_staged_pe_kernel via submit, L=({L0}, {L1}) strides=({s0}, {s1}) offsets=({o0}, {o1})"
        with Engine(segments=2) as e:
            keep = torch.zeros(2 * N_PE, dtype=torch.uint8, device="cuda")
            for b, (r0, r1) in enumerate(batches):
                segs = [Reads(lay_out(r0, s0, o0), uniform_len=L0, uniform_stride=s0), Reads(lay_out(r1, s1, o1), uniform_len=L1, uniform_stride=s1)]
                e.submit(segs, N_PE, keep[b * N_PE:])
                e.sync()
                check(read_store(e, (b + 1) * N_PE, L0, L1), exp[: (b + 1) * N_PE], what + f", {b + 1} batch(es)")


# ---------------------------------------------------------------------------------------------------------
# fqd_encode_uniform: records [hash, words] (lead 1, rw = W0 + 1), staged (no_stage False) and encode_general (True)
#   L:   1   17  31  32  33  63  64  65  100  128  149  150  151  250  256
#   rw:  3   3   3   3   4   4   4   6   7    7    9    9    9    13   13      (rw 4: magic 0; the rest divide)
@pytest.mark.parametrize("no_stage", [False, True])
@pytest.mark.parametrize("L", SE_LENGTHS)
def test_encode_uniform_se_records(L, no_stage):
    rows = make_rows(50 + L, N_SE, L)
    words = kl.words_of_rows(rows)
    exp = np.concatenate([kl.hashes_of_rows(L, words)[:, None], words], axis=1)
    assert int(exp[3, 0]) == kl.expected_hash(L, 0, kl.expected_words(bytes(rows[3])))
    extra = [] if no_stage or L != 150 else [(304, 1), (500, 2), (1000, 3), (1100, 1)]       # the tile tiers again, lead 1
    with Engine(segments=1, no_stage=no_stage) as e:
        for stride, offset in strides_for(L) + extra:
            rec = torch.full((N_SE * exp.shape[1],), -7, dtype=torch.int64, device="cuda")
            e.encode_uniform([Reads(lay_out(rows, stride, offset), uniform_len=L, uniform_stride=stride)], N_SE, rec)
            e.sync()
            got = rec.cpu().numpy().view(np.uint64).reshape(N_SE, -1)
            check(got, exp, f"{'encode_general_kernel<1>' if no_stage else 'encode_staged_kernel'} via encode_uniform, "
                            f"L={L} stride={stride} offset={offset}", col0=-1)


# pairs: rw = 17 (150, 150), 15, 15, 7 (33, 33), 6 (1, 64): none a power of two -> the division form with lead 1
@pytest.mark.parametrize("no_stage", [False, True])
@pytest.mark.parametrize("L0,L1", PE_LENGTHS)
def test_encode_uniform_pe_records(L0, L1, no_stage):
    r0, r1 = make_rows(3 * L0 + L1, N_PE, L0), make_rows(5 * L0 + L1, N_PE, L1)
    w0, w1 = kl.words_of_rows(r0), kl.words_of_rows(r1)
    exp = np.concatenate([kl.hashes_of_rows(L0, w0, L1, w1)[:, None], w0, w1], axis=1)
    assert int(exp[3, 0]) == kl.expected_hash(L0, L1, kl.expected_words(bytes(r0[3])), kl.expected_words(bytes(r1[3])))
    with Engine(segments=2, no_stage=no_stage) as e:
        for (s0, o0), (s1, o1) in pe_strides(L0, L1):
            rec = torch.full((N_PE * exp.shape[1],), -7, dtype=torch.int64, device="cuda")
            segs = [Reads(lay_out(r0, s0, o0), uniform_len=L0, uniform_stride=s0), Reads(lay_out(r1, s1, o1), uniform_len=L1, uniform_stride=s1)]
            e.encode_uniform(segs, N_PE, rec)
            e.sync()
            got = rec.cpu().numpy().view(np.uint64).reshape(N_PE, -1)
            check(got, exp, f"{'encode_general_kernel<2>' if no_stage else 'encode_staged_pe_kernel'} via encode_uniform, "
                            f"L=({L0}, {L1}) strides=({s0}, {s1}) offsets=({o0}, {o1})", col0=-1)


# ---------------------------------------------------------------------------------------------------------
# fqd_encode_padded, ragged descriptors
RAGGED_MAX = (160, 130)


def ragged_reads(seed, n, max_len):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, n)
    edge = [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, max_len - 1, max_len]
    lens[: len(edge)] = edge
    lens[n - 3:] = (max_len, 64, 1)                                      # the short tile's last records
    reads = [rng.choice(ACGTN, size=int(l), p=[.23, .23, .23, .23, .08]) for l in lens]
    for k, fill in ((20, "N"), (21, "G"), (22, "A")):
        reads[k] = np.full(max_len, ord(fill), np.uint8)
    for p in (0, 31, 32, 63, 64, max_len - 1):
        reads[15][p] = ord("N")
    return reads


def ragged_layout(reads, layout, seed):
    """packed: back to back.  gaps: FASTQ-like gaps, and from record 384 on 700 bytes between records (a tile's span
    no longer fits its LDS budget).  shuffled: small gaps, the records' places permuted inside every tile of 128."""
    n = len(reads)
    rng = np.random.default_rng(seed)
    place = np.arange(n)
    if layout == "shuffled":
        for a in range(0, n, 128):
            place[a: a + 128] = rng.permutation(place[a: a + 128])
    offs = np.zeros(n, np.int64)
    chunks, pos = [], 3                                                   # the first sequence starts 3 bytes in
    chunks.append(rng.choice(JUNK, size=3))
    for slot in range(n):
        k = int(place[slot])
        gap = 0 if layout == "packed" else (700 if layout == "gaps" and slot >= 384 else int(rng.integers(1, 40)))
        chunks.append(rng.choice(JUNK, size=gap)); pos += gap
        offs[k] = pos
        chunks.append(reads[k]); pos += len(reads[k])
    chunks.append(rng.choice(JUNK, size=64))
    return np.concatenate(chunks).astype(np.uint8), offs, np.array([len(r) for r in reads], np.int32)


@pytest.fixture(scope="module")
def ragged_expected():
    """The reads of the padded cases and their expected records, computed once."""
    out = {}
    for paired in (False, True):
        n = N_PE if paired else N_SE
        m0 = ragged_reads(1, n, RAGGED_MAX[0])
        m1 = ragged_reads(2, n, RAGGED_MAX[1]) if paired else None
        rows = []
        for i in range(n):
            s0, s1 = bytes(m0[i]), bytes(m1[i]) if paired else None
            h = kl.expected_hash(len(s0), len(s1) if paired else 0, kl.expected_words(s0), kl.expected_words(s1) if paired else None)
            rows.append([h] + kl.expected_padded(s0, s1, RAGGED_MAX[0], RAGGED_MAX[1] if paired else 0))
        out[paired] = (m0, m1, np.array(rows, np.uint64))
    return out


@pytest.mark.parametrize("no_stage", [False, True])
@pytest.mark.parametrize("layout", ["packed", "gaps", "shuffled"])
@pytest.mark.parametrize("paired", [False, True])
def test_encode_padded_ragged_records(ragged_expected, paired, layout, no_stage):
    """Records [hash][len0 | len1 << 32][words][zeros].  launch_encode: descriptors with offsets and not NO_STAGE ->
    encode_span_kernel<S> (tiles of 128 records; LDS budget 48 KiB single-end, 24 KiB per mate paired):
      packed    every tile's span (<= 128 * 160 B) fits and holds all its records: LDS-staged;
      gaps      tiles 0-2 staged (gaps < 40 B); from record 384 on the records lie 700 B apart, a tile spans > 89 KB:
                straight from HBM;
      shuffled  a tile's first record is no longer its lowest, some record lies outside [first, last]: the tile is
                vetoed, straight from HBM (a tile whose permutation keeps first and last in place would stage);
    no_stage=True: encode_general_kernel<S> for all three."""
    m0, m1, exp = ragged_expected[paired]
    n = len(m0)
    K = kl.padded_key_words(RAGGED_MAX[0], RAGGED_MAX[1] if paired else 0)
    assert exp.shape == (n, K + 1)
    segs = []
    for m, reads in enumerate([m0, m1] if paired else [m0]):
        data, offs, lens = ragged_layout(reads, layout, 10 + m)
        segs.append(Reads(torch.from_numpy(data).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda()))
    kernel = f"encode_general_kernel<{len(segs)}>" if no_stage else f"encode_span_kernel<{len(segs)}>"
    with Engine(segments=len(segs), no_stage=no_stage) as e:
        assert e.padded_key_words(RAGGED_MAX[0], RAGGED_MAX[1] if paired else 0) == K
        rec = torch.full((n * (K + 1),), -7, dtype=torch.int64, device="cuda")
        e.encode_padded(segs, n, RAGGED_MAX[0], RAGGED_MAX[1] if paired else 0, rec)
        e.sync()
    check(rec.cpu().numpy().view(np.uint64).reshape(n, K + 1), exp, f"{kernel} via encode_padded, layout={layout} paired={paired}", col0=-1)


# ---------------------------------------------------------------------------------------------------------
# fqd_encode_slabs / fqd_encode_slabs_hashed, one pass: encode_chunks_kernel / encode_chunks_pe_kernel
@pytest.mark.parametrize("hashed", [False, True])
@pytest.mark.parametrize("parts", [1, 3, 16])
@pytest.mark.parametrize("lens", [(150,), (100,), (33,), (150, 150), (150, 101), (33, 33)])
def test_encode_slabs_one_pass(lens, parts, hashed):
    """Chunks of two tiles (so a workgroup carries its running counts over a tile boundary), sub-slabs that hold a
    whole chunk: every filled slot holds the words of read origin[slot] and, hashed, its hash; every read is there
    once, in the slab of owner (hash >> 40) % parts, in input order inside its sub-slab."""
    S = len(lens)
    n = N_PE if S == 2 else N_SE
    per_tile = 128 if S == 2 else 256
    chunk, sub_cap = 2 * per_tile, 2 * per_tile
    G = -(-n // chunk)
    rows = [make_rows(900 + 13 * lens[m] + m, n, lens[m]) for m in range(S)]
    words = [kl.words_of_rows(r) for r in rows]
    exp_w = np.concatenate(words, axis=1)
    exp_h = kl.hashes_of_rows(lens[0], words[0], *((lens[1], words[1]) if S == 2 else ()))
    W = exp_w.shape[1]
    what = f"{'encode_chunks_pe_kernel' if S == 2 else 'encode_chunks_kernel'} via encode_slabs{'_hashed' if hashed else ''}, L={lens} parts={parts}"
    with Engine(segments=S) as e:
        # stride L + 7: >= 8 * W_m + 15 for these lengths (keys parked in LDS) and a 256-read tile within 64 KiB, so one pass applies
        segs = [Reads(lay_out(rows[m], lens[m] + 7, 41 + m), uniform_len=lens[m], uniform_stride=lens[m] + 7) for m in range(S)]
        slots = parts * G * sub_cap + n
        keys = torch.full((slots * W,), -7, dtype=torch.int64, device="cuda")
        hashes = torch.full((slots,), -7, dtype=torch.int64, device="cuda")
        origin = torch.full((slots,), -7, dtype=torch.int32, device="cuda")
        counts = torch.full((parts * G,), -7, dtype=torch.int64, device="cuda")
        totals = torch.full((parts + 1,), -7, dtype=torch.int64, device="cuda")
        if hashed:
            e.encode_slabs_hashed(segs, n, parts, chunk, G, sub_cap, keys, hashes, counts, totals, origin)
        else:
            e.encode_slabs(segs, n, parts, chunk, G, sub_cap, keys, counts, totals, origin)
        e.sync()
    totals = totals.cpu().numpy()
    assert totals[parts] == 0, what + ": not the one-pass form"               # the layout word: 0 = sub-slab by sub-slab
    used = parts * G * sub_cap
    origin = origin.cpu().numpy().view(np.uint32)[:used]
    keys = keys.cpu().numpy().view(np.uint64).reshape(slots, W)[:used]
    hashes = hashes.cpu().numpy().view(np.uint64)[:used]
    counts = counts.cpu().numpy().reshape(parts, G)
    filled = np.flatnonzero(origin != 0xFFFFFFFF)
    src = origin[filled].astype(np.int64)
    assert np.array_equal(np.sort(src), np.arange(n)), what + ": every read in exactly one slot"
    bad = np.argwhere(keys[filled] != exp_w[src])
    if len(bad):
        s, k = int(filled[bad[0][0]]), int(bad[0][1])
        raise AssertionError(f"{what}: slot {s} (record {int(origin[s])}), word {k}: got {int(keys[s, k]):#018x}, "
                             f"expected {int(exp_w[int(origin[s]), k]):#018x} ({len(bad)} words differ)")
    if hashed:
        bad = np.flatnonzero(hashes[filled] != exp_h[src])
        assert not len(bad), (f"{what}: slot {int(filled[bad[0]])} (record {int(src[bad[0]])}), hash: got {int(hashes[filled[bad[0]]]):#018x}, "
                              f"expected {int(exp_h[src[bad[0]]]):#018x} ({len(bad)} differ)")
    owner = ((exp_h >> np.uint64(40)) % np.uint64(parts)).astype(np.int64)
    for p in range(parts):
        for c in range(G):
            mine = np.flatnonzero(owner[c * chunk: (c + 1) * chunk] == p) + c * chunk
            a = (p * G + c) * sub_cap
            assert counts[p, c] == len(mine), f"{what}: count of sub-slab ({p}, {c})"
            assert np.array_equal(origin[a: a + len(mine)], mine.astype(np.uint32)), f"{what}: order inside sub-slab ({p}, {c})"
            assert np.all(origin[a + len(mine): a + sub_cap] == 0xFFFFFFFF), f"{what}: slots past the count of sub-slab ({p}, {c})"
    assert np.array_equal(totals[:parts], np.bincount(owner, minlength=parts)), what + ": totals"
