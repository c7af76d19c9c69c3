"""The helpers that deal records to GPUs in the multi-GPU `--unordered` run (fqd_sample_tags, fqd_classify_tags,
fqd_range_keep, fqd_max_u32, fqd_gather_seqs: csrc/fqd_join.hip; fqd_scatter_flags: csrc/fqd_engine.hip), each against
plain Python or numpy.

The rule: range of a tag = number of splitters < the tag (splitters ascending, FastqViewWithId::cmp order = Python's bytes
order for NUL-free tags), so equal tags share a range and a tag equal to a splitter lies in the range BELOW it.  Splitters
are stored as the host stores them, at a stride of 256 bytes, a longer tag cut to that."""
import bisect

import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine
from test_gpu_join import make_tags, tag_arrays, to_dev

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
STRIDE = 256
SIZES = [1, 63, 64, 65, 255, 256, 257, 600_001]             # 600 001 > 2048 blocks of 256: the grid-stride loops go round


@pytest.fixture(scope="module")
def engine():
    with Engine(segments=2) as e:
        yield e


def u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# fqd_classify_tags
LONG = bytes(range(1, 256)) + b"\x01" + b"tail-" * 40       # the long tags share its first 256 bytes; [255] is the lowest byte
CUT = LONG[:STRIDE]
HOT = b"abcdefgh"                                            # a tag of the `mixed` style, repeated below
assert len(LONG) >= 400


@pytest.fixture(scope="module")
def classify_tags_input():
    rng = np.random.default_rng(31)
    tags = make_tags(rng, 1500, "mixed") + make_tags(rng, 1500, "wide") + make_tags(rng, 300, "long")
    tags += [b"", b"\xff", b"\x01", LONG[:255], LONG[:256], LONG[:257], LONG[:400], LONG[:256] + b"\x01", LONG[:255] + b"\xff"]
    tags += [HOT] * 40 + [b""] * 3 + [CUT] * 2
    tags = [tags[i] for i in rng.permutation(len(tags))]
    assert all(0 not in t for t in tags)
    return tags


def splitter_sets(tags):
    """n_split -> ascending splitters (each at most 256 bytes)."""
    rng = np.random.default_rng(32)
    prefix = HOT[:-1]                                        # a proper prefix of an input tag, itself no tag
    longer = HOT + b"\x01"                                   # an input tag extended by one byte, itself no tag
    assert HOT in tags and prefix not in tags and longer not in tags and b"" in tags and CUT in tags
    seven = sorted([b"", prefix, HOT, HOT, longer, CUT, b"\xff"])
    drawn = [tags[i][:STRIDE] for i in rng.integers(0, len(tags), 40)]
    drawn += [bytes(rng.integers(1, 256, size=int(rng.integers(0, 12))).astype(np.uint8)) for _ in range(15)]
    many = sorted(seven + drawn + [drawn[0], b"\x01"])
    sets = {0: [], 1: [HOT], 2: [HOT, HOT], 3: sorted([b"", HOT, CUT]), 7: seven, 64: many}
    assert all(len(v) == k and v == sorted(v) and all(len(s) <= STRIDE for s in v) for k, v in sets.items())
    return sets


def upload_splitters(splitters):
    flat = np.full(max(1, len(splitters)) * STRIDE, 0xEE, dtype=np.uint8)      # what lies behind a splitter's end is not read
    for k, s in enumerate(splitters):
        flat[k * STRIDE:k * STRIDE + len(s)] = np.frombuffer(s, np.uint8)
    lens = np.array([len(s) for s in splitters] + [0], dtype=np.uint32)
    return to_dev(flat, lens)


def classify(e, tags, splitters):
    T = to_dev(*tag_arrays(tags))
    sb, sl = upload_splitters(splitters)
    out = torch.full((len(tags),), -1, dtype=torch.int32, device="cuda")
    e.classify_tags((*T, len(tags)), sb if splitters else None, STRIDE, sl if splitters else None, len(splitters), out)
    e.sync()
    return u32(out)


@pytest.mark.parametrize("n_split", [0, 1, 2, 3, 7, 64])
def test_classify_counts_the_splitters_below_the_tag(engine, classify_tags_input, n_split):
    tags = classify_tags_input
    splitters = splitter_sets(tags)[n_split]
    got = classify(engine, tags, splitters)
    exp = np.array([bisect.bisect_left(splitters, t) for t in tags], dtype=np.uint32)
    wrong = np.nonzero(got != exp)[0]
    assert wrong.size == 0, (f"{wrong.size} tags in a wrong range, the first {tags[wrong[0]]!r}: got {got[wrong[0]]}, "
                             f"expected {exp[wrong[0]]} of {splitters!r}")
    if n_split == 0:
        assert not got.any()
    # every copy of a tag that equals a splitter lies below it; the ranges never go down along the sorted tags
    for s in set(splitters):
        below = splitters.index(s)
        assert all(got[i] == below for i, t in enumerate(tags) if t == s)
    order = sorted(range(len(tags)), key=tags.__getitem__)
    assert (np.diff(got[order].astype(np.int64)) >= 0).all()
    if CUT in splitters:                                     # the long tags around the 256-byte cut
        at = splitters.index(CUT)
        side = {len(t): int(got[i]) for i, t in enumerate(tags) if t in (LONG[:255], LONG[:256], LONG[:257], LONG[:400])}
        assert side[255] <= at and side[256] == at and side[257] > at and side[400] > at
    # a second file with the same tags in another order: the same range per tag
    other = [tags[i] for i in np.random.default_rng(33).permutation(len(tags))]
    got_other = classify(engine, other, splitters)
    assert dict(zip(tags, got.tolist())) == dict(zip(other, got_other.tolist()))


# ---------------------------------------------------------------------------------------------------------------------
# fqd_sample_tags
def sample_input(n):
    """n distinct tags ("k:" and 0..400 random bytes), shorter and longer than 256 (and than 8) bytes."""
    rng = np.random.default_rng(40 + n)
    lens = rng.integers(0, 401, n)
    short = rng.random(n) < 0.2
    lens[short] = rng.integers(0, 6, int(short.sum()))
    lens[:2] = [0, 400][:n]                                  # the small cases sample records 0 and 1
    body = rng.integers(1, 256, size=int(lens.sum()) + 1, dtype=np.uint8).tobytes()
    at = np.concatenate([[0], np.cumsum(lens)])
    return [b"%d:" % k + body[at[k]:at[k + 1]] for k in range(n)]


@pytest.mark.parametrize("n,n_samples,stride", [(1, 1, 256), (5, 5, 256), (5, 3, 256), (3, 7, 256), (10_000, 4096, 256),
                                                (4097, 4096, 256), (10_000, 4096, 8)])
def test_sample_takes_every_n_over_samples_th_tag(engine, n, n_samples, stride):
    tags = sample_input(n)
    picked = [tags[k * n // n_samples] for k in range(n_samples)]
    if n > 1:
        assert min(map(len, picked)) < 8 and max(map(len, picked)) > 256
    T = to_dev(*tag_arrays(tags))
    pad = 512
    out = torch.full((n_samples * stride + pad,), 0xEE, dtype=torch.uint8, device="cuda")
    out_len = torch.full((n_samples + 16,), -1, dtype=torch.int32, device="cuda")
    engine.sample_tags((*T, n), n_samples, stride, out, out_len)
    engine.sync()
    got, got_len = out.cpu().numpy(), u32(out_len)
    exp = np.full(n_samples * stride + pad, 0xEE, dtype=np.uint8)            # untouched behind every sample and behind the last
    for k in range(n_samples):
        s = picked[k][:stride]
        exp[k * stride:k * stride + len(s)] = np.frombuffer(s, np.uint8)
        assert got_len[k] == len(s), k
    assert np.array_equal(got, exp)
    assert (got_len[n_samples:] == NONE).all()


# ---------------------------------------------------------------------------------------------------------------------
# fqd_range_keep, fqd_max_u32
@pytest.mark.parametrize("n", SIZES)
def test_range_keep_flags_and_counts_one_range(engine, n):
    rng = np.random.default_rng(50 + n)
    ranges = rng.integers(0, 6, n).astype(np.uint32)
    present = int(ranges[n // 2])
    (d_range,) = to_dev(ranges)
    for which in (present, 9, NONE):
        keep = torch.full((n + 64,), 7, dtype=torch.uint8, device="cuda")
        count = engine.range_keep(d_range, n, which, keep)
        got = keep.cpu().numpy()
        exp = (ranges == which).astype(np.uint8)
        assert np.array_equal(got[:n], exp) and (got[n:] == 7).all()
        assert count == int(exp.sum())
        assert (count > 0) == (which == present)


@pytest.mark.parametrize("n", SIZES)
def test_max_u32_is_unsigned(engine, n):
    rng = np.random.default_rng(60 + n)
    for place in (0, n - 1, n // 2):
        for top in (0xFFFFFFF0, 0x80000000, 0x7FFFFFFF, 1000):
            v = rng.integers(0, top, n, dtype=np.uint64).astype(np.uint32)   # all below top, most of them >= 2^31 when top is
            v[place] = top
            (d,) = to_dev(v)
            assert engine.max_u32(d, n) == top, (place, hex(top))
    (zeros,) = to_dev(np.zeros(n, np.uint32))
    assert engine.max_u32(zeros, n) == 0


def test_max_u32_of_nothing_is_zero(engine):
    assert engine.max_u32(None, 0) == 0


# ---------------------------------------------------------------------------------------------------------------------
# fqd_gather_seqs, fqd_scatter_flags
@pytest.mark.parametrize("n", [1, 1_100_000])               # 1 100 000 > 4096 blocks of 256
def test_gather_seqs_against_numpy(engine, n):
    rng = np.random.default_rng(70 + n)
    rows = 50_000
    off_table = rng.integers(2 ** 32, 2 ** 44, rows, dtype=np.uint64)
    len_table = rng.integers(0, 2 ** 32, rows, dtype=np.uint64).astype(np.uint32)
    idx = rng.integers(0, rows, n).astype(np.uint32)         # with repeats when n > 1
    idx[n // 2:n // 2 + 3] = idx[n // 2]
    d_idx, d_off, d_len = to_dev(idx, off_table, len_table)
    off_out = torch.full((n + 8,), -1, dtype=torch.int64, device="cuda")
    len_out = torch.full((n + 8,), -1, dtype=torch.int32, device="cuda")
    engine.gather_seqs(d_idx, n, d_off, d_len, off_out, len_out)
    engine.sync()
    got_off, got_len = off_out.cpu().numpy().view(np.uint64), u32(len_out)
    assert np.array_equal(got_off[:n], off_table[idx]) and (got_off[n:] == 2 ** 64 - 1).all()
    assert np.array_equal(got_len[:n], len_table[idx]) and (got_len[n:] == NONE).all()


def test_scatter_flags_against_numpy(engine):
    rng = np.random.default_rng(80)
    m, n = 70_000, 100_000                                   # m records in n slab slots, the others unused
    slots = np.sort(rng.permutation(n)[:m])
    origin = np.full(n, NONE, dtype=np.uint32)
    origin[slots] = rng.permutation(m).astype(np.uint32)
    flags = rng.integers(0, 2, n).astype(np.uint8)
    d_flags, d_origin = to_dev(flags, origin)
    for count in (n, n // 2):                                # the second time only the first half of the slots
        keep = torch.full((m + 64,), 7, dtype=torch.uint8, device="cuda")
        engine.scatter_flags(d_flags, d_origin, count, keep)
        engine.sync()
        exp = np.full(m + 64, 7, dtype=np.uint8)
        used = origin[:count] != NONE
        exp[origin[:count][used]] = flags[:count][used]
        assert np.array_equal(keep.cpu().numpy(), exp)
        assert (exp[:m] == 7).any() == (count < n)
