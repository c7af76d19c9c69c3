"""GPU checks of the ranged run's primitives (fqd_seq_prefix_keys, fqd_seq_plan_ranges: csrc/fqd_seq.hip) through ctypes,
against numpy: ragged lengths 0-200, sequences shorter than 8, IUPAC / lowercase bytes, a byte below '\\n' in mate 2
(reported, with the record that holds it), a stream cut into two blocks, and the plan against the brute-force plan of
tests/test_seq_ranged_core.py — the rules themselves are tested there, on the CPU."""
import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine
from test_gpu_seq import dev, spans
from test_seq_ranged_core import brute_plan

pytestmark = pytest.mark.gpu


def make_seqs(rng, n, alphabet=b"ACGTNacgtnRYKMSWBDHV"):
    alpha = np.frombuffer(alphabet, np.uint8)
    lens = rng.integers(0, 201, n)
    short = rng.random(n) < 0.2
    lens[short] = rng.integers(0, 9, int(short.sum()))
    lens[:12] = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16]
    return [rng.choice(alpha, size=int(L)).astype(np.uint8).tobytes() for L in lens]


def expected_keys(seqs):
    return np.array([int.from_bytes((s + b"\n" * 8)[:8], "big") for s in seqs], dtype=np.uint64)


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


def test_prefix_keys_ragged_two_mates_and_sizes():
    rng = np.random.default_rng(5)
    n = 50_000
    m1, m2 = make_seqs(rng, n), make_seqs(rng, n)
    d1, o1, l1 = (dev(x) for x in spans(m1))
    d2, o2, l2 = (dev(x) for x in spans(m2))
    s1 = rng.integers(1, 700, n).astype(np.uint32); s2 = rng.integers(1, 700, n).astype(np.uint32)
    s1[0] = s2[0] = 2 ** 32 - 1                                       # saturates
    key = torch.zeros(n, dtype=torch.int64, device="cuda")
    by = torch.zeros(n, dtype=torch.int32, device="cuda")
    with Engine(segments=2) as e:
        info = e.seq_prefix_keys((d1, o1, l1, n), key, mate2=(d2, o2, l2, n), size1=dev(s1), size2=dev(s2), bytes_=by)
        assert np.array_equal(host_u64(key), expected_keys(m1))
        exp_bytes = np.minimum(s1.astype(np.uint64) + s2, 2 ** 32 - 1)
        assert np.array_equal(by.cpu().numpy().view(np.uint32), exp_bytes.astype(np.uint32))
        assert info.record_bytes == int(s1.astype(np.uint64).sum() + s2.astype(np.uint64).sum())
        assert list(info.longest) == [max(map(len, m1)), max(map(len, m2))]
        assert info.bad_byte == -1 and all(v == 2 ** 64 - 1 for v in info.first_with)
        # the mates of a pair in blocks of their own: the second call adds to the first one's bytes, no key
        by2 = torch.zeros(n, dtype=torch.int32, device="cuda")
        e.seq_prefix_keys((d1, o1, l1, n), key, size1=dev(s1), bytes_=by2)
        info2 = e.seq_prefix_keys((d2, o2, l2, n), None, size1=dev(s2), bytes_=by2, accumulate=True)
        assert np.array_equal(by2.cpu().numpy().view(np.uint32), exp_bytes.astype(np.uint32))
        assert info2.longest[0] == max(map(len, m2))


def test_low_bytes_are_reported_with_their_first_record():
    rng = np.random.default_rng(6)
    n = 20_000
    m1, m2 = make_seqs(rng, n, b"ACGT"), make_seqs(rng, n, b"ACGT")
    plant = {}                                                       # byte -> first record
    for rec, c, mate, pos in [(17_000, 0, 1, -1), (15_000, 9, 1, 0), (16_000, 9, 0, 3), (9_000, 3, 1, 70), (19_999, 3, 0, 199)]:
        tgt = m2 if mate else m1
        s = bytearray(tgt[rec] if len(tgt[rec]) > max(pos, 0) else b"A" * 200)
        s[pos] = c
        tgt[rec] = bytes(s)
        plant[c] = min(plant.get(c, n), rec)
    d1, o1, l1 = (dev(x) for x in spans(m1))
    d2, o2, l2 = (dev(x) for x in spans(m2))
    key = torch.zeros(n, dtype=torch.int64, device="cuda")
    with Engine(segments=2) as e:
        info = e.seq_prefix_keys((d1, o1, l1, n), key, mate2=(d2, o2, l2, n))
        assert info.bad_byte == 0                                    # the lowest value, as the census of fqd_sort_seqs reports it
        for c in range(10):
            assert info.first_with[c] == plant.get(c, 2 ** 64 - 1)
        assert np.array_equal(host_u64(key), expected_keys(m1))     # keys are what the bytes are, low or not
        # mate 1 alone: only its own bytes
        only1 = e.seq_prefix_keys((d1, o1, l1, n), key)
        assert only1.bad_byte == 3 and only1.first_with[3] == 19_999 and only1.first_with[9] == 16_000 and only1.first_with[0] == 2 ** 64 - 1


def test_keys_and_plan_over_two_blocks():
    """A stream cut in mid-stream: the keys and sizes of two uploaded blocks land one behind the other, the plan over
    both is the brute-force plan, range_of is in input order."""
    rng = np.random.default_rng(7)
    n, cut = 60_000, 23_457
    pool = make_seqs(rng, 3_000, b"ACGTN")
    seqs = [pool[i] for i in rng.integers(0, len(pool), n)]
    sizes = np.array([2 * len(s) + 12 for s in seqs], dtype=np.uint32)
    key = torch.zeros(n, dtype=torch.int64, device="cuda")
    by = torch.zeros(n, dtype=torch.int32, device="cuda")
    range_of = torch.zeros(n, dtype=torch.int32, device="cuda")
    with Engine(segments=1) as e:
        for a, b in ((0, cut), (cut, n)):
            d, o, l = (dev(x) for x in spans(seqs[a:b]))
            e.seq_prefix_keys((d, o, l, b - a), key[a:], size1=dev(sizes[a:b]), bytes_=by[a:])
        keys = expected_keys(seqs)
        assert np.array_equal(host_u64(key), keys)
        pairs = list(zip(keys.tolist(), sizes.tolist()))
        total = int(sizes.sum())
        for target in (total // 4, total // 37, 1, total, 5_000):
            exp_rows, exp_range_of = brute_plan(pairs, target)
            R, rows = e.seq_plan_ranges(key, by, n, target, range_of, max_ranges=8192)
            assert R == len(exp_rows) and rows == exp_rows
            assert np.array_equal(range_of.cpu().numpy().view(np.uint32), np.array(exp_range_of, dtype=np.uint32))
        # mate 1's share of every range's bytes (what the first file's store has to hold), summed in LDS and, beyond 2048 ranges, in HBM
        share = (sizes // 3).astype(np.uint32)
        for target in (total // 4, 1):
            exp_rows, exp_range_of = brute_plan(pairs, target)
            R, rows, mate1 = e.seq_plan_ranges(key, by, n, target, range_of, max_ranges=8192, bytes_mate1=dev(share))
            assert rows == exp_rows
            assert mate1 == np.bincount(np.array(exp_range_of), weights=share.astype(np.float64), minlength=R).astype(np.uint64).tolist()
        # a table that is too small: the count is still the true one, the rows the first ones
        exp_rows, _ = brute_plan(pairs, 5_000)
        R, rows = e.seq_plan_ranges(key, by, n, 5_000, range_of, max_ranges=3)
        assert R == len(exp_rows) > 3 and rows == exp_rows[:3]


def test_plan_one_hot_key_and_large_bytes():
    """One key value far beyond the target among small ones, sizes near 2^32 (the scan is 64 bits wide)."""
    rng = np.random.default_rng(8)
    n = 300_000
    keys = rng.integers(0, 2 ** 63, n).astype(np.uint64) << np.uint64(1)
    keys[rng.random(n) < 0.4] = np.uint64(0x4141414141414141)
    sizes = rng.integers(1, 2 ** 32, n).astype(np.uint32)
    pairs = list(zip(keys.tolist(), sizes.tolist()))
    range_of = torch.zeros(n, dtype=torch.int32, device="cuda")
    with Engine(segments=1) as e:
        target = int(sizes.astype(np.uint64).sum()) // 10
        exp_rows, exp_range_of = brute_plan(pairs, target)
        R, rows = e.seq_plan_ranges(dev(keys), dev(sizes), n, target, range_of)
        assert rows == exp_rows and R == len(exp_rows)
        assert any(lo == hi == 0x4141414141414141 and b > target for lo, hi, _, b in rows)
        assert np.array_equal(range_of.cpu().numpy().view(np.uint32), np.array(exp_range_of, dtype=np.uint32))


def test_a_plan_of_too_many_ranges_is_refused():
    """A target that cuts the input into more than FQD_SEQ_MAX_RANGES (65536) ranges ends the one-lane walk there."""
    from fastq_dupaway_amd._lib import FqdError
    n = 70_000
    keys = (np.arange(n, dtype=np.uint64) * np.uint64(977)) + np.uint64(0x4141414141410000)
    sizes = np.full(n, 300, np.uint32)
    range_of = torch.zeros(n, dtype=torch.int32, device="cuda")
    with Engine(segments=1) as e:
        with pytest.raises(FqdError, match="more than 65536 ranges"):
            e.seq_plan_ranges(dev(keys), dev(sizes), n, 1, range_of)
        R, rows = e.seq_plan_ranges(dev(keys), dev(sizes), n, 600, range_of, max_ranges=40_000)
        assert R == n // 2 and all(p == 2 and b == 600 for _, _, p, b in rows)
