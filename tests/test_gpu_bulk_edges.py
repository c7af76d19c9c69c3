"""The bulk insert (launch_bulk_insert in csrc/fqd_engine.hip: bulk_hist1 / scan256 / scatter<1> / hist2 / scan_buckets /
scatter<2>, bucket_dedup_kernel<FRESH, RAGGED, VL>, heavy_bucket_insert_kernel) at its structural edges, with inputs
PLACED by the restated hash (tests/bulk_placement.py) and held against first occurrence over the read bytes.

Every case (run()): an Engine(profile=True) under FQD_BULK_MIN=0; batch 1 = the crafted population, shuffled; batch 2 = every
distinct key of batch 1 once more, fresh keys aimed at a bucket batch 1 left empty, and repeats up to the size at which a
batch takes the bulk path against a filled table (n * 12 >= slots).  Asserted: the flags of both batches, the duplicate
count, the table's size against the restated sizing, the profile's launch counts (partition and dedup rose, the atomic
insert's did not), and — from the restated hashes, before anything is submitted — that the population has the shape the
case is named for.  Nothing is compared with a tolerance.

  a. partition tiles (8192 records) and level-1 digits with 0 / 1 / 8192 / 8193 records, the last digit empty or not;
  b. every geometry: 2^16 slots at 12 / 13 / 14 segment bits, 2^22 (bits2 5 and 4), 2^29 (bits2 8 and the nine-bit digit);
  c. a bucket of 4608 / 4609 / 9217 records (dedup chunks) and of D + 1535 / 1536 / 1537 (the candidate queue), for the
     verify templates VL 4, VL 8, VL 0 and ragged;
  d. the retry side of the queue, under the weak hash;
  e. a bucket exactly at FQD_HEAVY_ABOVE and one above it, in a FRESH launch;
  f. a segment filled to its last slot, and one key more;
  g. FQD_DEDUP_THREADS 64 / 1024, FQD_PART_BLOCKS_PER_CU 1, a final batch 2, submit_linked.
"""
import zlib

import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, Reads
from fastq_dupaway_amd._lib import FqdError
import bulk_placement as bp

pytestmark = pytest.mark.gpu
UNWRITTEN = 0xFFFFFFFF
LAUNCHES = ("partition_launches", "dedup_launches", "insert_launches")

_POOLS = {}


def pool_of(lengths, n, weak=False):
    key = (tuple(lengths), n, weak)
    if key not in _POOLS:
        _POOLS[key] = bp.Pool(zlib.crc32(repr(key).encode()), n, list(lengths), weak=weak)
    return _POOLS[key]


def pool32():
    return pool_of([(32,)], 400_000)


SHAPES = {"se32": [(32,)], "se150_vl4": [(150,)], "pe150_vl8": [(150, 150)], "se75_vl0": [(75,)],
          "ragged149_151": [(149,), (150,), (151,)]}


def pool_shape(shape):
    return pool32() if shape == "se32" else pool_of(SHAPES[shape], 60_000)


@pytest.fixture(autouse=True)
def bulk_for_every_batch(monkeypatch):
    monkeypatch.setenv("FQD_BULK_MIN", "0")                  # read when an engine is created
    for name in ("FQD_SEG_BITS", "FQD_HEAVY_ABOVE", "FQD_DEDUP_THREADS", "FQD_PART_BLOCKS_PER_CU", "FQD_CHUNK_READS", "FQD_DEDUP_VL"):
        monkeypatch.delenv(name, raising=False)


def host_reads(pool, idx):
    out = []
    for m in range(pool.S):
        w = pool.width[m]
        flat = np.concatenate([pool.mates[m][idx].reshape(-1), np.zeros(64, np.uint8)])
        if pool.uniform:
            out.append(Reads(flat, uniform_len=w, uniform_stride=w))
        else:
            out.append(Reads(flat, offsets=np.arange(len(idx), dtype=np.uint64) * np.uint64(w),
                             lengths=np.ascontiguousarray(pool.lens[m][idx], dtype=np.uint32)))
    return out


def device_reads(pool, idx):
    out = []
    for r in host_reads(pool, idx):
        out.append(Reads(torch.from_numpy(r.bases).cuda(),
                         None if r.offsets is None else torch.from_numpy(r.offsets.view(np.int64)).cuda(),
                         None if r.lengths is None else torch.from_numpy(r.lengths.view(np.int32)).cuda(),
                         r.uniform_len, r.uniform_stride))
    return out


def run(monkeypatch, pool, batches, slots, seg_bits=13, capacity=0, final_last=False, linked=False, bulk=None, big=False):
    """Submits the batches (pool indices) to one engine and asserts everything the module's docstring lists; bulk: which
    batches take the bulk path (default: all).  Returns the flags."""
    monkeypatch.setenv("FQD_SEG_BITS", str(seg_bits))        # read when a table is made
    ref = bp.first_occurrence(pool, np.concatenate(batches))
    size = bp.TableSize(capacity)
    try:
        e = Engine(segments=pool.S, capacity_reads=capacity, profile=True, weak_hash=pool.weak)
    except FqdError as err:
        if big and "hipMalloc(&nt" in str(err) and "out of memory" in str(err):      # ensure_table's allocation of the table itself
            pytest.skip(f"no room for a table of {slots} slots on this device: {err}")
        raise
    flags, links, done = [], [], 0
    with e:
        for k, idx in enumerate(batches):
            n = len(idx)
            assert size.after(done + n) == slots, "the case must keep its table at the size it is named for"
            want_bulk = True if bulk is None else bulk[k]
            assert bp.bulk_applies(n, done, slots) == want_bulk
            before = e.profile()
            last = final_last and k == len(batches) - 1
            if linked:
                keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
                link = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                e.submit_linked(device_reads(pool, idx), n, keep, link, last=last)
                e.sync()
                flags.append(keep.cpu().numpy()); links.append(link.cpu().numpy().view(np.uint32))
            else:
                flags.append(e.submit(host_reads(pool, idx), n, final=last))
            after = e.profile()
            rose = tuple(after[f] - before[f] for f in LAUNCHES)
            assert rose == ((1, 1, 0) if want_bulk else (0, 0, 1)), f"batch {k}: (partition, dedup, insert) launches rose by {rose}"
            st = e.stats()
            assert st["table_slots"] == slots and st["records"] == done + n
            done += n
        e.sync()
        assert e.stats()["duplicates"] == ref.duplicates
    keep = np.concatenate(flags)
    wrong = np.flatnonzero(keep != ref.keep)
    assert len(wrong) == 0, (f"{len(wrong)} flags differ from first occurrence (batches end at {np.cumsum([len(b) for b in batches]).tolist()}); "
                             f"first at {wrong[:8].tolist()}: got {keep[wrong[:8]].tolist()}")
    if linked:
        link = np.concatenate(links)
        assert np.all(link[keep == 1] == UNWRITTEN)
        assert ref.links_hold(keep, link)
        for i in np.flatnonzero(keep == 0)[:: max(1, int((keep == 0).sum()) // 50)]:       # the same, spelled out on a sample
            assert int(link[i]) in ref.earlier(int(i))
    return keep


def second_batch(pick, batch1, empty_bucket, rng, n_fresh=40, fresh_also=None):
    """Every distinct key of batch 1 once, n_fresh fresh keys of the bucket batch 1 left empty (fresh_also: and of that
    bucket), repeats up to the bulk path's size — or, where batch 1 is too small to be repeated that often, more fresh keys."""
    at, slots = pick.at, pick.geom.slots
    assert not np.any(at.bucket[batch1] == empty_bucket)
    distinct = np.unique(batch1)
    parts = [distinct, pick.take(empty_bucket, n_fresh, distinct_tags=not pick.pool.weak)]
    if fresh_also is not None:
        parts.append(pick.take(fresh_also, n_fresh, distinct_tags=not pick.pool.weak))
    short = -(-slots // bp.BULK_RATIO) - sum(len(p) for p in parts)
    if short > 0:
        parts.append(distinct[np.arange(short) % len(distinct)] if len(distinct) >= 100 else pick.take_outside(set(), short))
    b2 = np.concatenate(parts)
    rng.shuffle(b2)
    return b2


def cyc(keys, count):
    """count records over the given keys, every key at least count // len(keys) times."""
    return keys[np.arange(count) % len(keys)]


# ---- a. partition tiles and level-1 digits ---------------------------------------------------------------------------------
A_SLOTS, A_HINT = 1 << 22, 1 << 21                           # 13 segment bits: bits1 = 5, bits2 = 4


@pytest.mark.parametrize("n", [1, 8191, 8192, 8193])
def test_batch_of_whole_and_broken_tiles(monkeypatch, n):
    """Level 1 cuts the batch into ceil(n / 8192) tiles: one record, one short of a tile, a whole tile, a tile and one record."""
    pool, rng = pool32(), np.random.default_rng(n)
    pick = bp.Picker(pool, bp.geometry(A_SLOTS, 13))
    assert (pick.geom.bits1, pick.geom.bits2) == (5, 4)
    empty = 77
    b1 = pick.take_outside({empty}, n)
    rng.shuffle(b1)
    b2 = second_batch(pick, b1, empty, rng)
    assert len(b2) >= 349_526
    run(monkeypatch, pool, [b1, b2], A_SLOTS, capacity=A_HINT)


def digits_population(pick, counts, background, rng, distinct_at_most):
    """Batch 1 with exactly counts[d] records in level-1 digit d (over at most distinct_at_most keys each) and `background`
    in every digit not named."""
    g, at = pick.geom, pick.at
    parts = []
    for d in range(1 << g.bits1):
        c = counts.get(d, background)
        if c:
            parts.append(cyc(pick.take(None, min(c, distinct_at_most), digit1=d), c))
    b1 = np.concatenate(parts)
    rng.shuffle(b1)
    got = np.bincount(at.digit1[b1], minlength=1 << g.bits1)
    for d, c in counts.items():
        assert got[d] == c
    return b1, got


@pytest.mark.parametrize("last_digit_empty", [True, False])
def test_digits_of_0_1_8192_8193_records(monkeypatch, last_digit_empty):
    """Level-2 tiles are cut per level-1 digit as ceil(count / 8192): digits with no tile, one record, one full tile, and a
    full tile plus a tile of one record, in one batch; the last digit without a tile, or with two."""
    pool, rng = pool32(), np.random.default_rng(3)
    pick = bp.Picker(pool, bp.geometry(A_SLOTS, 13))
    counts = {31: 0, 30: 1, 3: 8192, 4: 8193} if last_digit_empty else {0: 0, 1: 1, 30: 8192, 31: 8193}
    b1, got = digits_population(pick, counts, 50, rng, 3000)
    assert (got[31] == 0) == last_digit_empty and sorted(set(got.tolist())) == [0, 1, 50, 8192, 8193]
    empty = (31 if last_digit_empty else 0) << pick.geom.bits2          # a bucket of the digit that got nothing
    run(monkeypatch, pool, [b1, second_batch(pick, b1, empty, rng)], A_SLOTS, capacity=A_HINT)


def test_digits_of_0_1_8192_8193_records_single_level(monkeypatch):
    """The same at 2^21 slots: bits1 = 8, bits2 = 0, the largest table partitioned in one pass; a digit is a bucket, so the
    buckets of 8192 and 8193 records also run two dedup chunks — and batch 2, which repeats their 1000 keys some 39 times, makes
    them heavy (more than 4 << 13 records) in a launch that is not FRESH."""
    pool, rng = pool32(), np.random.default_rng(4)
    pick = bp.Picker(pool, bp.geometry(1 << 21, 13))
    assert (pick.geom.bits1, pick.geom.bits2) == (8, 0)
    b1, got = digits_population(pick, {0: 0, 1: 1, 254: 8192, 255: 8193}, 10, rng, 1000)
    assert got[255] == 8193 and got[0] == 0
    b2 = second_batch(pick, b1, 0, rng)
    assert len(b2) >= 174_763
    run(monkeypatch, pool, [b1, b2], 1 << 21, capacity=1 << 20)


# ---- b. the geometry sweep ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,seg_bits,bits2", [(16, 12, 0), (16, 13, 0), (16, 14, 0), (22, 12, 5), (22, 13, 4), (29, 13, 8), (29, 12, 9)])
def test_geometry_sweep(monkeypatch, t, seg_bits, bits2):
    """Random reads, about 30 % copies, through every partition geometry.  2^16: all three segment widths (14 bits: 143 KB of
    LDS, one workgroup per CU).  2^29 slots: the widest digit2 byte plane (bits2 = 8) and the nine-bit level-2 digit, which
    bulk_hist2_kernel<true> reads out of the records.  At 2^16 and 2^22 a second batch runs the launch that is not FRESH; at
    2^29 that batch would have to hold 2^29 / 12 = 44.7 M reads, so the fresh batch is all these two cases run."""
    pool, rng = pool32(), np.random.default_rng(t * 100 + seg_bits)
    slots = 1 << t
    g = bp.geometry(slots, seg_bits)
    assert (g.seg_bits, g.bits2) == (seg_bits, bits2)
    at = bp.place(pool.hash, g)
    n1, d1 = (14_000, 9_800) if t == 16 else (200_000, 140_000)
    keys = rng.permutation(pool.n)[:d1]
    b1 = np.concatenate([keys, keys[rng.integers(0, d1, n1 - d1)]])
    rng.shuffle(b1)
    batches = [b1]
    if t < 29:
        rest = np.setdiff1d(np.arange(pool.n), keys)
        fresh = rest[: 1000 if t == 16 else 100_000]
        b2 = np.concatenate([keys, fresh])
        short = -(-slots // bp.BULK_RATIO) - len(b2)
        if short > 0:
            b2 = np.concatenate([b2, cyc(keys, short)])
        rng.shuffle(b2)
        batches.append(b2)
    else:
        assert len(np.unique(at.digit1[b1])) == 256                       # every level-1 digit has tiles
        assert int((at.bucket[b1] & ((1 << bits2) - 1)).max()) >> (bits2 - 1) == 1      # the level-2 digit's top bit is in use
    run(monkeypatch, pool, batches, slots, seg_bits=seg_bits, capacity=slots >> 1, big=t == 29)


# ---- c. dedup chunks and the candidate queue -------------------------------------------------------------------------------
C_SLOTS = 1 << 16
TARGET, EMPTY = 2, 5


def target_population(pick, R, keys, rng, background=40, twice=False):
    """Batch 1: R records over `keys` in bucket TARGET, a little background elsewhere, nothing in bucket EMPTY."""
    g, at, weak = pick.geom, pick.at, pick.pool.weak
    parts = [np.concatenate([keys, keys]) if twice else cyc(keys, R)]
    for b in range(g.n_buckets):
        if b not in (TARGET, EMPTY):
            parts.append(pick.take(b, background, distinct_tags=not weak))
    b1 = np.concatenate(parts)
    rng.shuffle(b1)
    counts = np.bincount(at.bucket[b1], minlength=g.n_buckets)
    inside = b1[at.bucket[b1] == TARGET]
    assert counts[TARGET] == R == len(inside) and counts[EMPTY] == 0 and len(np.unique(inside)) == len(keys)
    assert np.all(np.delete(counts, [TARGET, EMPTY]) == background)
    if not weak:
        assert len(np.unique(at.tag[keys])) == len(keys)             # a tag match in this bucket is an equal key
    return b1


# (R, D, what it reaches); rows of D = 4608 need a 2^13-slot segment
C_ROWS_13 = [(4608, 4608), (4609, 4608), (4609, 4609), (2535, 1000), (2536, 1000), (2537, 1000), (9217, 200)]
# a 2^12-slot segment cannot hold 4608 keys: its bucket of 4609 records (a second chunk of one record) has 3000
C_ROWS_12 = [(4609, 3000), (2535, 1000), (2536, 1000), (2537, 1000), (9217, 200)]


def chunk_case(monkeypatch, shape, seg_bits, R, D, **variant):
    pool, rng = pool_shape(shape), np.random.default_rng(R * 7 + D + seg_bits)
    pick = bp.Picker(pool, bp.geometry(C_SLOTS, seg_bits))
    assert D <= pick.geom.seg_slots
    keys = pick.take(TARGET, D)
    b1 = target_population(pick, R, keys, rng)
    # what the case is named for: chunks of 4608 records, and candidates (records - keys, as all tags differ) against the queue's 1536
    chunks = -(-R // bp.DEDUP_RECORDS)
    if (R, D) == (4608, 4608):
        assert chunks == 1 and R - D == 0
    elif R == 4609:
        assert chunks == 2 and R - (chunks - 1) * bp.DEDUP_RECORDS == 1
    elif D == 1000:
        assert chunks == 1 and R - D in (bp.DEDUP_QUEUE - 1, bp.DEDUP_QUEUE, bp.DEDUP_QUEUE + 1)
    else:
        assert chunks == 3 and R - 2 * bp.DEDUP_RECORDS == 1 and bp.DEDUP_RECORDS - D >= 4408 > bp.DEDUP_QUEUE
        assert np.bincount(b1)[keys].min() >= 2                       # so the last chunk's single record is a copy, whichever it is
    b2 = second_batch(pick, b1, EMPTY, rng)
    total = len(b1) + len(b2)
    assert total <= 32768
    return run(monkeypatch, pool, [b1, b2], C_SLOTS, seg_bits=seg_bits, capacity=0 if total <= 16384 else 1 << 15, **variant)


@pytest.mark.parametrize("seg_bits,R,D", [(13, r, d) for r, d in C_ROWS_13] + [(12, r, d) for r, d in C_ROWS_12])
def test_chunks_and_candidate_queue(monkeypatch, seg_bits, R, D):
    """32-base reads.  4608 = 4608 keys: exactly one chunk, no candidate.  4609: a second chunk of one record (the early
    loads v0 belong to the first chunk only).  1000 keys + 1535 / 1536 / 1537 copies: the queue's last entry, a full
    queue, and the first record settled inside walk.  9217 over 200 keys: three chunks, at least 4408 candidates in each
    full one however the scatter ordered the bucket, and a last chunk of one copy."""
    chunk_case(monkeypatch, "se32", seg_bits, R, D)


@pytest.mark.parametrize("shape", ["se150_vl4", "pe150_vl8", "se75_vl0", "ragged149_151"])
@pytest.mark.parametrize("seg_bits,R,D", [(13, r, d) for r, d in C_ROWS_13[1:2] + C_ROWS_13[3:]] + [(12, r, d) for r, d in C_ROWS_12])
def test_chunks_and_candidate_queue_per_verify_template(monkeypatch, shape, seg_bits, R, D):
    """The same buckets for every template of the verify phase: 150 bases (8 key words, VL 4), 2 x 150 (16 words, VL 8),
    75 bases (5 words — odd — VL 0) and a ragged key store (149 / 150 / 151 bases mixed)."""
    chunk_case(monkeypatch, shape, seg_bits, R, D)


# ---- d. the retry side of the queue: weak hash ------------------------------------------------------------------------------
def weak_case(monkeypatch, D, twice, **variant):
    pool, rng = pool_of([(32,)], 100_000, weak=True), np.random.default_rng(D + twice)
    pick = bp.Picker(pool, bp.geometry(C_SLOTS, 13))
    at = pick.at
    assert np.all(at.tag == 0) and np.all(at.start % 64 == 0)
    keys = pick.take(TARGET, D, distinct_tags=False)
    R = 2 * D if twice else D
    b1 = target_population(pick, R, keys, rng, twice=twice)
    # one record per start slot claims it unopposed; every other record of the bucket meets an occupied slot, whose tag (0) is its own
    starts = len(np.unique(at.start[keys]))
    assert starts <= 1 << (13 - 6)
    candidates = R - starts
    queued = min(candidates, bp.DEDUP_QUEUE)
    # a queued candidate is retried unless it is a copy of the slot's owner: none is (once each), at most one per start slot (twice)
    retries_at_least, retries_at_most = queued - (starts if twice else 0), queued
    regime = {(600, False): "fit", (1100, False): "reach", (1700, False): "no room",
              (600, True): "reach", (1100, True): "no room", (1700, True): "no room"}[(D, twice)]
    if regime == "fit":
        assert candidates + retries_at_most <= bp.DEDUP_QUEUE         # every retry finds room behind the candidates
    elif regime == "reach":
        assert candidates < bp.DEDUP_QUEUE < candidates + retries_at_least      # the retries reach the candidates: the rest walk inline
    else:
        assert candidates >= bp.DEDUP_QUEUE                            # the candidates fill the queue (the rest settle in walk): no retry finds room
    return run(monkeypatch, pool, [b1, second_batch(pick, b1, EMPTY, rng)], C_SLOTS, **variant)


@pytest.mark.parametrize("twice", [False, True])
@pytest.mark.parametrize("D", [600, 1100, 1700])
def test_retries_under_the_weak_hash(monkeypatch, D, twice):
    """No tag and start slots that are multiples of 64: every occupied slot a record walks over is a tag match, so all but
    at most 128 records of the bucket are candidates and nearly all candidates are retried.  Once each: 600 keys' retries fit
    behind the candidates, 1100 keys' reach them, 1700 keys leave no room; twice each: 600 keys' reach them, 1100 and 1700 leave
    no room (weak_case asserts the regime from the start slots)."""
    weak_case(monkeypatch, D, twice)


# ---- e. the heavy-bucket threshold -------------------------------------------------------------------------------------------
def test_heavy_threshold_in_a_fresh_launch(monkeypatch):
    """hi - lo > heavy_above: a bucket of exactly FQD_HEAVY_ABOVE records stays with the LDS kernel, one of a record more
    goes to heavy_bucket_insert_kernel — in a FRESH launch, so the dedup kernel must clear that segment in global memory
    before the atomic path fills it.  Batch 2 then finds every key of the heavy bucket and keeps fresh keys aimed at it."""
    monkeypatch.setenv("FQD_HEAVY_ABOVE", "3000")            # read per call
    pool, rng = pool32(), np.random.default_rng(8)
    pick = bp.Picker(pool, bp.geometry(C_SLOTS, 13))
    at, at_limit, heavy = pick.at, 1, 6
    parts = [cyc(pick.take(at_limit, 2000), 3000), cyc(pick.take(heavy, 2000), 3001)]
    for b in (0, 2, 3, 4, 7):
        parts.append(pick.take(b, 40))
    b1 = np.concatenate(parts)
    rng.shuffle(b1)
    counts = np.bincount(at.bucket[b1], minlength=8)
    assert counts[at_limit] == 3000 and counts[heavy] == 3001 and counts[EMPTY] == 0
    b2 = second_batch(pick, b1, EMPTY, rng, fresh_also=heavy)
    c2 = np.bincount(at.bucket[b2], minlength=8)
    assert c2.max() <= 3000 and c2[heavy] >= 2040             # batch 2 reads the heavy bucket's segment in the LDS kernel
    run(monkeypatch, pool, [b1, b2], C_SLOTS)


# ---- f. a full segment ---------------------------------------------------------------------------------------------------------
def test_segment_filled_to_its_last_slot(monkeypatch):
    """2^12 distinct keys in one 2^12-slot segment: every probe run wraps, nothing is lost.  64 of them again (the atomic
    path, 64 * 12 < slots), then all of them again on the bulk path, which walks the full segment in LDS."""
    pool, rng = pool32(), np.random.default_rng(9)
    pick = bp.Picker(pool, bp.geometry(C_SLOTS, 12))
    keys = pick.take(TARGET, 4096)
    b1 = target_population(pick, 4096, keys, rng)
    b2 = keys[rng.permutation(4096)[:64]]
    b3 = second_batch(pick, b1, EMPTY, rng)
    keep = run(monkeypatch, pool, [b1, b2, b3], C_SLOTS, seg_bits=12, bulk=[True, False, True])
    assert keep[:len(b1)].all() and not keep[len(b1):len(b1) + 64].any()


def test_one_key_more_than_a_segment_holds(monkeypatch):
    """4097 distinct keys in one 2^12-slot segment: the last one walks all 4096 slots (walk's loop is bounded by the
    segment) and is counted; the call ends with the overflow error, not with flags."""
    monkeypatch.setenv("FQD_SEG_BITS", "12")
    pool, rng = pool32(), np.random.default_rng(10)
    pick = bp.Picker(pool, bp.geometry(C_SLOTS, 12))
    b1 = target_population(pick, 4097, pick.take(TARGET, 4097), rng)
    e = Engine(profile=True)
    try:
        with pytest.raises(FqdError, match="hash set overflowed its table"):
            e.submit(host_reads(pool, b1), len(b1))
        assert e.stats()["table_slots"] == C_SLOTS
        prof = e.profile()                                    # the overflow is the bulk path's: no atomic insert ran
        assert tuple(prof[f] for f in LAUNCHES) == (1, 1, 0)
    finally:
        e.close()


# ---- g. launch shapes, the final batch, links ----------------------------------------------------------------------------------
VARIANTS = {"dedup_threads_64": {"FQD_DEDUP_THREADS": "64"}, "dedup_threads_1024": {"FQD_DEDUP_THREADS": "1024"},
            "part_blocks_per_cu_1": {"FQD_PART_BLOCKS_PER_CU": "1"}, "final_batch_2": {"final_last": True}, "linked": {"linked": True}}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", ["second_chunk_of_one", "three_chunks_full_queue", "weak_1100"])
def test_variants(monkeypatch, case, variant):
    """FQD_DEDUP_THREADS changes every stride of the dedup kernel (64: one wave, twelve probe rounds per chunk; 1024: the early
    loads cover the whole chunk); a final batch 2 leaves its segments in LDS; submit_linked names, for every dropped record,
    an earlier record of the same key.  FQD_PART_BLOCKS_PER_CU=1 only has to be harmless here: these batches are one or two
    tiles, far below any cap on the partition grids; test_partition_blocks_stride_over_tiles makes the cap bind."""
    args = {}
    for name, value in VARIANTS[variant].items():
        if name.startswith("FQD_"):
            monkeypatch.setenv(name, value)                    # both are read per call
        else:
            args[name] = value
    if case == "second_chunk_of_one":
        chunk_case(monkeypatch, "se32", 13, 4609, 4608, **args)
    elif case == "three_chunks_full_queue":
        chunk_case(monkeypatch, "se32", 13, 9217, 200, **args)
    else:
        weak_case(monkeypatch, 1100, False, **args)


def test_partition_blocks_stride_over_tiles(monkeypatch):
    """FQD_PART_BLOCKS_PER_CU=1 caps the partition grids at one workgroup per CU; a fresh batch of more than n_cu tiles, at a
    two-level geometry, makes blocks of bulk_hist1 / scatter<1> / scatter<2> take a second tile (hist2's grid is 2 per CU
    whatever the variable says).  One fresh batch: a second one on the bulk path would add nothing to the strides."""
    monkeypatch.setenv("FQD_PART_BLOCKS_PER_CU", "1")        # read per call
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    pool, rng = pool32(), np.random.default_rng(12)
    slots, hint = 1 << 23, 1 << 22
    g = bp.geometry(slots, 13)
    assert (g.bits1, g.bits2) == (5, 5)
    n = (n_cu + 5) * bp.PART_TILE + 1
    assert n <= hint
    b1 = cyc(rng.permutation(pool.n), n)
    rng.shuffle(b1)
    tiles1 = -(-n // bp.PART_TILE)
    per_digit = np.bincount(bp.place(pool.hash, g).digit1[b1], minlength=1 << g.bits1)
    tiles2 = int((-(-per_digit // bp.PART_TILE)).sum())
    assert tiles1 > n_cu and tiles2 > n_cu                    # the cap of n_cu * 1 blocks binds at both levels
    run(monkeypatch, pool, [b1], slots, capacity=hint)
