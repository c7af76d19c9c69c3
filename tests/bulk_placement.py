"""Inputs for the bulk insert chosen by WHERE they land in the table, and the reference they are held against.  CPU only.

  * the table geometry of csrc/fqd_table_geometry.hpp restated in plain Python (tests/test_table_geometry.py holds it
    against the header's own numbers) and the engine's sizing history (TableSize);
  * Pool: random distinct reads (single-end, paired, or of mixed lengths) with their placement hashes, from
    key_layout.words_of_rows / hashes_of_rows — strong hash or weak (key_layout.weak);
  * Placement: every pool read's table position, bucket, level-1 digit, start slot and tag in one geometry;
  * take(): "D reads of bucket b with pairwise different tags" — then a tag match inside that bucket means an equal key,
    and a fresh single-chunk bucket of R records over D such keys queues exactly R - D candidates;
  * first_occurrence(): the reference — first occurrence wins over the READ BYTES (np.unique over the rows); it never
    sees a hash.
"""
from dataclasses import dataclass

import numpy as np

import key_layout as kl

# ---- csrc/fqd_table_geometry.hpp, restated ---------------------------------------------------------------------------
MIN_SLOTS = 1 << 16
PART_TILE = 8192            # records per partition tile (kPartTile)
DEDUP_RECORDS = 4608        # records per chunk of bucket_dedup_kernel (kDedupRecords)
DEDUP_QUEUE = 1536          # entries of its candidate / retry queue (kDedupChunk)
BULK_RATIO = 12             # a batch takes the bulk path against a filled table when n * 12 >= slots


def pow2_at_least(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def log2_ceil(slots):
    return max(0, (slots - 1).bit_length())


def seg_bits_for(slots, want=13):
    t = log2_ceil(slots)
    if t <= 12:
        return t
    return min(14, max(want, t - 17 if t >= 17 else 12))


def table_digits(t, seg_bits):
    nb_bits = t - seg_bits if t > seg_bits else 0
    bits1 = nb_bits if nb_bits <= 8 else min(8, (nb_bits + 1) // 2)
    return bits1, nb_bits - bits1


def tag_mask_for(slots, seg_bits):
    _, bits2 = table_digits(log2_ceil(slots), seg_bits)
    tag_bits = 32 - min(seg_bits, 14) - min(bits2, 9)
    return 0xFFFFFFFF if tag_bits >= 32 else (1 << tag_bits) - 1


def min_slots_for(records_after, table_exact, pct=200):
    return (records_after * pct + 99) // 100 if table_exact else 2 * records_after


def slots_for(records_after, exact, pct=200):
    return max(pow2_at_least((records_after * pct + 99) // 100 if exact else 4 * records_after), MIN_SLOTS)


@dataclass(frozen=True)
class Geometry:
    slots: int
    seg_bits: int
    bits1: int
    bits2: int
    tag_mask: int

    @property
    def n_buckets(self):
        return self.slots >> self.seg_bits

    @property
    def seg_slots(self):
        return 1 << self.seg_bits


def geometry(slots, want_seg_bits=13):
    sb = seg_bits_for(slots, want_seg_bits)
    b1, b2 = table_digits(log2_ceil(slots), sb)
    return Geometry(slots, sb, b1, b2, tag_mask_for(slots, sb))


class TableSize:
    """ensure_table's history of one engine: created with a capacity hint or none, then told the record total after
    every submit.  .slots is what stats()["table_slots"] must say."""
    def __init__(self, capacity_reads=0):
        self.slots, self.exact = 0, False
        if capacity_reads:
            self.after(capacity_reads, exact=True)

    def after(self, records_after, exact=False):
        if self.slots and self.slots >= min_slots_for(records_after, self.exact):
            return self.slots
        self.exact = exact
        self.slots = slots_for(records_after, exact)
        return self.slots


def bulk_applies(n, records_before, slots):
    """bulk_applies of csrc/fqd_engine.hip with FQD_BULK_MIN=0."""
    return slots >= (1 << 13) and (records_before == 0 or n * BULK_RATIO >= slots)


# ---- pools of reads with their hashes ------------------------------------------------------------------------------------
ACGT = np.frombuffer(b"ACGT", np.uint8)


class Pool:
    """n distinct random records.  lengths: one tuple of mate lengths per shape the pool mixes, e.g. [(32,)], [(150, 150)],
    [(149,), (150,), (151,)]: record i has shape i % len(lengths).  .mates[m] is an (n, max length of mate m) uint8 array, zero
    behind a shorter read; .lens[m] the lengths; .hash the 64 placement bits of every record (weak: what
    FQD_FLAG_WEAK_HASH leaves of them)."""
    def __init__(self, seed, n, lengths, weak=False):
        rng = np.random.default_rng(seed)
        S = len(lengths[0])
        assert all(len(t) == S for t in lengths)
        self.S, self.n, self.weak = S, n, weak
        self.uniform = len(lengths) == 1
        shape = np.arange(n) % len(lengths)
        self.lens = [np.array([t[m] for t in lengths], np.uint32)[shape] for m in range(S)]
        self.width = [max(t[m] for t in lengths) for m in range(S)]
        self.mates = []
        for m in range(S):
            rows = ACGT[rng.integers(0, 4, size=(n, self.width[m]))]
            rows[np.arange(self.width[m])[None, :] >= self.lens[m][:, None]] = 0
            self.mates.append(rows)
        assert len(np.unique(self.key_rows(np.arange(n)), axis=0)) == n, "the pool's records are not distinct"
        h = np.zeros(n, np.uint64)
        for k, t in enumerate(lengths):
            sel = np.flatnonzero(shape == k)
            w = [kl.words_of_rows(np.ascontiguousarray(self.mates[m][sel, :t[m]])) for m in range(S)]
            h[sel] = kl.hashes_of_rows(t[0], w[0]) if S == 1 else kl.hashes_of_rows(t[0], w[0], t[1], w[1])
        self.hash = h & np.uint64(kl.weak(kl.M64)) if weak else h

    def key_rows(self, idx):
        """The bytes that make records equal or not: every mate's bases (zero-padded) and length, side by side."""
        cols = []
        for m in range(self.S):
            cols.append(self.mates[m][idx])
            cols.append(self.lens[m][idx].astype("<u4").view(np.uint8).reshape(-1, 4))
        return np.ascontiguousarray(np.concatenate(cols, axis=1))


@dataclass
class Placement:
    geom: Geometry
    pos: np.ndarray          # table position of the record's first probe
    bucket: np.ndarray       # pos >> seg_bits: the segment, = (digit1 << bits2) | digit2
    digit1: np.ndarray
    start: np.ndarray        # first slot probed inside the segment
    tag: np.ndarray          # what a slot remembers of the hash


def place(hashes, geom):
    pos = hashes & np.uint64(geom.slots - 1)
    bucket = (pos >> np.uint64(geom.seg_bits)).astype(np.int64)
    return Placement(geom, pos.astype(np.int64), bucket, bucket >> geom.bits2,
                     (pos & np.uint64(geom.seg_slots - 1)).astype(np.int64),
                     ((hashes >> np.uint64(32)) & np.uint64(geom.tag_mask)).astype(np.int64))


class Picker:
    """Hands out pool records by bucket, every record at most once."""
    def __init__(self, pool, geom):
        self.pool, self.geom, self.at = pool, geom, place(pool.hash, geom)
        self.free = np.ones(pool.n, bool)

    def take(self, bucket, count, distinct_tags=True, digit1=None):
        """count unused records of `bucket` (or, with digit1, of any bucket of that level-1 digit), with pairwise different
        tags unless told otherwise (the weak hash has one tag)."""
        where = self.at.digit1 == digit1 if digit1 is not None else self.at.bucket == bucket
        cand = np.flatnonzero(where & self.free)
        if distinct_tags:
            key = self.at.bucket[cand] * (int(self.geom.tag_mask) + 1) + self.at.tag[cand]     # tags need differ inside a bucket only
            _, first = np.unique(key, return_index=True)
            cand = cand[np.sort(first)]
        assert len(cand) >= count, f"the pool holds {len(cand)} such records, {count} are wanted"
        got = cand[:count]
        self.free[got] = False
        return got

    def take_outside(self, buckets, count):
        """count unused records of any bucket but `buckets`, different tags per bucket."""
        ok = self.free & ~np.isin(self.at.bucket, np.asarray(list(buckets)))
        cand = np.flatnonzero(ok)
        key = self.at.bucket[cand] * (int(self.geom.tag_mask) + 1) + self.at.tag[cand]
        _, first = np.unique(key, return_index=True)
        cand = cand[np.sort(first)]
        assert len(cand) >= count
        got = cand[:count]
        self.free[got] = False
        return got


# ---- the reference: first occurrence wins, over the bytes ---------------------------------------------------------------
def unique_rows(rows):
    """np.unique(rows, axis=0, return_index=True, return_inverse=True) without its slow sort of whole rows: np.unique over
    one 8-byte column at a time, the columns' class numbers combined pair by pair (exact: numbers, not hashes).  Returns
    (class numbers in use, first record of every class, class of every record)."""
    n, w = rows.shape
    if (-w) % 8:
        rows = np.concatenate([rows, np.zeros((n, (-w) % 8), np.uint8)], axis=1)
    cols = np.ascontiguousarray(rows).view("<u8")
    code = np.zeros(n, np.int64)
    for c in range(cols.shape[1]):
        values, inv = np.unique(cols[:, c], return_inverse=True)
        code = np.unique(code * len(values) + inv.reshape(-1), return_inverse=True)[1].reshape(-1)      # both factors are at most n
    return np.unique(code, return_index=True, return_inverse=True)


class FirstOccurrence:
    """keep[i] = 1 for the first record of every distinct row.  cls[i] numbers the rows' classes; first[i] = the first
    record of record i's class.  earlier(i): the records before i with i's row (what a link of i may name)."""
    def __init__(self, rows):
        rows = np.ascontiguousarray(rows)
        n = len(rows)
        _, first_of_class, cls = unique_rows(rows)
        self.cls = np.asarray(cls).reshape(-1)
        self.first = first_of_class[self.cls]
        self.keep = (self.first == np.arange(n)).astype(np.uint8)
        self.duplicates = int(n - self.keep.sum())
        self._order = np.argsort(self.cls, kind="stable")
        self._class_start = np.searchsorted(self.cls[self._order], np.arange(len(first_of_class) + 1))

    def earlier(self, i):
        c = self.cls[i]
        members = self._order[self._class_start[c]:self._class_start[c + 1]]
        return set(int(j) for j in members if j < i)

    def links_hold(self, got_keep, link):
        """Every dropped record's link names a member of earlier(i): an earlier record of i's class."""
        dup = np.flatnonzero(np.asarray(got_keep) == 0)
        to = np.asarray(link)[dup].astype(np.int64)
        return bool(np.all(to < dup) and np.all(to >= 0) and np.all(self.cls[np.minimum(to, len(self.cls) - 1)] == self.cls[dup]))


def first_occurrence(pool, idx):
    """The reference over the pool records idx (in submission order, batches concatenated)."""
    return FirstOccurrence(pool.key_rows(np.asarray(idx)))


def first_occurrence_of_reads(mate1, mate2=None):
    """The same over plain (n, L) arrays of read bytes: mate 1, or mate 1 || mate 2 for pairs."""
    return FirstOccurrence(mate1 if mate2 is None else np.concatenate([mate1, mate2], axis=1))
