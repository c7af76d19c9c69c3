"""Near-duplicate families through every key compare of the insert paths.

A record is a duplicate iff a word-for-word compare says so: keys_equal (insert_kernel, heavy_bucket_insert_kernel,
the inline walk of bucket_dedup_kernel) and the verify phase of bucket_dedup_kernel<FRESH, RAGGED, VL>.  The other
tests feed them reads of random pools, of which any two differ in most words: a compare that skipped one lane's 16
bytes, the words past 16 or the ragged header would still tell every pair apart.  Here the input is families: a base
read and ALL its single-base neighbours (every position, every other letter of ACGTN, so also G -> N, which changes
the N-mask word alone), for ragged engines also the base read cut by one base and grown by one (same words where the
word count allows, another header).  Any two members differ in one or two words only.

Which verify variant a key shape takes (launch_bulk_insert, csrc/fqd_engine.hip): uniform key store with an even
W0: W0 <= 8 -> VL 4 (four lanes x 16 B), W0 <= 16 -> VL 8 (eight lanes x 16 B), else VL 0; odd W0, FQD_DEDUP_VL=0
(read per call) and ragged stores -> VL 0 (eight lanes x one or two words, the words past 16 in a tail loop; ragged:
the header word first).

Unequal keys only meet behind a tag match, so the families run with FQD_FLAG_WEAK_HASH (every tag zero, every start
slot a multiple of 64: every occupied slot a record walks over is fully compared) and without it.  The engine's
smallest table has 65536 slots = 1024 start classes; each shape brings enough families (of different base reads)
for at least 4 distinct keys per class, which the tests assert from stats()["table_slots"].

That ratio alone does not say that the keys a given compare could get wrong meet.  The hash is restated in
tests/key_layout.py, so the input is built until they do, and the tests assert it (meeting_pairs): for every lane of
the shape's verify variant, for the words past 16 and — ragged — for the header, at least two pairs of keys that
differ THERE ALONE start in the same class (a class holds a few dozen keys at most, so one of the two walks over
the other's slot).  Keys that differ in the header alone have other lengths, which enter the hash: a family's
B[:-1] / B / B + 'A' practically never share a class, so base reads whose trio does are picked by the restated hash.
"""
import functools

import numpy as np
import pytest

import key_layout as kl
from fastq_dupaway_amd import Engine, Reads

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
LETTERS = b"ACGTN"
MIN_CLASSES = 65536 // 64              # start classes of the smallest table under the weak hash
SECOND_BATCH = 6000                    # bulk_applies: a batch into a table that holds records goes the bulk way from slots / 12 = 5462 records on

# uniform key shapes: mate lengths -> W0 -> verify variant
#   (32,)       W0 2   VL 4, only lane 0 loads        (150, 150)  W0 16  VL 8
#   (100,)      W0 6   VL 4, lanes 0-2                (150, 101)  W0 14  VL 8, last lane idle
#   (150,)      W0 8   VL 4, all lanes                (75,)       W0 5   odd -> VL 0
#   (384,)      W0 18  VL 0, tail loop                (450,)      W0 23  VL 0, tail loop
UNIFORM_SHAPES = [(32,), (100,), (150,), (150, 150), (150, 101), (75,), (384,), (450,)]
RAGGED_SHAPES = [(150,), (384,), (150, 101)]


def neighbours(base):
    """The base read and every single substitution of it: (1 + 4 L, L)."""
    L = len(base)
    out = np.tile(base, (1 + 4 * L, 1))
    k = 1
    for p in range(L):
        for c in LETTERS:
            if c != base[p]:
                out[k, p] = c
                k += 1
    assert k == len(out)
    return out


def family(rng, lens, ragged):
    """One family as a list of records, a record = a tuple of byte strings (one per mate).  Pairs: substitutions in
    mate 1 only and in mate 2 only — among them the last base of mate 1 and the first of mate 2, the two sides of the
    key's split.  ragged: the base read ends in 'A' (what the packer pads with), so that cutting it by one base, or
    adding an 'A', changes the header and nothing else wherever the word count stays."""
    bases = [rng.choice(ACGT, size=L) for L in lens]
    if ragged:
        for b in bases:
            b[-1] = ord("A")
    whole = [bytes(b) for b in bases]
    members = []
    for m in range(len(lens)):
        for row in neighbours(bases[m])[0 if m == 0 else 1:]:
            rec = list(whole); rec[m] = bytes(row); members.append(tuple(rec))
    if ragged:
        for m in range(len(lens)):
            for other in (whole[m][:-1], whole[m] + b"A", whole[m] + b"C"):
                rec = list(whole); rec[m] = other; members.append(tuple(rec))
    assert len(set(members)) == len(members)
    return members


def keys_of(members):
    """Per member (a tuple of byte strings): its key words and its hash, by tests/key_layout.py."""
    words, hashes = [None] * len(members), np.zeros(len(members), np.uint64)
    by_len = {}
    for i, r in enumerate(members):
        by_len.setdefault(tuple(len(x) for x in r), []).append(i)
    for ln, idx in by_len.items():
        w = [kl.words_of_rows(np.array([np.frombuffer(members[i][m], np.uint8) for i in idx]).reshape(len(idx), ln[m])) for m in range(len(ln))]
        h = kl.hashes_of_rows(ln[0], w[0], *((ln[1], w[1]) if len(ln) == 2 else ()))
        both = np.concatenate(w, axis=1)
        for k, i in enumerate(idx):
            words[i], hashes[i] = both[k], h[k]
    return words, hashes


def start_class(h):
    """The start slot of a hash under FQD_FLAG_WEAK_HASH in the smallest table (65536 slots)."""
    return kl.weak(int(h)) & (MIN_CLASSES * 64 - 1)


def lane_groups(W0, ragged):
    """The word sets one lane of the shape's verify variant owns, and the words past 16 (the tail loops)."""
    if not ragged and W0 % 2 == 0 and W0 <= 16:                             # VL 4 / VL 8: lane s loads words 2s, 2s + 1
        return {f"lane {s}": {2 * s, 2 * s + 1} for s in range(W0 // 2)}
    g = {f"lane {s}": {s, s + 8} & set(range(min(W0, 16))) for s in range(min(W0, 8))}       # VL 0: lane s words s, s + 8
    if W0 > 16:
        g["past 16"] = set(range(16, W0))
    return g


def meeting_pairs(members, lens, ragged):
    """{group: pairs of distinct keys that start in the same class and differ in that group's words alone};
    "header": equal words, other lengths (ragged)."""
    words, hashes = keys_of(members)
    groups = lane_groups(kl.seg_words(lens[0]) + (kl.seg_words(lens[1]) if len(lens) == 2 else 0), ragged)
    count = {g: 0 for g in groups}
    if ragged:
        count["header"] = 0
    by_class = {}
    for i, h in enumerate(hashes):
        by_class.setdefault(start_class(h), []).append(i)
    for idx in by_class.values():
        for a in range(len(idx)):
            for b in range(a + 1, len(idx)):
                i, j = idx[a], idx[b]
                same_len = [len(x) for x in members[i]] == [len(x) for x in members[j]]
                if len(words[i]) != len(words[j]):
                    continue
                d = set(np.flatnonzero(words[i] != words[j]).tolist())
                if not d:
                    assert not same_len
                    if ragged:
                        count["header"] += 1
                elif same_len:
                    for g, ws in groups.items():
                        if d <= ws:
                            count[g] += 1
    return count


def header_trios(rng, lens, want=8, candidates=8192):
    """Records that differ in the header alone AND meet: for each mate, base reads B ending in 'A' of which two of
    B[:-1], B, B + 'A' have the same number of key words and, by the restated hash, the same start class."""
    out = []
    for m in range(len(lens)):
        rows = [rng.choice(ACGT, size=(candidates, L)) for L in lens]
        rows[m][:, -1] = ord("A")
        forms = [rows[m][:, :-1], rows[m], np.concatenate([rows[m], np.full((candidates, 1), ord("A"), np.uint8)], axis=1)]
        cls = []
        for f in forms:
            mates = list(rows); mates[m] = f
            w = [kl.words_of_rows(x) for x in mates]
            h = kl.hashes_of_rows(mates[0].shape[1], w[0], *((mates[1].shape[1], w[1]) if len(lens) == 2 else ()))
            cls.append((h & np.uint64(0xFFFFFFC0)) & np.uint64(MIN_CLASSES * 64 - 1))
        nw = [kl.seg_words(f.shape[1]) for f in forms]
        meet = np.zeros(candidates, bool)
        for a, b in ((0, 1), (1, 2), (0, 2)):
            if nw[a] == nw[b]:
                meet |= cls[a] == cls[b]
        picked = np.flatnonzero(meet)[:want]
        assert len(picked) >= 2, (lens, m)
        for c in picked:
            for f in forms:
                rec = [bytes(rows[k][c]) for k in range(len(lens))]; rec[m] = bytes(f[c]); out.append(tuple(rec))
    return out


def picked_pairs(rng, lens, ws, ragged, want=4, candidates=8192):
    """Pairs of records that differ in the words `ws` alone AND meet, for a word set the families' members rarely
    meet in (a mask word that covers a few bases): B against B with one base changed — a letter of ACGT where ws holds
    the base's codes word, else G against N (the mask word alone) — picked by the restated hash's start class."""
    spots = []                                                               # (mate, position, codes word, mask word)
    first = 0
    for m, L in enumerate(lens):
        for p in range(L):
            blk, r = divmod(p, 64)
            spots.append((m, p, first + 3 * blk + r // 32, first + 3 * blk + (2 if L - 64 * blk > 32 else 1)))
        first += kl.seg_words(L)
    codes = [x for x in spots if x[2] in ws]
    m, p, _, _ = codes[0] if codes else [x for x in spots if x[3] in ws][0]
    rows = [rng.choice(ACGT, size=(candidates, L)) for L in lens]
    if ragged:
        for r in rows:
            r[:, -1] = ord("A")
    other = rows[m].copy()
    if codes:
        other[:, p] = np.where(rows[m][:, p] == ord("C"), ord("T"), ord("C"))
    else:
        rows[m][:, p] = ord("G"); other[:, p] = ord("N")
    cls = []
    for f in (rows[m], other):
        mates = list(rows); mates[m] = f
        w = [kl.words_of_rows(x) for x in mates]
        h = kl.hashes_of_rows(lens[0], w[0], *((lens[1], w[1]) if len(lens) == 2 else ()))
        cls.append((h & np.uint64(0xFFFFFFC0)) & np.uint64(MIN_CLASSES * 64 - 1))
    picked = np.flatnonzero(cls[0] == cls[1])[:want]
    assert len(picked) >= 2, (lens, ws)
    out = []
    for c in picked:
        for f in (rows[m], other):
            rec = [bytes(rows[k][c]) for k in range(len(lens))]; rec[m] = bytes(f[c]); out.append(tuple(rec))
    return out


@functools.lru_cache(maxsize=None)
def family_input(lens, ragged):
    """Records (every member of every family 1-3 times, shuffled with a fixed seed), the flags a dict gives them
    (first occurrence wins), the number of distinct keys and meeting_pairs of them.  Families are added until there
    are 4 keys per start class; a word set in which fewer than two pairs of them meet gets picked_pairs."""
    rng = np.random.default_rng(1000 * len(lens) + sum(lens) + (7 if ragged else 0))
    members = header_trios(rng, lens) if ragged else []
    while len(members) < 4 * MIN_CLASSES:
        members += family(rng, lens, ragged)
    W0 = sum(kl.seg_words(L) for L in lens)
    for g, ws in lane_groups(W0, ragged).items():
        if meeting_pairs(members, lens, ragged)[g] < 2:
            members += picked_pairs(rng, lens, ws, ragged)
    power = meeting_pairs(members, lens, ragged)
    assert len(members) < 12000                                              # 2 copies on average: the table stays at 65536 slots
    assert len(set(members)) == len(members)
    order = np.repeat(np.arange(len(members)), rng.integers(1, 4, len(members)))
    rng.shuffle(order)
    records = [members[k] for k in order]
    return records, first_wins(records), len(members), power


def first_wins(records):
    seen, keep = set(), np.zeros(len(records), np.uint8)
    for i, r in enumerate(records):
        if r not in seen:
            seen.add(r); keep[i] = 1
    return keep


def mate_arrays(records, m):
    """Mate m of the records back to back: (bytes, offsets, lengths)."""
    lens = np.array([len(r[m]) for r in records], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    data = np.frombuffer(b"".join(r[m] for r in records) + b"\0" * 16, np.uint8).copy()
    return data, offs, lens


def oracle_flags(oracle, records):
    mates = [mate_arrays(records, m) for m in range(len(records[0]))]
    return oracle.dedup_paired(*mates[0], *mates[1]) if len(mates) == 2 else oracle.dedup_single(*mates[0])


_CHECKED = set()


def checked_input(oracle, lens, ragged):
    """family_input, its dict flags held against the oracle's the first time a shape is asked for."""
    records, exp, distinct, power = family_input(lens, ragged)
    if (lens, ragged) not in _CHECKED:
        assert np.array_equal(oracle_flags(oracle, records), exp)
        assert 0 < int((exp == 0).sum()) < len(records)
        _CHECKED.add((lens, ragged))
    return records, exp, distinct, power


def submit_batches(records, cuts, lens, descriptors, weak, bulk, final):
    """The records in batches cut at `cuts`; descriptors[b]: "uniform" or "ragged".  Returns (flags, stats)."""
    S = len(records[0])
    got = []
    with Engine(segments=S, weak_hash=weak, profile=True) as e:
        for b, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            part = records[lo:hi]
            segs = []
            for m in range(S):
                data, offs, ln = mate_arrays(part, m)
                if descriptors[b] == "uniform":
                    assert np.all(ln == lens[m])
                    segs.append(Reads(data, uniform_len=lens[m], uniform_stride=lens[m]))
                else:
                    segs.append(Reads(data, offs, ln))
            got.append(e.submit(segs, hi - lo, final=final and hi == cuts[-1]))
        st, prof = e.stats(), e.profile()
    # the path the case is about was the one taken: bucket_dedup_kernel for every batch, or insert_kernel
    n = len(records)
    assert (prof["dedup_reads"], prof["insert_reads"]) == ((n, 0) if bulk else (0, n)), (prof["dedup_reads"], prof["insert_reads"])
    return np.concatenate(got), st


def assert_flags(got, exp, records, what):
    bad = np.flatnonzero(got != exp)
    if len(bad):
        i = int(bad[0])
        first = next(j for j in range(len(records)) if records[j] == records[i])
        raise AssertionError(f"{what}: {len(bad)} of {len(exp)} flags differ; record {i} (lengths {[len(x) for x in records[i]]}) "
                             f"got {int(got[i])}, expected {int(exp[i])}; its first copy is record {first}")


def run_family(oracle, monkeypatch, lens, ragged, weak, bulk_min):
    records, exp, distinct, power = checked_input(oracle, lens, ragged)    # the dict's flags, cross-checked with the oracle
    n = len(records)
    assert min(power.values()) >= 2, power                                  # every lane, the tail and the header have keys that meet
    assert n - SECOND_BATCH >= 1000
    monkeypatch.setenv("FQD_BULK_MIN", bulk_min)
    bulk = bulk_min == "0"
    kind = "ragged" if ragged else "uniform"
    # one batch: fresh segments; two batches, the copies split between them: a segment that holds records is loaded
    # into LDS (atomic path: owners resident in the table); the second batch also declared the last one
    plans = [([0, n], False), ([0, n - SECOND_BATCH, n], False), ([0, n - SECOND_BATCH, n], True)]
    variants = [{}]
    if bulk:
        variants.append({"FQD_HEAVY_ABOVE": "0"})                            # every bucket to heavy_bucket_insert_kernel (keys_equal)
        if not ragged:
            variants.append({"FQD_DEDUP_VL": "0"})                           # the 8-byte verify on a shape that takes VL 4 / 8
    for env in variants:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for cuts, final in plans:
            what = f"lens={lens} {kind} weak_hash={weak} FQD_BULK_MIN={bulk_min} {env} cuts={cuts} final={final}"
            got, st = submit_batches(records, cuts, lens, [kind] * (len(cuts) - 1), weak, bulk, final)
            assert_flags(got, exp, records, what)
            assert st["records"] == n and st["duplicates"] == int((exp == 0).sum()), what
            if weak:
                assert st["table_slots"] == 64 * MIN_CLASSES, what           # the table meeting_pairs counted for
                assert distinct * 64 >= 4 * st["table_slots"], what          # at least 4 distinct keys per start class
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("bulk_min", ["0", "-1"])
@pytest.mark.parametrize("weak", [True, False])
@pytest.mark.parametrize("lens", UNIFORM_SHAPES)
def test_uniform_families(oracle, monkeypatch, lens, weak, bulk_min):
    run_family(oracle, monkeypatch, lens, False, weak, bulk_min)


@pytest.mark.parametrize("bulk_min", ["0", "-1"])
@pytest.mark.parametrize("weak", [True, False])
@pytest.mark.parametrize("lens", RAGGED_SHAPES)
def test_ragged_families(oracle, monkeypatch, lens, weak, bulk_min):
    """Offsets / lengths descriptors: bucket_dedup_kernel<FRESH, true, 0> compares the header word, then the words;
    the members cut and grown by one base differ from the base read in the header alone (150: 149 / 150 / 151 bases
    are 8 words each), and header_trios brings such members that start in the same class."""
    run_family(oracle, monkeypatch, lens, True, weak, bulk_min)


@pytest.mark.parametrize("bulk_min", ["0", "-1"])
@pytest.mark.parametrize("weak", [True, False])
def test_uniform_engine_switched_to_ragged(oracle, monkeypatch, weak, bulk_min):
    """A first batch of 150-base reads under a uniform descriptor, then the whole family — other lengths and copies
    of first-batch members among it — under ragged descriptors: relayout_ragged_kernel rewrites the stored keys with
    headers, and the second batch's compares run against them."""
    lens = (150,)
    ragged_records, _, distinct, power = checked_input(oracle, lens, True)
    assert power["header"] >= 2, power
    first = [r for r in ragged_records if len(r[0]) == 150][:2500][::-1]
    records = first + ragged_records
    exp = first_wins(records)
    assert np.array_equal(oracle_flags(oracle, records), exp)
    assert 0 < int(exp[len(first):].sum()) < len(ragged_records)            # the second batch holds both copies and new keys
    monkeypatch.setenv("FQD_BULK_MIN", bulk_min)
    what = f"uniform then ragged, weak_hash={weak} FQD_BULK_MIN={bulk_min}"
    got, st = submit_batches(records, [0, len(first), len(records)], lens, ["uniform", "ragged"], weak, bulk_min == "0", False)
    assert_flags(got, exp, records, what)
    assert st["duplicates"] == int((exp == 0).sum()), what
    if weak:
        assert st["table_slots"] == 64 * MIN_CLASSES and distinct * 64 >= 4 * st["table_slots"], what
