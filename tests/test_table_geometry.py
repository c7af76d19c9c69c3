"""csrc/fqd_table_geometry.hpp on the CPU (tests/native/table_geometry_check.cpp, built with g++): the invariants the bulk
insert's kernels rely on, for every table of 2^13 .. 2^31 slots and every wished segment width, and the plain Python
restatement of tests/bulk_placement.py that the GPU tests place their inputs with.  Also: the reference of those tests
(first occurrence over the read bytes) against the oracle."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bulk_placement as bp

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "table_geometry_check.cpp"
EXE = HERE / "native" / "table_geometry_check"
HDR = HERE.parent / "fastq-dupaway_amd" / "csrc" / "fqd_table_geometry.hpp"


@pytest.fixture(scope="module")
def printed():
    if not EXE.exists() or EXE.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(EXE), str(SRC)], check=True)
    out = subprocess.run([str(EXE)], capture_output=True, text=True, check=True).stdout
    rows = {"geom": [], "size": [], "clamp_seg": [], "clamp_pct": []}
    for line in out.splitlines():
        kind, *vals = line.split()
        rows[kind].append(tuple(int(v) for v in vals))
    return rows


def test_every_table_and_segment_width_is_listed(printed):
    assert [(t, w) for t, w, *_ in printed["geom"]] == [(t, w) for t in range(13, 32) for w in (12, 13, 14)]


def test_partition_record_packing_and_digit_widths(printed):
    for t, want, seg_bits, bits1, bits2, tag_mask in printed["geom"]:
        where = (t, want)
        assert 12 <= seg_bits <= 14, where
        nb_bits = max(0, t - seg_bits)                           # 2^13 slots under a 2^14-slot wish: no bucket at all (the engine's tables start at 2^16)
        assert bits1 + bits2 == nb_bits, where
        assert nb_bits <= 17, where                              # bulk_plan gives up above 2^17 buckets: never, up to 2^31 slots
        assert bits1 <= 8 and bits2 <= 9, where                  # 256 bins at level 1, 512 at level 2 (bulk_scatter_kernel)
        assert tag_mask & (tag_mask + 1) == 0, where             # a run of low bits
        if nb_bits:
            assert seg_bits + bits2 + bin(tag_mask).count("1") == 32, where      # BulkGeom: q fits the record's upper 32 bits
        if t - want <= 17:
            assert seg_bits == want, where                       # the wish holds wherever the bucket count allows it


def test_the_edges_the_gpu_tests_are_named_for(printed):
    """tests/test_gpu_bulk_edges.py relies on these geometries."""
    g = {(t, w): rest for t, w, *rest in printed["geom"]}
    assert g[(16, 12)][:3] == [12, 4, 0] and g[(16, 13)][:3] == [13, 3, 0] and g[(16, 14)][:3] == [14, 2, 0]
    assert g[(21, 13)][:3] == [13, 8, 0]                          # the last single-level geometry
    assert g[(22, 13)][:3] == [13, 5, 4] and g[(22, 12)][:3] == [12, 5, 5]
    assert g[(29, 13)][:3] == [13, 8, 8]                          # the widest digit2 byte plane
    assert g[(29, 12)][:3] == [12, 8, 9]                          # nine bits: bulk_hist2_kernel<true>
    assert g[(31, 12)][:3] == [14, 8, 9]                          # the segment widens so that 2^17 buckets are enough


def test_python_restatement_agrees(printed):
    for t, want, seg_bits, bits1, bits2, tag_mask in printed["geom"]:
        g = bp.geometry(1 << t, want)
        assert (g.seg_bits, g.bits1, g.bits2, g.tag_mask) == (seg_bits, bits1, bits2, tag_mask), (t, want)
        assert g.n_buckets == (1 << t) >> seg_bits
    for records, exact, pct, slots, min_slots in printed["size"]:
        assert bp.slots_for(records, bool(exact), pct) == slots, (records, exact, pct)
        assert bp.min_slots_for(records, bool(exact), pct) == min_slots, (records, exact, pct)
        assert slots >= 1 << 16 and slots & (slots - 1) == 0 and slots >= min_slots
    assert printed["clamp_seg"] == [(-1, 12), (0, 12), (11, 12), (12, 12), (13, 13), (14, 14), (15, 14), (99, 14)]
    assert printed["clamp_pct"] == [(0, 115), (114, 115), (115, 115), (200, 200), (400, 400), (401, 400)]


def test_sizing_history():
    """What the GPU tests count on: a table made for a capacity hint holds twice the hint and stays; one made without grows
    fourfold once it is more than half full."""
    assert bp.TableSize(1 << 21).slots == 1 << 22 and bp.TableSize(1 << 20).slots == 1 << 21 and bp.TableSize(1 << 28).slots == 1 << 29
    s = bp.TableSize(1 << 15)
    assert s.slots == 1 << 16 and s.after(32768) == 1 << 16 and s.after(32769) == 1 << 18
    s = bp.TableSize()
    assert s.after(1) == 1 << 16 and s.after(16384) == 1 << 16 and s.after(32768) == 1 << 16 and s.after(32769) == 1 << 18
    s = bp.TableSize()
    assert s.after(16385) == 1 << 17
    assert bp.bulk_applies(5462, 1, 1 << 16) and not bp.bulk_applies(5461, 1, 1 << 16) and bp.bulk_applies(1, 0, 1 << 16)
    assert bp.bulk_applies(349526, 1, 1 << 22) and not bp.bulk_applies(349525, 1, 1 << 22)


# ---- the helper's pools and its reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [[(32,)], [(75,)], [(40, 33)], [(63,), (64,), (65,)]])
def test_pool_hashes_are_the_scalar_statement(lengths):
    import key_layout as kl
    pool = bp.Pool(5, 60, lengths)
    for i in range(pool.n):
        seqs = [pool.mates[m][i, :pool.lens[m][i]].tobytes() for m in range(pool.S)]
        w = [kl.expected_words(s) for s in seqs]
        exp = kl.expected_hash(len(seqs[0]), len(seqs[1]) if pool.S == 2 else 0, w[0], w[1] if pool.S == 2 else None)
        assert int(pool.hash[i]) == exp
    weak = bp.Pool(5, 60, lengths, weak=True)
    assert all(int(a) == kl.weak(int(b)) for a, b in zip(weak.hash, pool.hash))


def test_picker_takes_different_tags_of_one_bucket():
    pool = bp.Pool(1, 30_000, [(32,)])
    g = bp.geometry(1 << 16, 13)
    pick = bp.Picker(pool, g)
    got = pick.take(3, 1500)
    at = pick.at
    assert np.all(at.bucket[got] == 3) and len(set(at.tag[got].tolist())) == 1500
    assert np.all(at.pos[got] == (3 << 13) + at.start[got]) and np.all(at.digit1[got] == 3)
    more = pick.take(3, 100)
    assert not set(more.tolist()) & set(got.tolist())
    out = pick.take_outside({3, 7}, 500)
    assert not np.isin(at.bucket[out], [3, 7]).any()
    with pytest.raises(AssertionError):
        pick.take(3, 30_000)


def test_reference_is_the_oracles_first_occurrence(oracle):
    rng = np.random.default_rng(11)
    n, L = 3000, 40
    src = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, size=(400, L))]
    a, b = src[rng.integers(0, 400, n)], src[rng.integers(0, 6, n)]
    offs, lens = np.arange(n, dtype=np.uint64) * np.uint64(L), np.full(n, L, np.uint32)
    flat = lambda x: np.concatenate([x.reshape(-1), np.zeros(16, np.uint8)])
    ref = bp.first_occurrence_of_reads(a)
    assert np.array_equal(ref.keep, oracle.dedup_single(flat(a), offs, lens)) and 0 < ref.duplicates < n
    ref2 = bp.first_occurrence_of_reads(a, b)
    assert np.array_equal(ref2.keep, oracle.dedup_paired(flat(a), offs, lens, flat(b), offs, lens))
    assert ref.duplicates > ref2.duplicates > 0
    # earlier(i): exactly the records before i with the same bytes
    for i in rng.integers(0, n, 50):
        exp = {j for j in range(int(i)) if a[j].tobytes() == a[i].tobytes()}
        assert ref.earlier(int(i)) == exp and (ref.keep[i] == 1) == (not exp)
    _, first_np, cls_np = np.unique(a, axis=0, return_index=True, return_inverse=True)        # the column-wise form against numpy's own
    assert np.array_equal(ref.first, first_np[np.asarray(cls_np).reshape(-1)])
    link = ref.first.copy()
    assert ref.links_hold(ref.keep, link)
    d = int(np.flatnonzero(ref.keep == 0)[-1])
    for wrong in (d, d + 1 if d + 1 < n else d, int(np.flatnonzero(ref.cls != ref.cls[d])[0])):      # itself, a later one, another key
        bad = link.copy(); bad[d] = wrong
        assert not ref.links_hold(ref.keep, bad)
    # a pool's own rows (mixed lengths, zero padded) against the oracle on the reads themselves
    pool = bp.Pool(2, 500, [(30,), (31,), (32,)])
    idx = rng.integers(0, 60, 400)
    stride = pool.width[0]
    got = bp.first_occurrence(pool, idx)
    exp = oracle.dedup_single(flat(pool.mates[0][idx]), np.arange(400, dtype=np.uint64) * np.uint64(stride), pool.lens[0][idx])
    assert np.array_equal(got.keep, exp)
