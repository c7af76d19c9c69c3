"""fqd_sort_tags / fqd_join_tags / fqd_extract_tags (csrc/fqd_join.hip) on tag lists built around the join's own structure.
The lists are those of tests/join_edge_cases.py, which tests/test_edge_inputs.py holds to their claims on the host; the
reference is Python's stable order of bytes (`reference_sort`) and a join from dicts of tag to sorted positions
(`reference_join`).  Every comparison is exact: a permutation equal to the reference's is the stability check, a join
has to give all six arrays and the number of pairs, and 64 guard entries behind every output stay as they were.

Reached:
- code widths: every width 1 .. 8 at both ends of its range of values without END, 1 .. 9 with END (2^w - 1 values: END
  fits, 2^w: it costs a bit, 256: nine bits and `rank + 1 == 256`), bytes 0 and 255 among the values; the same number of
  values on either side of min_len, with one record of that length; tags that are prefixes of one another, the empty tag;
- key words: a field of 2 .. 8 bits across key bit 64 and across 128 at every split, a nine-bit field with END across 64,
  neighbours in sorted order decided by the field's high part, its low part and the positions on either side; keys of
  exactly 63, 64, 65, 127, 128, 129 bits (a last pass of one bit) and 130 (64 rows of the code table in a word); no key
  bits at all (equal tags, empty tags, one record);
- census: variation at position 158, 159, 160 or 161 alone (`kCensusLds = 160`), and at those four only;
- heads: tags of 31 .. 97 bytes that share the top key word and differ in the last byte, in byte L - 9, not at all, or
  in length;
- radix passes: 1 .. 12289 records (a wave's round of 64, the four waves' 1024, a tile's 4096, three tiles and one) of
  equal tags, two tags in turns of 1, 64 and 1024, all 256 digits, and a last pass of three bits;
- the join's scans: a run that starts on place 2047, 2048, 2049 (7, 8, 9; 511, 512, 513) of the sorted union, file 2's
  part starting a tile and covering one and two tiles without a head, either file's part the longer, a run of one file
  alone followed by a run of the other alone; with keys of one word and of several;
- pair compaction: 2047, 2048, 2049 and 4097 records of file 1 with all, none, every other, only a tile's last and only
  the next tile's first place matched;
- limits: a key of exactly 32768 bits is sorted, 32776 bits and 2^31 records are refused with nothing written;
- extract: ID lines of 1 .. 26 bytes at every start offset mod 8, a '.' and a ' ' at every place among bytes that differ
  from them in one bit, and lines of 64 .. 66 bytes whose first '.' lies in the last 8-byte word or behind it.

Not reached: `radix_rowscan_kernel`'s second round of 1024 tiles needs more than 4 M records, `join_carry_scan_kernel`'s
and `scan_tiles_kernel`'s more than 2 M, and the grid loops of the histogram and the scatter (2048 blocks) more than 8 M.
Only test_gpu_join.py::test_join_at_50m_tags_per_side goes there; a list that fits a test of seconds does not take those
paths, so nothing here stands in for them."""
import numpy as np
import pytest

import join_edge_cases as jc

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0x5A5A5A5A
ARRAYS = ("perm_a", "perm_b", "match_a", "match_b", "pair_a", "pair_b")


@pytest.fixture
def eng():
    from fastq_dupaway_amd import Engine
    with Engine(segments=2) as e:
        yield e


def to_dev(*arrs):
    import torch
    return [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
            for a in arrs]


def guarded(n, dtype="int32"):
    import torch
    return torch.full((n + GUARD,), FILL, dtype=getattr(torch, dtype), device="cuda")


def unguard(t, n, what):
    """The first n entries on the host; the guard behind them has to be as it was."""
    h = t.cpu().numpy()
    assert (h[n:] == FILL).all(), ("guard written", what)
    return h[:n].view(np.uint32 if h.dtype == np.int32 else np.uint64)


def device_sort(eng, tags, what):
    import torch
    d, o, l = to_dev(*jc.tag_arrays(tags))
    perm = guarded(len(tags))
    torch.cuda.synchronize()
    eng.sort_tags(d, o, l, len(tags), perm)
    return unguard(perm, len(tags), what)


def check_sort(eng, name, tags):
    got = device_sort(eng, tags, name)
    assert np.array_equal(got, np.array(jc.reference_sort(tags), dtype=np.uint32)), name


def device_join(eng, a, b, what):
    import torch
    A, B = to_dev(*jc.tag_arrays(a)), to_dev(*jc.tag_arrays(b))
    sizes = dict(perm_a=len(a), match_a=len(a), perm_b=len(b), match_b=len(b), pair_a=min(len(a), len(b)), pair_b=min(len(a), len(b)))
    out = {k: guarded(sizes[k]) for k in ARRAYS}
    torch.cuda.synchronize()
    n_pairs = eng.join_tags((*A, len(a)), (*B, len(b)), *(out[k] for k in ARRAYS))
    assert n_pairs <= sizes["pair_a"], what
    got = {k: unguard(out[k], n_pairs if k.startswith("pair") else sizes[k], (what, k)) for k in ARRAYS}
    got["n_pairs"] = n_pairs
    return got


def check_join(eng, name, a, b):
    got, want = device_join(eng, a, b, name), jc.reference_join(a, b)
    assert got["n_pairs"] == len(want["pairs"]), name
    want["pair_a"], want["pair_b"] = [x for x, _ in want["pairs"]], [y for _, y in want["pairs"]]
    for k in ARRAYS:
        assert np.array_equal(got[k], np.array(want[k], dtype=np.uint32)), (name, k)


def sort_cases(*prefixes):
    picked = [c for c in jc.sort_cases() if c[0].startswith(prefixes)]
    assert picked
    return picked


def join_cases(prefix):
    picked = [c for c in jc.join_cases() if c[0].startswith(prefix)]
    assert picked
    return picked


# ---- sort ----------------------------------------------------------------------------------------------------------------
def test_code_widths_without_end(eng):
    for name, tags, _ in sort_cases("fixed_"):
        check_sort(eng, name, tags)


def test_code_widths_with_end_and_around_min_len(eng):
    for name, tags, _ in sort_cases("ragged_", "below_min_len_", "at_min_len_", "prefix_chain"):
        check_sort(eng, name, tags)


def test_field_across_key_bit_64(eng):
    for name, tags, _ in sort_cases("cross_64_", "end_cross_"):
        check_sort(eng, name, tags)


def test_field_across_key_bit_128(eng):
    for name, tags, _ in sort_cases("cross_128_"):
        check_sort(eng, name, tags)


def test_keys_that_end_on_a_word_and_keys_of_no_bits(eng):
    for name, tags, _ in sort_cases("bits_", "all_e", "one_"):
        check_sort(eng, name, tags)


def test_variation_around_the_census_lds_rows(eng):
    for name, tags, _ in sort_cases("census_"):
        check_sort(eng, name, tags)


def test_sort_of_tags_that_share_the_top_key_word(eng):
    for name, tags, _ in sort_cases("heads_"):
        check_sort(eng, name, tags)


@pytest.mark.parametrize("kind", jc.STABLE_KINDS)
def test_sort_is_stable_across_rounds_waves_and_tiles(eng, kind):
    for n in jc.STABLE_NS:
        check_sort(eng, (kind, n), jc.stable_tags(n, kind))


# ---- join ----------------------------------------------------------------------------------------------------------------
def test_join_heads_of_tags_that_share_the_top_key_word(eng):
    for name, a, b, _ in join_cases("heads_"):
        check_join(eng, name, a, b)


@pytest.mark.parametrize("style", jc.RUN_STYLES)
def test_join_runs_on_thread_wave_and_tile_edges(eng, style):
    for name, a, b, _ in join_cases("run_"):
        if name.endswith(style):
            check_join(eng, name, a, b)


def test_join_pair_compaction_at_tile_edges(eng):
    for name, a, b, _ in join_cases("pairs_"):
        check_join(eng, name, a, b)


# ---- limits --------------------------------------------------------------------------------------------------------------
def limit_tags(length):
    rows = jc.all_values_everywhere(length)
    order = np.random.default_rng(length).permutation(256)
    return [rows[i] for i in order], np.argsort(order, kind="stable").astype(np.uint32)      # tag i is the i-th smallest


def test_key_of_exactly_32768_bits_is_sorted(eng):
    tags, want = limit_tags(4096)
    assert np.array_equal(device_sort(eng, tags, "32768 bits"), want)


def test_key_of_more_than_32768_bits_is_refused_and_nothing_is_written(eng):
    from fastq_dupaway_amd import FqdError
    from fastq_dupaway_amd import _lib
    import torch
    tags, _ = limit_tags(4097)
    d, o, l = to_dev(*jc.tag_arrays(tags))
    perm = guarded(256)
    torch.cuda.synchronize()
    with pytest.raises(FqdError) as err:
        eng.sort_tags(d, o, l, 256, perm)
    assert err.value.code == _lib.ERR_ARG and "ID tags need more than 32768 key bits" in err.value.message
    eng.sync()
    assert (perm.cpu().numpy() == FILL).all()
    check_sort(eng, "after a refusal", [b"b", b"a", b"b", b""])                          # the engine goes on


def test_2_31_records_are_refused_before_anything_is_launched(eng):
    from fastq_dupaway_amd import FqdError
    from fastq_dupaway_amd import _lib
    import torch
    tags = [b"b", b"a", b"c"]
    A, B = to_dev(*jc.tag_arrays(tags)), to_dev(*jc.tag_arrays(tags))
    out = [guarded(3) for _ in range(7)]
    torch.cuda.synchronize()
    with pytest.raises(FqdError) as err:
        eng.sort_tags(*A, 2 ** 31, out[6])
    assert err.value.code == _lib.ERR_ARG and "at most 2^31-1 records" in err.value.message
    for n_a, n_b in ((2 ** 31, 3), (3, 2 ** 31)):
        with pytest.raises(FqdError) as err:
            eng.join_tags((*A, n_a), (*B, n_b), *out[:6])
        assert err.value.code == _lib.ERR_ARG and "at most 2^31-1 records" in err.value.message
    eng.sync()
    assert all((t.cpu().numpy() == FILL).all() for t in out)
    eng.sort_tags(*A, 3, out[6])                                                         # the same arrays are fine with their own n
    assert unguard(out[6], 3, "n = 3").tolist() == [1, 0, 2]


# ---- extract -------------------------------------------------------------------------------------------------------------
def test_extract_tags_on_every_line_length_offset_and_place_of_the_hits(eng):
    import torch
    text, starts, lens, exp_off, exp_len = jc.extract_text()
    n = len(starts)
    d_text = torch.from_numpy(np.frombuffer(text + b"\n" * 16, dtype=np.uint8).copy()).cuda()
    d_start = torch.tensor(starts, dtype=torch.int64, device="cuda")
    d_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    off, ln = guarded(n, "int64"), guarded(n)
    torch.cuda.synchronize()
    eng.extract_tags(d_text, d_start, d_len, n, off, ln)
    eng.sync()
    got_off = unguard(off, n, "tag_off").astype(np.int64) - np.array(starts, dtype=np.int64)
    got_len = unguard(ln, n, "tag_len").astype(np.int64)
    bad = np.flatnonzero((got_off != np.array(exp_off)) | (got_len != np.array(exp_len)))
    assert len(bad) == 0, [(text[starts[k]:starts[k] + lens[k]], starts[k] % 8, int(got_off[k]), int(got_len[k])) for k in bad[:5]]
