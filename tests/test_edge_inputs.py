"""The inputs of tests/test_gpu_scan_edges.py, test_gpu_plan_edges.py and test_gpu_hamming_walk.py held to their own claims
on the host: those tests are only as good as the places their newlines, sums and clusters fall on.  No GPU."""
import numpy as np
import pytest

import hamming_walk_cases as hw
import plan_edge_cases as pc
import scan_edge_cases as sc
import seq_reference as ref
from record_reference import numpy_records


# ---- scan ------------------------------------------------------------------------------------------------------------
def newline_offsets(text: bytes):
    return np.flatnonzero(np.frombuffer(text, np.uint8) == 10)


def tile_counts(text: bytes):
    return np.bincount(newline_offsets(text) // sc.TILE, minlength=(len(text) + sc.TILE - 1) // sc.TILE)


@pytest.mark.parametrize("name,k", sc.ids(sc.ALL))
def test_scan_case_is_whole_records(name, k):
    text = sc.text_of(name, k)
    assert text[-1:] == b"\n"
    assert text.count(b"\n") % k == 0
    start, seq_off, id_len, seq_len, size = numpy_records(text, k)
    assert len(start) == text.count(b"\n") // k and int(start[-1] + size[-1]) == len(text)
    lead = ord("@") if k == 4 else ord(">")
    assert all(text[int(s)] == lead for s in start)
    assert (id_len >= 2).all()                               # the lead and the '\n'
    if k == 4:
        nl = newline_offsets(text).reshape(-1, 4)
        assert np.array_equal(nl[:, 1] - nl[:, 0], nl[:, 3] - nl[:, 2])          # sequence and quality of one length
    m = sc.marks(name, k)
    assert all(text[p] == 10 for p in m["newlines"])
    assert set(m["record_starts"]) <= set(start.tolist())


@pytest.mark.parametrize("k", sc.KS)
def test_scan_newlines_are_on_the_edges(k):
    lane = np.array(sc.marks("lane_edges", k)["newlines"])
    assert (lane % sc.LANE == sc.LANE - 1).sum() >= 6 and (lane % sc.LANE == 0).sum() >= 6
    assert len(sc.text_of("lane_edges", k)) < sc.TILE
    tile = sc.marks("tile_edges", k)
    nl = np.array(tile["newlines"])
    assert (nl % sc.TILE == sc.TILE - 1).sum() >= 2 and (nl % sc.TILE == 0).sum() >= 2
    starts = np.array(tile["record_starts"])
    assert (starts % sc.TILE == 0).any() and (starts % sc.TILE == sc.TILE - 1).any()
    assert len(sc.text_of("tile_edges", k)) % sc.TILE == 0   # the last byte of the text is the last byte of a tile
    assert len(sc.text_of("one_record", k)) == 11


@pytest.mark.parametrize("k", sc.KS)
def test_scan_text_lengths(k):
    assert [len(sc.text_of("n_%d" % n, k)) % sc.LANE for n in (64, 65, 95)] == [0, 1, 31]
    for t in (1, 2):
        for r in (0, 1, sc.TILE - 1):
            assert len(sc.text_of("n_%dx8192+%d" % (t, r), k)) == t * sc.TILE + r


@pytest.mark.parametrize("k", sc.KS)
def test_scan_tiles_without_and_with_many_newlines(k):
    counts = tile_counts(sc.text_of("long_lines", k))
    runs = "".join("0" if c == 0 else "1" for c in counts)
    assert "00" in runs and "0000000" in runs                # 20 000 bytes: two whole tiles; 70 000: eight
    assert counts.max() >= 300
    text = sc.text_of("empty_lines", k)
    assert (b"\n\n+\n\n" if k == 4 else b"\n\n>") in text and text.endswith(b"\n\n")


@pytest.mark.parametrize("k", sc.KS)
def test_scan_part_cases_have_1024_1025_and_2049_tiles(k):
    for name, tiles in sc.PART_TILE_COUNTS.items():
        text = sc.text_of(name, k)
        assert (len(text) + sc.TILE - 1) // sc.TILE == tiles
        counts = tile_counts(text)
        assert len(set(counts.tolist())) > 10                # ragged: a carry that is off cannot hide behind equal counts
    assert len(sc.text_of("tiles_1024", k)) == sc.PART_TILES * sc.TILE
    assert sc.PART_TILES * sc.TILE in sc.marks("tiles_1025", k)["record_starts"]
    assert 60_000 > len(numpy_records(sc.text_of("tiles_2049", 2), 2)[0]) > 40_000


def test_scan_line_count_cases():
    cases = dict(sc.line_count_cases())
    assert len(cases["only_newlines"]) == 3 * sc.TILE + 5 == cases["only_newlines"].count(b"\n")
    assert len(cases["no_newline"]) == 3 * sc.TILE + 5 and cases["no_newline"].count(b"\n") == 0
    assert cases["one_byte_newline"] == b"\n" and len(cases["one_byte_other"]) == 1 and cases["one_byte_other"] != b"\n"


def host_well_formed(text: bytes, k: int) -> bool:
    """The rule of fqd_scan_records, in numpy."""
    nl = newline_offsets(text)
    if not text.endswith(b"\n") or len(nl) % k:
        return False
    start = numpy_records(text, k)[0]
    lead = ord("@") if k == 4 else ord(">")
    if any(text[int(s)] != lead for s in start):
        return False
    nl = nl.reshape(-1, k)
    return k == 2 or bool(np.array_equal(nl[:, 1] - nl[:, 0], nl[:, 3] - nl[:, 2]))


@pytest.mark.parametrize("kind", sc.DAMAGE)
def test_scan_damage_is_damage_and_nothing_else(kind):
    good, bad = sc.text_of("tiles_1025", 4), sc.damaged(kind)
    assert host_well_formed(good, 4) and not host_well_formed(bad, 4)
    assert abs(len(good) - len(bad)) <= 3
    if kind.startswith("bad_lead"):
        differ = np.flatnonzero(np.frombuffer(good, np.uint8) != np.frombuffer(bad, np.uint8))
        at = int(differ[0])
        assert len(differ) == 1 and at % sc.TILE == 0 and good[at] == ord("@")
        assert (at == sc.PART_TILES * sc.TILE) == (kind == "bad_lead_first_of_second_part")


# ---- plan ------------------------------------------------------------------------------------------------------------
def test_plan_sizes_are_on_the_edges():
    assert {pc.LANE - 1, pc.LANE, pc.LANE + 1, pc.TILE - 1, pc.TILE, pc.TILE + 1} <= set(pc.NS)
    wave, rnd = pc.WAVE_TILES * pc.TILE, pc.ROUND_TILES * pc.TILE
    assert {wave - 1, wave, wave + 1, rnd - 1, rnd, rnd + 1, rnd + pc.TILE + 3} <= set(pc.NS)


@pytest.mark.parametrize("n", [n for n in pc.NS if n <= 131_073])
def test_plan_wide_sums_need_64_bits(n):
    for keep_kind in pc.keeps_for(n):
        case = pc.make(n, keep_kind, "wide")
        kept = np.flatnonzero(case["keep"])
        assert len(kept) == {"all": n, "none": 0, "first": 1, "last": 1, "alternating": (n + 1) // 2}.get(keep_kind, len(kept))
        assert sorted(set(case["idx"].tolist())) == sorted(case["idx"].tolist()) and int(case["idx"].max()) < case["n_rec"]
        for use_idx in (True, False):
            src, lens, dst, total = pc.plan_reference(case, use_idx)
            if len(kept):
                assert lens[kept[0]] == pc.U32_MAX and lens[kept[-1]] == pc.U32_MAX      # planted, and kept
                assert total == sum(int(x) for x in lens)
            if len(kept) >= 2:
                assert total > 2**32 and int(dst[kept[1]]) == pc.U32_MAX
            if len(kept) >= 3:
                assert int(dst[kept[2]]) >= 2**32 or int(lens[kept[1]]) == 0
        dest, total = pc.offsets_reference(case)
        assert (dest >= 0).sum() == len(kept)


def test_plan_largest_wide_sum_and_the_small_sizes():
    case = pc.make(pc.NS[-1], "all", "wide")
    assert 2**51 < pc.plan_reference(case, True)[3] < 2**54
    small = pc.make(2049, "random", "small")
    assert small["sizes"].max() == 400 and (small["sizes"] == 0).any()
    assert pc.plan_reference(small, True)[3] == int(small["sizes"][small["idx"]][small["keep"] == 1].sum())


def test_plan_span_case():
    case = pc.span_case()
    kept_sizes = set(case["sizes"][case["idx"]][case["keep"] == 1].tolist())
    assert set(pc.SPAN_EDGES) <= kept_sizes and max(kept_sizes) <= 400
    assert len(set((case["starts"][case["idx"]] % 16).tolist())) == 16          # every alignment of the source
    assert len(pc.span_window(case)) == int(case["sizes"][case["idx"]][case["keep"] == 1].sum())
    ends = case["starts"] + case["sizes"]
    assert (ends[:-1] <= case["starts"][1:]).all() and int(ends[-1]) <= len(case["text"])


# ---- hamming walk ------------------------------------------------------------------------------------------------------
def check_layout(layout, d, what):
    recs, want = hw.records(layout), hw.flags(layout)
    mates = hw.shuffled(layout)
    assert [mates[i] for i in ref.sorted_order(mates)] == recs, what           # the sorted order is the layout
    assert ref.heads(ref.HAMMING, d, recs) == want, what                       # and the heads are the intended ones
    return recs, want


@pytest.mark.parametrize("d", hw.DISTANCES)
def test_hamming_lists_are_what_they_claim(d):
    assert len(hw.prefix(0, 8) + bytes(29)) == 37 and 37 % 8 and 5 < 8
    lanes_of_heads, totals, sizes_seen = set(), set(), set()
    for name, layout in hw.all_lists(d):
        recs, want = check_layout(layout, d, (d, name))
        assert len(recs) <= 20_000
        if name.startswith("lead"):
            lanes_of_heads |= {k % 64 for k, f in enumerate(want) if f}
            totals.add(len(recs) % 64)
            first = [r[0][:8] for r in recs]                 # sizes of the clusters = runs of one prefix
            runs = np.diff(np.flatnonzero([True] + [a != b for a, b in zip(first, first[1:])] + [True]))
            sizes_seen |= set(runs.tolist())
            lead = int(name[4:name.index("_")])
            assert list(runs[:lead]) == [1] * lead and want[lead] == 1 and lead % 64 in (0, 1, 62, 63)
            # neighbours at exactly 2d (no certain cut: both are members) and at 2d + 1 (a certain cut, so a head)
            pairs = [(hw.ham(a[0], b[0]), fa, fb) for (a, fa), (b, fb) in zip(layout, layout[1:])]
            assert any(h == 2 * d and fb == 0 for h, fa, fb in pairs)
            assert any(h == 2 * d + 1 and fb == 1 for h, fa, fb in pairs)
        if name.startswith("short"):
            assert {len(r[0]) for r in recs} == {5}
            totals.add(len(recs) % 64)
    assert {0, 63} <= lanes_of_heads and totals == set(hw.N_MODS) and set(hw.SIZES) <= sizes_seen


@pytest.mark.parametrize("d", hw.DISTANCES)
def test_hamming_members_at_d_and_heads_at_d_plus_1(d):
    """In a full cluster: D1 and D2 at exactly d are members, H2 at d + 1 is a head, Z is one substitution from the first
    head and still a head, because it is measured from H2.  The substitutions that decide lie on the word and tail edges."""
    used = set()
    for c in range(3):
        read = hw.prefix(c, 8) + b"AC" * 14 + b"A"
        H, D1, D2, H2, X, Z = [r for r, _ in hw.cluster(read, 8, 6, d, rot=c)]
        assert [f for _, f in hw.cluster(read, 8, 6, d, rot=c)] == [1, 0, 0, 1, 1 if d == 0 else 0, 1]
        assert (hw.ham(H, D1), hw.ham(H, D2), hw.ham(H, H2), hw.ham(D1, D2), hw.ham(D2, H2)) == (d, d, d + 1, 2 * d, 2 * d + 1)
        assert hw.ham(H2, X) == 1 and hw.ham(H, X) == d + 2 and hw.ham(H, Z) == 1 and hw.ham(H2, Z) == d + 2
        for r in (D1, D2, H2, X, Z):
            used |= {k - 8 for k in range(8, 37) if r[k] != H[k]}
    if d >= 2:
        assert set(hw.SPECIAL) <= used
    else:
        assert {0, 7, 8} <= used and (d == 0 or {23, 24, 28} <= used)


@pytest.mark.parametrize("d", [d for d in hw.DISTANCES if d >= 1])
def test_hamming_drift_chain_tells_head_based_from_neighbour_based(d):
    layout = hw.drift_list(d)
    recs, want = check_layout(layout, d, ("drift", d))
    by_neighbour = hw.neighbour_heads(d, recs)
    assert by_neighbour != want and sum(by_neighbour) == 3 < sum(want)
    assert all(hw.ham(a[0], b[0]) == 1 for a, b in zip(recs, recs[1:]) if a[0][:8] == b[0][:8])


@pytest.mark.parametrize("d", hw.DISTANCES)
def test_hamming_pairs_and_mixed_lengths(d):
    layout = hw.pair_list(d)
    check_layout(layout, d, ("pairs", d))
    seen = set()
    for (h, fh), (x, fx) in zip(layout, layout[1:]):
        if h[0][:8] != x[0][:8] or not fh:
            continue
        lens = (len(h[0]), len(h[1]), len(x[0]), len(x[1]))
        if lens == (37, 37, 37, 37):
            dist = (hw.ham(h[0], x[0]), hw.ham(h[1], x[1]))
            assert dist in ((d, d + 1), (d + 1, d), (d, d)) and fx == (0 if dist == (d, d) else 1)
            seen.add(("d", "d+1")[dist[0] - d] + "," + ("d", "d+1")[dist[1] - d])
        elif lens == (37, 36, 37, 37):
            assert h[0] == x[0] and fx == 1
            seen.add("length")
        else:
            assert lens == (37, 0, 37, 0) and hw.ham(h[0], x[0]) == d and fx == 0
            seen.add("empty")
    assert seen == {"d,d+1", "d+1,d", "d,d", "length", "empty"}
    places = {k % 64 for k, (r, f) in enumerate(layout) if k and layout[k - 1][0][0][:8] == r[0][:8]}
    assert {0, 63} <= places                                 # a cluster of two straddles two chunks, and ends one
    mixed = hw.mixed_length_list(d)
    recs, want = check_layout(mixed, d, ("mixed", d))
    assert {len(r[0]) for r in recs} == {36, 37}
    assert all(f == 1 for (a, _), (b, f) in zip(mixed, mixed[1:]) if len(a[0]) != len(b[0]))


@pytest.mark.parametrize("d", hw.LARGE_DISTANCES)
def test_hamming_large_distances_leave_one_cluster_per_length(d):
    for name, layout in hw.large_distance_lists(d):
        recs, want = check_layout(layout, d, (d, name))
        lens = [tuple(len(m) for m in r) for r in recs]
        assert want == [1] + [int(a != b) for a, b in zip(lens, lens[1:])]
    assert sum(hw.flags(dict(hw.large_distance_lists(d))["main"])) == 1
