"""The inputs of tests/test_gpu_scan_edges.py, test_gpu_plan_edges.py, test_gpu_hamming_walk.py and test_gpu_join_edges.py
held to their own claims on the host: those tests are only as good as the places their newlines, sums, clusters, key
fields and runs fall on.  No GPU."""
import numpy as np
import pytest

import hamming_walk_cases as hw
import join_edge_cases as jc
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


# ---- join --------------------------------------------------------------------------------------------------------------
SORT_CASES = list(jc.sort_cases())
JOIN_CASES = list(jc.join_cases())


def hold_to_claims(name, tags, claims):
    table = jc.code_table(tags)
    for what in ("min_len", "max_len", "B"):
        if what in claims:
            assert getattr(table, what) == claims[what], (name, what)
    for p, w in claims.get("widths", {}).items():
        assert table.width[p] == w, (name, p)
    assert table.B == sum(table.width) and (not table.width or table.lsb[-1] == 0)
    if "n_min_len" in claims:
        assert sum(len(t) == table.min_len for t in tags) == claims["n_min_len"], name
    if "crosses" in claims:
        p, bit = claims["crosses"]
        assert table.lsb[p] < bit < table.lsb[p] + table.width[p], name               # bits of the field on either side
        assert jc.deciders(tags, table, p, bit) >= claims["decided_by"], name
    return table


@pytest.mark.parametrize("name,tags,claims", SORT_CASES, ids=[c[0] for c in SORT_CASES])
def test_join_sort_case_keeps_its_claims_and_keys_order_as_bytes(name, tags, claims):
    table = hold_to_claims(name, tags, claims)
    order = jc.reference_sort(tags)
    assert sorted(range(len(tags)), key=lambda i: jc.key_of(tags[i], table)) == order
    keys = {}
    for t in tags:
        assert keys.setdefault(jc.key_of(t, table), t) == t                             # distinct tags, distinct keys
    assert all(k < 2 ** table.B for k in keys) and len(tags) <= 3000


def test_join_width_cases_reach_every_width_with_and_without_end():
    got = {(claims["widths"][1], kind) for kind, make, ks in (("fixed", jc.width_fixed, jc.FIXED_KS), ("ragged", jc.width_ragged, jc.RAGGED_KS))
           for k in ks for _, claims in [make(k)]}
    assert {(w, "fixed") for w in range(1, 9)} | {(w, "ragged") for w in range(1, 10)} == got
    assert jc.FIXED_KS == [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256]
    for k in jc.FIXED_KS:
        tags, _ = jc.width_fixed(k)
        assert {0, 255} <= {t[1] for t in tags} and len({t[1] for t in tags}) == k
    for k in jc.RAGGED_KS:                                       # 2^w - 1 values: END fits; 2^w: END costs a bit
        assert jc.width_ragged(k)[1]["widths"][1] == (k.bit_length() if k & (k + 1) == 0 else (k - 1).bit_length() + (k & (k - 1) == 0))
    for k in jc.MINLEN_KS:
        below, at = jc.width_at_min_len(k, False)[1]["widths"], jc.width_at_min_len(k, True)[1]["widths"]
        assert (below[2], at[3]) == ((k - 1).bit_length(), k.bit_length())
    assert jc.width_at_min_len(256, True)[1]["widths"][3] == 9 == jc.width_ragged(256)[1]["widths"][1]


def test_join_key_word_cases_cover_the_asked_places():
    for bit in (64, 128):
        for w in range(2, 9):
            ts = {t for ww, t, b in jc.CROSSINGS if (ww, b) == (w, bit)}
            assert {bit - w + 1, bit - 1} <= ts and (w not in (2, 5, 8) or ts == set(range(bit - w + 1, bit)))
    assert {63, 64, 65, 127, 128, 129, 130} == set(jc.KEY_BITS)
    table = jc.code_table(jc.one_bit_fields(130)[0])
    assert [sum(1 for l in table.lsb if 64 * word <= l < 64 * word + 64) for word in range(3)] == [64, 64, 2]


def test_join_census_cases_straddle_the_lds_rows():
    assert {jc.CENSUS_LDS - 1, jc.CENSUS_LDS, jc.CENSUS_LDS + 1} <= {n - 1 for n in jc.CENSUS_LENGTHS}
    for length in jc.CENSUS_LENGTHS:
        tags, _ = jc.census_last(length)
        assert len({t[:-1] for t in tags}) == 1 and len({t[-1] for t in tags}) == 200
    tags, _ = jc.census_four()
    table = jc.code_table(tags)
    assert [p for p, w in enumerate(table.width) if w] == [158, 159, 160, 161]
    order = jc.reference_sort(tags)
    assert any(tags[x][:159] == tags[y][:159] and tags[x][159] != tags[y][159] for x, y in zip(order, order[1:]))


@pytest.mark.parametrize("length", jc.HEAD_LENGTHS)
def test_join_head_cases_differ_where_they_say(length):
    a, b = jc.head_groups(length)
    table = jc.code_table(a + b)
    assert table.B > 64 and all(len({t[j] for t in a + b}) == 256 for j in range(8))
    top_bits = table.B - 64 * ((table.B - 1) // 64)
    u = [t for t, _, _ in jc.sorted_union(a, b)]
    kinds = set()
    for x, y in zip(u, u[1:]):
        if x[:8] == y[:8]:
            assert jc.key_of(x, table) >> (table.B - top_bits) == jc.key_of(y, table) >> (table.B - top_bits)   # equal top key word
            differ = [p for p in range(length) if x[p] != y[p]]
            kinds.add("same" if not differ else {length - 1: "last", length - 9: "ninth_last"}[differ[0]])
            assert len(differ) <= 1
    assert kinds == {"same", "last", "ninth_last"}
    a, b = jc.head_lengths_differ()
    u = [t for t, _, _ in jc.sorted_union(a, b)]
    assert any(len(x) + 1 == len(y) and y[:len(x)] == x for x, y in zip(u, u[1:]))


def test_join_stability_lists():
    assert {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289} == set(jc.STABLE_NS)
    assert {jc.SORT_TILE - 1, jc.SORT_TILE, jc.SORT_TILE + 1, 3 * jc.SORT_TILE + 1} <= set(jc.STABLE_NS)
    for n in jc.STABLE_NS:
        for kind in jc.STABLE_KINDS:
            tags = jc.stable_tags(n, kind)
            assert len(tags) == n
            table = jc.code_table(tags)
            assert table.B == jc.stable_claims(n, kind).get("B", table.B), (n, kind)
            if n >= 512:
                assert len(set(tags)) < n                        # equal tags: the permutation is a matter of stability
            if kind == "bytes_256" and n >= 256:
                counts = np.bincount([t[0] for t in tags], minlength=256)
                assert counts.min() == n // 256 and counts.max() <= n // 256 + 1
            assert sorted(range(n), key=lambda i: jc.key_of(tags[i], table)) == jc.reference_sort(tags)


@pytest.mark.parametrize("style", jc.RUN_STYLES)
def test_join_runs_lie_where_they_say(style):
    starts, b_starts = set(), set()
    for which, (s, runs) in enumerate(jc.RUN_LAYOUTS):
        a, b, claims = jc.run_case(which, style)
        u = jc.sorted_union(a, b)
        hot, at = claims["hot"], claims["run_start"]
        assert u[at][0] == hot and (at == 0 or u[at - 1][0] != hot), (which, style)
        assert len(set(t for t, _, _ in u[:at])) == at                               # singletons below
        if claims["b_start"] is not None:
            p = claims["b_start"]
            assert u[p][:2] == (hot, 1) and (p == at or u[p - 1][:2] == (hot, 0)), (which, style)
            b_starts.add(p)
        starts.add(at)
        assert (a.count(hot), b.count(hot)) == runs[0]
        W = (jc.code_table(a + b).B + 63) // 64
        assert (W == 1) if style == "short" else (W >= 2)
    T = jc.JOIN_TILE
    assert {T - 1, T, T + 1, 7, 8, 9, 511, 512, 513} <= starts and {T, 2 * T, 8, 512} <= b_starts
    whole = [(s + ra, s + ra + rb) for s, runs in jc.RUN_LAYOUTS for ra, rb in runs[:1] if rb >= T]
    assert any(lo % T == 0 and hi - lo >= T for lo, hi in whole) and any(lo % T == 0 and hi - lo >= 2 * T for lo, hi in whole)
    firsts = [runs[0] for _, runs in jc.RUN_LAYOUTS]
    assert any(ra > rb > 0 for ra, rb in firsts) and any(rb > ra > 0 for ra, rb in firsts)
    pairs_of_runs = [(x, y) for _, runs in jc.RUN_LAYOUTS for x, y in zip(runs, runs[1:])]
    assert any(x[1] == 0 and y[0] == 0 for x, y in pairs_of_runs) and any(x[0] == 0 and y[1] == 0 for x, y in pairs_of_runs)


def test_join_pair_patterns():
    T = jc.PAIR_TILE
    assert {T - 1, T, T + 1, 2 * T + 1} == set(jc.PAIR_NS)
    for n_a in jc.PAIR_NS:
        for pattern in jc.PAIR_PATTERNS:
            a, b, claims = jc.pair_case(n_a, pattern)
            j = jc.reference_join(a, b)
            assert [k for k, m in enumerate(j["match_a"]) if m != jc.NONE] == claims["matched"], (n_a, pattern)
            assert len(a) == n_a and len(j["pairs"]) == len(claims["matched"]) and j["match_b"].count(jc.NONE) > 100
        assert jc.pair_matched(n_a, "last_of_tile")[0] == min(T, n_a) - 1
        assert jc.pair_matched(n_a, "first_of_next_tile")[0] == (T if n_a > T else 0)


NUL_FREE_JOINS = [c for c in JOIN_CASES if not any(0 in t for t in c[1] + c[2])]


@pytest.mark.parametrize("name,a,b,claims", NUL_FREE_JOINS, ids=[c[0] for c in NUL_FREE_JOINS])
def test_join_reference_is_the_oracles_join(oracle, name, a, b, claims):
    j = jc.reference_join(a, b)
    i1, i2, unpaired = oracle.join_tags(*jc.tag_arrays(a), *jc.tag_arrays(b), tail_rule=False)
    assert list(zip(i1.tolist(), i2.tolist())) == j["pairs"]
    assert unpaired == len(a) + len(b) - 2 * len(j["pairs"])
    assert sorted(j["perm_a"]) == list(range(len(a))) and sorted(j["perm_b"]) == list(range(len(b)))
    assert all(j["match_b"][y] == x for x, y in enumerate(j["match_a"]) if y != jc.NONE)


def test_join_cases_with_nul_bytes_are_the_head_cases():
    assert len(NUL_FREE_JOINS) == len(JOIN_CASES) - len(jc.HEAD_LENGTHS) - 1 == 2 * len(jc.RUN_LAYOUTS) + len(jc.PAIR_NS) * len(jc.PAIR_PATTERNS)


def test_join_limit_rows_are_in_order_and_hold_every_value():
    rows = jc.all_values_everywhere(4096)
    assert len(rows) == 256 and {len(r) for r in rows} == {4096} and rows == sorted(rows)
    cols = np.frombuffer(b"".join(rows), np.uint8).reshape(256, 4096)
    assert (np.sort(cols, axis=0) == np.arange(256, dtype=np.uint8)[:, None]).all()     # 256 codes at each position: 8 bits
    assert 8 * 4096 == 32768 and jc.code_table(jc.all_values_everywhere(16)).B == 128


def test_join_extract_lines():
    lines = jc.extract_lines()
    text, starts, lens, exp_off, exp_len = jc.extract_text()
    assert len(starts) == 8 * len(lines) and len(text) < 8 << 20
    assert {(n, s % 8) for n, s in zip(lens, starts)} >= {(n, r) for n in range(1, 27) for r in range(8)}
    assert all(text[s + n - 1] == 10 and text[s:s + n].count(b"\n") == 1 for s, n in zip(starts, lens))
    for n in range(2, 27):
        mine = [l for l in lines if len(l) == n]
        inner = set(range(1, n - 1))
        assert {l.find(b".") for l in mine} == inner | {-1} and {l.find(b" ") for l in mine} == inner | {-1}
        assert any(b"." not in l and b" " not in l for l in mine)                    # near-misses only
        for hit in b". ":
            around = {(l[l.index(hit) - 1], l[l.index(hit) + 1]) for l in mine if hit in l and 1 < l.index(hit) < n - 2}
            assert n < 6 or ({x for x, _ in around} >= set(jc.NEAR) and {y for _, y in around} >= set(jc.NEAR))
        if n > 2:
            assert any(l[-2:] == b".\n" for l in mine)
    assert all(set(l[1:-1]) <= set(jc.NEAR + b". ") for l in lines)
    for n in (64, 65, 66):
        assert {l.find(b".") for l in lines if len(l) == n} == set(range(56, n - 1))
    assert {64} <= {l.find(b".") for l in lines if len(l) == 66}
    assert any(n == 0 for n in exp_len) and any(o + n == m for o, n, m in zip(exp_off, exp_len, lens))
