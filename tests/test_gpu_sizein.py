"""GPU checks of FQD_FAST_SIZEIN's primitives (fqd_size_annotations, fqd_cluster_weights, fqd_size_relabel,
fqd_copy_relabelled in csrc/fqd_sizein.hip) through ctypes, against the plain-Python statement (tests/sizein_reference.py).

fqd_size_annotations: ID lines of 1 .. 600 bytes at every start modulo 16; `;size=` beginning at word offsets 10 .. 17 and
250 .. 258, so that the pattern and the digits straddle a lane's chunk and the group's round; 1 .. 11 digits; every end byte
and a line that ends without one; leading zeros; both sides of 2^31; every reason of the enum, and the lowest refused record
of several; annotations that only the comment holds; file 2 held against file 1's weights; n around the wave and block
sizes.  fqd_cluster_weights: test_gpu_sizes.py's sizes and tile-edge head patterns with random weights, weights of 1 against
fqd_cluster_sizes, every level edge reached by weight, a second round of the carry kernel, and runs above 2^31-1.
fqd_size_relabel and fqd_copy_relabelled: byte for byte around part lengths 1, 15, 16, 17 and cuts of 0, 7 and 16 bytes,
through a window, with the fill around the destination unchanged and the source ending with its allocation.  Guard entries
behind every output stay as they were."""
import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, _lib
from fastq_dupaway_amd._lib import FqdError
import size_reference as sizes
import sizein_reference as ref
import test_gpu_sizes as base                                 # its helpers: dev, guarded_u32, split_guard, layout, id_lines, NS, TILE
import test_sizein_core as core                               # its ID lines around the rule's edges

pytestmark = pytest.mark.gpu
dev, host_u32, guarded_u32, split_guard = base.dev, base.host_u32, base.guarded_u32, base.split_guard
TILE, PAD, FILL8 = base.TILE, base.PAD, base.FILL8
NO_RECORD = ref.NO_RECORD


# ---------------------------------------------------------------- fqd_size_annotations

def file_of(lines):
    """(device text, start, id_len) of records that are their ID lines alone, at starts that are i mod 16."""
    text, start, id_len, _ = base.layout(lines, [b""] * len(lines))
    return dev(np.frombuffer(text, np.uint8)), dev(start), dev(id_len), start


def annotate(e, d_text, d_start, d_len, n, lo=0, expect=None, outputs=True):
    weight, at, cut = (guarded_u32(n) for _ in range(3)) if outputs else (None, None, None)
    info = e.size_annotations(d_text, d_start[lo:], d_len[lo:], n, expect, weight, at, cut)
    assert info.reserved == 0
    if not outputs:
        return info, None
    return info, tuple(split_guard(x, n).tolist() for x in (weight, at, cut))


def accepted_lines():
    return [x for x in base.id_lines() + core.annotated_lines() if ref.parse(x)[3] == ref.OK]


@pytest.mark.parametrize("shift", [0, 5])
def test_weights_places_and_cuts_of_accepted_lines(shift):
    lines = [b"@x\n"] * shift + accepted_lines()
    n = len(lines)
    d_text, d_start, d_len, start = file_of(lines)
    assert sorted(set((start % 16).tolist())) == list(range(16))
    expect = ref.annotations(lines)
    annotated = [i for i in range(n) if expect[2][i]]
    assert {int(start[i]) % 16 for i in annotated} == set(range(16)) and {expect[2][i] for i in annotated} == set(range(7, 17))
    with Engine(segments=1) as e:
        info, got = annotate(e, d_text, d_start, d_len, n)
        assert (info.bad_record, info.bad_reason) == (NO_RECORD, ref.OK)
        assert got[0] == expect[0] and got[1] == expect[1] and got[2] == expect[2]
        assert info.annotated == len(annotated) and info.total_weight == sum(expect[0])
        # label_at of a line without an annotation is fqd_size_labels' value
        plain = [i for i in range(n) if not expect[2][i]]
        assert [got[1][i] for i in plain] == [sizes.first_word_end(lines[i]) for i in plain]
        # each output may be left out
        info, _ = annotate(e, d_text, d_start, d_len, n, outputs=False)
        assert (info.bad_record, info.annotated, info.total_weight) == (NO_RECORD, len(annotated), sum(expect[0]))


def test_every_reason_and_the_lowest_refused_record():
    rng = np.random.default_rng(41)
    good = accepted_lines()
    bad = [x for x in core.annotated_lines() if ref.parse(x)[3] != ref.OK]
    by_reason = {}
    for x in bad:
        by_reason.setdefault(ref.parse(x)[3], []).append(x)
    assert set(by_reason) == {ref.NO_DIGITS, ref.BAD_END, ref.ZERO, ref.TOO_LARGE, ref.TWICE}
    chosen = [x for xs in by_reason.values() for x in xs[::max(1, len(xs) // 25)]]          # about 25 of every reason
    lines, at = [], []
    for x in chosen:                                          # each behind 0 .. 69 accepted lines: every lane and step of a wave's tile
        lines += [good[int(k)] for k in rng.integers(0, len(good), int(rng.integers(0, 70)))]
        at.append(len(lines))
        lines.append(x)
    d_text, d_start, d_len, _ = file_of(lines)
    with Engine(segments=1) as e:
        lo = 0
        for b, x in zip(at, chosen):                          # the slice [lo, b] holds one refused record, its last
            info, _ = annotate(e, d_text, d_start, d_len, b + 1 - lo, lo=lo)
            assert (info.bad_record, info.bad_reason) == (b - lo, ref.parse(x)[3]), x
            lo = b + 1
        for first in (0, 3, len(at) - 2):                     # several refused records: the lowest is named
            lo = at[first - 1] + 1 if first else 0
            info, _ = annotate(e, d_text, d_start, d_len, len(lines) - lo, lo=lo, outputs=False)
            assert (info.bad_record, info.bad_reason) == (at[first] - lo, ref.parse(chosen[first])[3])


def test_file_two_is_held_against_file_ones_weights():
    rng = np.random.default_rng(42)
    n = 300
    w1 = [int(rng.choice([1, 1, 2, 17, 2147483647])) for _ in range(n)]
    lines2 = [f"@r{i}{f';size={w1[i]}' if i % 3 else ''}{' 2:N:0' if i % 2 else ''}\n".encode() for i in range(n)]      # agreeing, or absent
    d_text, d_start, d_len, _ = file_of(lines2)
    with Engine(segments=1) as e:
        info, got = annotate(e, d_text, d_start, d_len, n, expect=dev(np.array(w1, np.uint32)))
        assert info.bad_record == NO_RECORD and got[0] == [w1[i] if i % 3 else 1 for i in range(n)]
        other = list(w1)
        for at in (299, 130, 64, 7):                          # differing at lower and lower records: the lowest is named
            assert at % 3
            other[at] += 1 if other[at] < ref.MAX else -1
            info, _ = annotate(e, d_text, d_start, d_len, n, expect=dev(np.array(other, np.uint32)), outputs=False)
            assert (info.bad_record, info.bad_reason) == (at, ref.MATES_DIFFER)
        # a malformed annotation in file 2 is refused for its own reason, lower or not
        lines2[5] = b"@r5;size=x\n"
        d_text, d_start, d_len, _ = file_of(lines2)
        info, _ = annotate(e, d_text, d_start, d_len, n, expect=dev(np.array(w1, np.uint32)), outputs=False)
        assert (info.bad_record, info.bad_reason) == (5, ref.NO_DIGITS)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_parse_at_the_wave_and_block_edges(n):
    rng = np.random.default_rng(n)
    lines = [f"@read{i}{f';size={int(rng.integers(1, 5000))}' if rng.random() < 0.6 else ''}{' c;size=9' if i % 2 else ''}\n".encode() for i in range(n)]
    with Engine(segments=1) as e:
        if n == 0:
            info = e.size_annotations(None, None, None, 0, None, None, None, None)
            assert (info.bad_record, info.annotated, info.total_weight) == (NO_RECORD, 0, 0)
            return
        d_text, d_start, d_len, _ = file_of(lines)
        expect = ref.annotations(lines)
        info, got = annotate(e, d_text, d_start, d_len, n)
        assert info.bad_record == NO_RECORD and list(got) == [expect[0], expect[1], expect[2]]
        lines[n - 1] = b"@last;size=0\n"                        # the last record of the last wave
        d_text, d_start, d_len, _ = file_of(lines)
        info, _ = annotate(e, d_text, d_start, d_len, n)
        assert (info.bad_record, info.bad_reason) == (n - 1, ref.ZERO)


def test_parse_misuse_is_refused():
    d_text, d_start, d_len, _ = file_of([b"@a;size=2\n"] * 10)
    with Engine(segments=1) as e:
        for args in ((d_text, d_start, d_len, 10, None, None, None, None, None),                # info is not optional
                     (d_text, np.zeros(10, np.uint64), d_len, 10, None, None, None, None, True),   # a host pointer
                     (None, d_start, d_len, 10, None, None, None, None, True), (d_text, d_start, d_len, 2 ** 32 - 1, None, None, None, None, True)):
            with pytest.raises(FqdError, match="fqd_size_annotations") as ei:
                e.size_annotations(*args)
            assert ei.value.code == _lib.ERR_ARG


# ---------------------------------------------------------------- fqd_cluster_weights

def check_weights(e, perm, head, weight, levels=True):
    perm, head, weight = np.asarray(perm, np.uint32), np.asarray(head, np.uint8), np.asarray(weight, np.uint32)
    n = len(perm)
    size = guarded_u32(n)
    got, over = e.cluster_weights(dev(perm), dev(head), dev(weight), n, size, levels)
    got_sizes = split_guard(size, n)
    expect, expect_over = ref.weighted_sizes(perm.tolist(), head.tolist(), weight.tolist())
    assert expect_over is None and (over.over_record, over.over_sum) == (NO_RECORD, 0)
    assert got_sizes.tolist() == expect                      # (the fill is no size: every entry was written)
    if levels:
        clusters, records, largest = sizes.levels_of(expect)
        assert list(got.clusters) == clusters and list(got.records) == records and got.largest == largest and got.reserved == 0
        assert sum(records) == int(weight.astype(np.uint64).sum()) and sum(clusters) == int(head.sum())
    else:
        assert got is None
    return got_sizes


def random_weights(rng, n):
    return rng.choice(np.array([1, 1, 1, 2, 3, 40, 999, 70000], np.uint32), n)


@pytest.mark.parametrize("n", base.NS)
def test_weighted_sizes_at_the_wave_block_and_tile_edges(n):
    rng = np.random.default_rng(100 + n)
    with Engine(segments=1) as e:
        if n == 0:
            got, over = e.cluster_weights(None, None, None, 0, None)
            assert list(got.clusters) == [0] * 16 and got.largest == 0 and over.over_record == NO_RECORD
            assert e.cluster_weights(None, None, None, 0, None, levels=False)[0] is None
            return
        ident, shuffled = np.arange(n, dtype=np.uint32), rng.permutation(n).astype(np.uint32)
        w = random_weights(rng, n)
        check_weights(e, ident, np.ones(n, np.uint8), w)                              # all singletons: the sizes are the weights
        check_weights(e, shuffled, np.ones(n, np.uint8), w)
        one = np.zeros(n, np.uint8); one[0] = 1
        check_weights(e, ident, one, w)                                               # one run of n
        check_weights(e, shuffled, one, w, levels=False)
        for p in (0.5, 0.1, 0.01):
            head = (rng.random(n) < p).astype(np.uint8); head[0] = 1
            check_weights(e, shuffled, head, random_weights(rng, n))
            # all weights 1: fqd_cluster_sizes' output
            plain = guarded_u32(n)
            lv = e.cluster_sizes(dev(shuffled), dev(head), n, plain)
            ones = check_weights(e, shuffled, head, np.ones(n, np.uint32))
            assert ones.tolist() == split_guard(plain, n).tolist()
            got = e.cluster_weights(dev(shuffled), dev(head), dev(np.ones(n, np.uint32)), n, guarded_u32(n))[0]
            assert (list(got.clusters), list(got.records), got.largest) == (list(lv.clusters), list(lv.records), lv.largest)
        last = np.zeros(n, np.uint8); last[0] = 1; last[n - 1] = 1                    # a singleton on the last place
        check_weights(e, shuffled, last, w)


def test_weighted_runs_that_begin_on_a_tiles_last_place_and_on_its_first():
    n = 3 * TILE + 10
    rng = np.random.default_rng(51)
    perm = rng.permutation(n).astype(np.uint32)
    with Engine(segments=1) as e:
        for places in ([TILE - 1], [TILE], [TILE - 1, TILE], [TILE - 1, 2 * TILE], [TILE, 2 * TILE - 1, 3 * TILE], [3 * TILE - 1, 3 * TILE, n - 1]):
            head = np.zeros(n, np.uint8); head[0] = 1; head[places] = 1
            check_weights(e, perm, head, random_weights(rng, n))


def test_a_weighted_run_over_tiles_without_a_head_between_singletons():
    run = 3 * TILE + 5                                       # 6149
    for front in (100, TILE - 1, TILE):
        head = np.concatenate([np.ones(front, np.uint8), [1], np.zeros(run - 1, np.uint8), np.ones(100, np.uint8)])
        n = len(head)
        rng = np.random.default_rng(front)
        perm, w = rng.permutation(n).astype(np.uint32), random_weights(rng, n)
        with Engine(segments=1) as e:
            got = check_weights(e, perm, head, w)
        assert got[perm[front]] == int(w[perm[front:front + run]].astype(np.uint64).sum())


def test_every_level_edge_is_reached_by_weight():
    edges = [9, 10, 49, 50, 99, 100, 499, 500, 999, 1000, 4999, 5000, 9999, 10000, ref.MAX]
    rng = np.random.default_rng(52)
    runs = []                                                 # (members' weights): two or three records that add up to an edge, and small ones
    for s in edges:
        a = int(rng.integers(1, s - 1))
        runs.append([a, s - a] if s % 2 else [a, 1, s - a - 1])
    runs += [[1]] * 300 + [[1, 1]] * 20 + [[2]] * 7 + [[3, 5]] * 3
    order = rng.permutation(len(runs))
    head = np.concatenate([[1] + [0] * (len(runs[k]) - 1) for k in order]).astype(np.uint8)
    in_place = np.concatenate([runs[k] for k in order]).astype(np.uint32)
    n = len(head)
    perm = rng.permutation(n).astype(np.uint32)
    weight = np.zeros(n, np.uint32); weight[perm] = in_place
    with Engine(segments=1) as e:
        got = check_weights(e, perm, head, weight)
    clusters, records, largest = sizes.levels_of(got.tolist())
    assert largest == ref.MAX and clusters[9:] == [2, 2, 2, 2, 2, 2, 2] and clusters[8] == 1 and clusters[7] == 3
    assert max(len(r) for r in runs) == 3                     # no run reaches its level by its members' number


def test_a_second_round_of_the_carry_kernel():
    n = 1025 * TILE + 3                                       # 1026 tile values: more than the carry's one block takes at once
    rng = np.random.default_rng(53)
    head = (rng.random(n) < 0.3).astype(np.uint8); head[0] = 1
    head[1023 * TILE - 5:1025 * TILE + 2] = 0                 # a run across the round's edge, over a tile without a head
    perm = rng.permutation(n).astype(np.uint32)
    weight = random_weights(rng, n)
    starts = np.flatnonzero(head)
    sums = np.add.reduceat(weight[perm].astype(np.uint64), starts)                       # the statement, vectorised for this size
    expect = np.zeros(n, np.uint64); expect[perm[starts]] = sums
    assert sums.max() < ref.MAX and np.diff(np.append(starts, n)).max() > 2 * TILE
    size = guarded_u32(n)
    with Engine(segments=1) as e:
        got, over = e.cluster_weights(dev(perm), dev(head), dev(weight), n, size)
    assert over.over_record == NO_RECORD
    assert np.array_equal(split_guard(size, n).astype(np.uint64), expect)
    assert sum(got.records) == int(weight.astype(np.uint64).sum()) and sum(got.clusters) == len(starts) and got.largest == int(sums.max())


def test_runs_above_the_limit_are_reported_with_their_exact_sum():
    run = 3 * TILE + 5
    rng = np.random.default_rng(54)
    with Engine(segments=1) as e:
        # one run of 6149 records of weight 2^31-1 between singletons
        head = np.concatenate([np.ones(51, np.uint8), np.zeros(run - 1, np.uint8), np.ones(30, np.uint8)])
        n = len(head)
        perm = rng.permutation(n).astype(np.uint32)
        weight = np.ones(n, np.uint32); weight[perm[50:50 + run]] = ref.MAX
        size = guarded_u32(n)
        lv, over = e.cluster_weights(dev(perm), dev(head), dev(weight), n, size)
        assert (over.over_record, over.over_sum) == (int(perm[50]), run * ref.MAX) and over.over_sum > 2 ** 43
        assert ref.weighted_sizes(perm.tolist(), head.tolist(), weight.tolist())[1] == (int(perm[50]), run * ref.MAX)
        assert list(lv.clusters) == [0] * 16 and lv.largest == 0
        split_guard(size, n)
        # two such runs: the lower record at a head place is named, wherever its run stands
        for flip in (False, True):
            head = np.zeros(5000, np.uint8); head[[0, 10, 2500, 2502, 4000]] = 1
            perm = rng.permutation(5000).astype(np.uint32)
            a, b = int(perm[10]), int(perm[2500])
            if (a > b) != flip:
                perm[[10, 2500]] = perm[[2500, 10]]
            weight = np.ones(5000, np.uint32); weight[perm[11]] = ref.MAX; weight[perm[2501]] = ref.MAX - 1; weight[perm[2500]] = 2
            _, over = e.cluster_weights(dev(perm), dev(head), dev(weight), 5000, guarded_u32(5000), levels=False)
            expect = ref.weighted_sizes(perm.tolist(), head.tolist(), weight.tolist())[1]
            assert (over.over_record, over.over_sum) == expect and over.over_record == min(int(perm[10]), int(perm[2500]))
        # exactly 2^31-1 is a size
        head = np.array([1, 0, 1], np.uint8)
        got = check_weights(e, [2, 0, 1], head, [1, 7, ref.MAX - 1])
        assert got.tolist() == [0, 7, ref.MAX]


def test_weights_misuse_is_refused():
    n = 300
    perm = dev(np.arange(n, dtype=np.uint32))
    ones8, ones32 = np.ones(n, np.uint8), np.ones(n, np.uint32)
    head = ones8.copy(); head[0] = 0
    size = guarded_u32(n)
    with Engine(segments=1) as e:
        with pytest.raises(FqdError, match="fqd_cluster_weights.*head\\[0\\]") as ei:
            e.cluster_weights(perm, dev(head), dev(ones32), n, size)
        assert ei.value.code == _lib.ERR_ARG
        e.sync()
        assert np.all(host_u32(size) == base.FILL32)         # nothing was written to size
        for at in (0, 63, 64, n - 1):                        # a weight of 0, wherever it stands
            w = ones32.copy(); w[at] = 0
            with pytest.raises(FqdError, match="fqd_cluster_weights.*weight 0") as ei:
                e.cluster_weights(perm, dev(ones8), dev(w), n, guarded_u32(n))
            assert ei.value.code == _lib.ERR_ARG
        for args in ((perm, dev(ones8), dev(ones32), 2 ** 31, size), (perm, ones8, dev(ones32), n, size), (perm, dev(ones8), ones32, n, size),
                     (perm, dev(ones8), None, n, size)):
            with pytest.raises(FqdError, match="fqd_cluster_weights") as ei:
                e.cluster_weights(*args)
            assert ei.value.code == _lib.ERR_ARG
        with pytest.raises(FqdError, match="fqd_cluster_weights") as ei:                 # info is not optional
            e.cluster_weights(perm, dev(ones8), dev(ones32), n, size, info=None)
        assert ei.value.code == _lib.ERR_ARG
        assert np.all(host_u32(size) == base.FILL32)


# ---------------------------------------------------------------- fqd_size_relabel, fqd_copy_relabelled

def spans():
    """[(record bytes or None for a span that is not written, label_at, cut, size)]: parts of 1, 15, 16, 17 bytes on both
    sides, cuts of 0, 7 and 16 bytes against labels shorter than, as long as and longer than the cut."""
    rng = np.random.default_rng(61)
    out = []

    def rec(k):
        return rng.integers(33, 127, k, dtype=np.uint8).tobytes()

    labels = {0: [5, 4294967295], 7: [3, 42, 1234567890], 16: [9, 1000000000, 77777]}      # 7 = ";size=3", 16 = ";size=1000000000"
    for cut, size_list in labels.items():
        k = 0
        for at in (1, 15, 16, 17, 40):
            for tail in (0, 1, 15, 16, 17, 300):
                out.append((rec(at + cut + tail), at, cut, size_list[k % len(size_list)]))
                k += 1
                if (at + tail) % 2:
                    out.append((None, 0, 0, 0))               # spans that are not written in between
    for at, cut, tail in ((1, 7, 1), (2, 7, 3), (1, 0, 4), (3, 7, 0), (128, 16, 128), (300, 7, 1)):      # short records, long parts
        out.append((rec(at + cut + tail), at, cut, 21))
    out.append((None, 5, 7, 77))
    out.append((rec(16 + 7 + 300), 16, 7, 123))              # the last source byte ends with its allocation
    return out


def span_arrays(sp):
    src = b"".join(r for r, _, _, _ in sp if r is not None)
    src_off, lens, label_at, cut, size, parts, at = [], [], [], [], [], [], 0
    for r, a, c, s in sp:
        src_off.append(at if r is not None else len(src) - 1)
        label_at.append(a); cut.append(c); size.append(s)
        if r is None:
            lens.append(0); parts.append(b"")
            continue
        parts.append(r[:a] + sizes.label(s) + r[a + c:])
        lens.append(len(parts[-1]))
        at += len(r)
    lens = np.array(lens, np.uint32)
    dst_off = np.zeros(len(sp), np.uint64)
    dst_off[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
    return src, np.array(src_off, np.uint64), lens, np.array(label_at, np.uint32), np.array(cut, np.uint32), np.array(size, np.uint32), dst_off, parts


def test_the_spans_cover_the_cases():
    sp = [s for s in spans() if s[0] is not None]
    for cut in (0, 7, 16):
        labs = {len(sizes.label(s)) for _, _, c, s in sp if c == cut}
        assert (cut == 0 or cut in labs) and any(x > cut for x in labs) == (cut < 16) and any(x < cut for x in labs) == (cut == 16)


def test_grown_sizes_without_the_annotation():
    sp = spans()
    _, _, lens, _, cut, size, _, _ = span_arrays(sp)
    n = len(sp)
    rec_size = np.array([len(r) if r is not None else 40 for r, _, _, _ in sp], np.uint32)
    keep = np.array([r is not None for r, _, _, _ in sp], np.uint8)
    out_size = guarded_u32(n)
    with Engine(segments=1) as e:
        e.size_relabel(dev(rec_size), dev(keep), dev(size), dev(cut), n, out_size)
        got = split_guard(out_size, n)
        assert got.tolist() == [int(lens[i]) if keep[i] else 40 for i in range(n)]
        bad = size.copy(); bad[0] = 0                         # a kept record of size 0
        with pytest.raises(FqdError, match="fqd_size_relabel.*size 0") as ei:
            e.size_relabel(dev(rec_size), dev(keep), dev(bad), dev(cut), n, out_size)
        assert ei.value.code == _lib.ERR_ARG
        with pytest.raises(FqdError, match="fqd_size_relabel") as ei:                    # a host pointer
            e.size_relabel(rec_size, dev(keep), dev(size), dev(cut), n, out_size)
        assert ei.value.code == _lib.ERR_ARG
        e.size_relabel(None, None, None, None, 0, None)


def test_the_relabelled_copy_byte_for_byte():
    sp = spans()
    src, src_off, lens, label_at, cut, size, dst_off, parts = span_arrays(sp)
    expect = b"".join(parts)
    n = len(sp)
    d_src = dev(np.frombuffer(src, np.uint8))                # exactly as long as the records
    dst = torch.full((PAD + len(expect) + PAD,), FILL8, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        e.copy_relabelled(d_src, dev(src_off), dev(lens), dev(label_at), dev(cut), dev(size), n, dst.data_ptr() + PAD, dev(dst_off))
        e.sync()
        got = dst.cpu().numpy().tobytes()
        assert got[PAD:PAD + len(expect)] == expect
        assert got[:PAD] == bytes([FILL8]) * PAD and got[PAD + len(expect):] == bytes([FILL8]) * PAD
        # cut = 0 everywhere is fqd_copy_labelled
        zero = np.zeros(n, np.uint32)
        plain = [b"" if r is None else r[:a] + sizes.label(s) + r[a:] for r, a, _, s in sp]
        plens = np.array([len(x) for x in plain], np.uint32)
        poff = np.zeros(n, np.uint64); poff[1:] = np.cumsum(plens.astype(np.uint64))[:-1]
        a, b = (torch.full((int(plens.sum()) + PAD,), FILL8, dtype=torch.uint8, device="cuda") for _ in range(2))
        e.copy_relabelled(d_src, dev(src_off), dev(plens), dev(label_at), dev(zero), dev(size), n, a, dev(poff))
        e.copy_labelled(d_src, dev(src_off), dev(plens), dev(label_at), dev(size), n, b, dev(poff))
        e.sync()
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == b"".join(plain) + bytes([FILL8]) * PAD
        e.copy_relabelled(None, None, None, None, None, None, 0, None, None)
        with pytest.raises(FqdError, match="fqd_copy_relabelled") as ei:
            e.copy_relabelled(d_src, dev(src_off), dev(lens), dev(label_at), None, dev(size), n, dst.data_ptr() + PAD, dev(dst_off))
        assert ei.value.code == _lib.ERR_ARG


@pytest.mark.parametrize("a,b", [(0, 9), (9, 41), (41, None), (8, 9)])
def test_a_window_with_advanced_pointers(a, b):
    sp = spans()
    src, src_off, lens, label_at, cut, size, dst_off, parts = span_arrays(sp)
    b = len(sp) if b is None else b
    lo = int(dst_off[a])
    want = b"".join(parts[a:b])
    win = torch.full((PAD + len(want) + PAD,), FILL8, dtype=torch.uint8, device="cuda")
    with Engine(segments=1) as e:
        e.copy_relabelled(dev(np.frombuffer(src, np.uint8)), dev(src_off)[a:], dev(lens)[a:], dev(label_at)[a:], dev(cut)[a:], dev(size)[a:], b - a,
                          win.data_ptr() + PAD - lo, dev(dst_off)[a:])
        e.sync()
    got = win.cpu().numpy().tobytes()
    assert got[PAD:PAD + len(want)] == want
    assert got[:PAD] == bytes([FILL8]) * PAD and got[PAD + len(want):] == bytes([FILL8]) * PAD
