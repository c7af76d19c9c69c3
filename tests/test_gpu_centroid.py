"""fqd_subcluster_sizes and fqd_subcluster_scores (csrc/fqd_centroid.hip) through the binding, exactly against the sequential
statement (tests/centroid_reference.py): every abundance, every field of the info, the centroid fqd_seq_pick_best makes of
them, the masked scores and the member the second pick takes; nothing written behind the last entry.
Run lengths round the kernels' classes (one member, eight lanes, a wave, a workgroup's table in LDS, the table in scratch),
each at, across and up to a scan tile's edge and as the last run; the label patterns of tests/centroid_cases.py, with THE SAME
LABEL VALUES IN SEVERAL RUNS of every class — the shape an optical split leaves, which a counter per label alone gets wrong;
weights whose sums pass 2^32; all classes in one call, once inside a guarded arena.  Misuse: each case FQD_ERR_ARG."""
import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, _lib
from fastq_dupaway_amd._lib import FqdError
import centroid_reference as ref
from centroid_cases import PATTERNS, W_MAX, layout, pattern
from guarded_arena import Arena, to_torch_bits

pytestmark = pytest.mark.gpu
GUARD = 8                                                      # entries behind the last one of every output array
NONE32 = 0xFFFFFFFF
LIMIT = _lib.CENTROID_BLOCK_LIMIT
LENGTHS = [1, 2, 7, 8, 9, 63, 64, 65, LIMIT - 1, LIMIT, LIMIT + 1, 3 * LIMIT + 17]


def dev(a):
    return to_torch_bits(a).cuda()


def host(t, dtype=np.uint32):
    return t.cpu().numpy().view(dtype)


def check_sizes(e, perm, head, label, weight, want_info=True):
    """One call against the statement; returns (the abundances on the device, the statement's)."""
    n = len(perm)
    d_perm, d_head, d_label = dev(perm), dev(head), dev(label)
    d_weight = None if weight is None else dev(weight)
    out = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    got = e.subcluster_sizes(d_perm, d_head, d_label, n, out, d_weight, info=want_info)
    want, _, info = ref.abundances(perm, head, label, weight)
    a = host(out)
    assert np.all(a[n:] == NONE32)                             # nothing behind the last entry
    bad = np.nonzero(a[:n] != want)[0]
    assert bad.size == 0, (bad[:10], a[bad[:10]], want[bad[:10]])
    if want_info:
        assert dict(clusters=got.clusters, mixed=got.mixed, subclusters=got.subclusters, tier_clusters=list(got.tier_clusters), largest=got.largest) == info
        assert got.reserved == 0
    else:
        assert got is None
    return (d_perm, d_head, d_label, out), want


def check_picks(e, perm, head, label, weight, on_device, abundance, score):
    """The centroid's pick, the masked scores and the second pick against the statement."""
    n = len(perm)
    d_perm, d_head, d_label, d_abundance = on_device
    order = d_perm.clone()
    moved = e.seq_pick_best(d_abundance, d_head, n, order)
    want_order, want_moved = ref.pick(perm, head, abundance)
    assert moved == want_moved
    assert np.array_equal(host(order), want_order)
    heads = np.nonzero(head)[0]
    assert [int(r) for r in want_order[heads]] == ref.written(perm, head, label, weight, stored=abundance)
    masked = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    e.subcluster_scores(order, d_head, d_label, dev(score), n, masked)
    want_masked = ref.masked_scores(want_order, head, label, score)
    m = host(masked)
    assert np.all(m[n:] == NONE32)
    assert np.array_equal(m[:n], want_masked)
    e.seq_pick_best(masked, d_head, n, order)
    best_order, _ = ref.pick(want_order, head, want_masked)
    assert np.array_equal(host(order), best_order)
    assert [int(r) for r in best_order[heads]] == ref.written(perm, head, label, weight, score, stored=abundance)
    return want_moved


def scores_for(rng, n):
    score = rng.integers(0, 40, n).astype(np.uint32)           # (few values: ties inside every sub-cluster)
    score[rng.integers(0, n, max(1, n // 7))] = 0xFFFFFFFF
    score[rng.integers(0, n, max(1, n // 7))] = 0xFFFFFFFE
    return score


@pytest.mark.parametrize("s", LENGTHS)
def test_every_pattern_at_every_tile_edge(s):
    """A run of s members of every pattern at, across and up to a tile edge, and — every pattern in turn — as the last run.  The
    patterns share two label values, so every one of them stands in a dozen runs of this size class."""
    rng = np.random.default_rng(s)
    a, b = 11, 11 + s + 7
    with Engine(segments=1) as e:
        for last in PATTERNS if 1 < s <= 64 else PATTERNS[:1]:
            runs = [pattern(name, s, a, b) + (where,) for name in PATTERNS for where in ("at", "across", "upto")]
            runs.append(pattern(last, s, a, b) + (None,))
            perm, head, label, weight, _ = layout(runs, rng)
            for given in (weight, None) if last == PATTERNS[0] else (weight,):
                on_device, want = check_sizes(e, perm, head, label, given)
                moved = check_picks(e, perm, head, label, given, on_device, want, scores_for(rng, len(perm)))
                if s >= 5:                                         # the two ties behind a lone member and, weighted, last_alone: three places each
                    assert moved >= (9 if given is not None else 6)


def test_the_same_label_in_runs_of_every_class():
    """One label value in runs of 1, 5, 40, 300 and 5000 members, twice each, beside other labels: the sub-clusters are cut to
    their runs."""
    runs = []
    for s in (1, 5, 40, 300, LIMIT + 2952) * 2:
        labels = [7 if i % 3 else 9 for i in range(s)]             # a third 9, two thirds 7 — but the first member holds 9
        runs.append((labels, None, None))
    perm, head, label, weight, _ = layout(runs, np.random.default_rng(3))
    with Engine(segments=1) as e:
        on_device, want = check_sizes(e, perm, head, label, None)
        assert check_picks(e, perm, head, label, None, on_device, want, scores_for(np.random.default_rng(4), len(perm))) == 8
    per_label = np.bincount(label, minlength=10)
    assert per_label[7] > int(want.max())                          # a counter per label alone would say more than any run holds


@pytest.mark.parametrize("s", [40, 300, 2 * LIMIT + 5])
def test_weights_whose_sum_passes_2_to_the_32(s):
    """Three members of 2^31 - 1 in one sub-cluster (saturated), two in another (2^32 - 2: not saturated), in the wave, LDS and
    scratch classes; the run's other members weigh 1."""
    labels = [5 + i for i in range(s)]
    weights = [1] * s
    for i in (1, s // 2, s - 1):
        labels[i], weights[i] = 3, W_MAX
    for i in (2, s - 2):
        labels[i], weights[i] = 4, W_MAX
    perm, head, label, weight, _ = layout([([1], None, None), (labels, weights, "across"), (labels, weights, None)], np.random.default_rng(s))
    with Engine(segments=1) as e:
        on_device, want = check_sizes(e, perm, head, label, weight)
        assert sorted(set(want.tolist()))[-2:] == [0xFFFFFFFE, 0xFFFFFFFF]
        assert check_picks(e, perm, head, label, weight, on_device, want, scores_for(np.random.default_rng(1), len(perm))) == 2


def mixed_runs(rng):
    runs = []
    for s in [1] * 40 + [2, 3, 8] * 6 + [9, 30, 64] * 3 + [65, 700, LIMIT] * 2 + [LIMIT + 1, 2 * LIMIT + 100]:
        labels = rng.integers(0, max(1, min(s, 5)), s) + 20        # up to five sub-clusters, the same values in every run
        runs.append((labels.tolist(), rng.integers(1, 9, s).tolist() if s % 2 else None, None))
    rng.shuffle(runs)
    return runs


def test_all_classes_in_one_call_and_the_info():
    rng = np.random.default_rng(8)
    perm, head, label, weight, _ = layout(mixed_runs(rng), rng)
    with Engine(segments=1) as e:
        for given in (weight, None):
            on_device, want = check_sizes(e, perm, head, label, given)
            check_picks(e, perm, head, label, given, on_device, want, scores_for(rng, len(perm)))
        check_sizes(e, perm, head, label, weight, want_info=False)
    _, _, info = ref.abundances(perm, head, label, weight)
    assert all(info["tier_clusters"]) and info["mixed"] > 20 and info["largest"] == 2 * LIMIT + 100


def big_grouping():
    """(perm, head, label) of 1024 tiles of 2048 places, one tile and three places more: clusters of one but for five mixed ones."""
    edge = 1024 * 2048
    n = edge + 2048 + 3
    # (first place, members): near the front; ending two places short of the round's edge; from there across that edge; 1000
    # places behind the edge; across the last tile's edge
    runs = [(100, 3), (edge - 2 - 40, 40), (edge - 2, 5), (edge + 1000, 300), (n - 9, 9)]
    perm = np.arange(n - 1, -1, -1, dtype=np.uint32)             # place k holds record n - 1 - k
    head = np.ones(n, np.uint8)
    label = np.arange(n, dtype=np.uint32)
    for at, m in runs:
        head[at + 1:at + m] = 0
        label[perm[at:at + m]] = np.where(np.arange(m) % 3 == 0, 5, 6)   # a third of the members under one label, the rest under another
    return perm, head, label


def test_more_places_than_the_tile_scans_first_round():
    """The one block that scans the head counts takes 1024 tiles of 2048 places a round: the smallest grouping that reaches the
    second round.  The four mixed clusters lie near the front, up to two places short of the round's edge, 1000 places behind
    it and across the last tile's edge; a fifth starts where the second ends and lies across the round's edge itself."""
    perm, head, label = big_grouping()
    with Engine(segments=1) as e:
        _, want = check_sizes(e, perm, head, label, None)
    assert sorted(set(want.tolist())) == [1, 2, 3, 6, 14, 26, 100, 200]   # every mixed cluster's two sub-clusters, and the ones


def test_a_mixed_call_inside_guards():
    """Every buffer of the two calls in one guarded arena: a store outside abundance or masked shows."""
    rng = np.random.default_rng(9)
    perm, head, label, weight, _ = layout(mixed_runs(rng), rng)
    n = len(perm)
    score = scores_for(rng, n)
    A = Arena("cuda", 8 * (4 * n + 2 * 4096) + 65536, 0xA5)
    ins = {}
    for name, a in (("perm", perm), ("head", head), ("label", label), ("weight", weight), ("score", score)):
        ins[name] = A.take(name, a.dtype, n, "in")
        ins[name].copy_(to_torch_bits(a))
    abundance, masked = A.take("abundance", np.uint32, n, "out"), A.take("masked", np.uint32, n, "out")
    A.seal()
    with Engine(segments=1) as e:
        e.subcluster_sizes(ins["perm"], ins["head"], ins["label"], n, abundance, ins["weight"])
        e.subcluster_scores(ins["perm"], ins["head"], ins["label"], ins["score"], n, masked)
        e.sync()
    torch.cuda.synchronize()
    A.check()
    assert np.array_equal(host(abundance), ref.abundances(perm, head, label, weight)[0])
    assert np.array_equal(host(masked), ref.masked_scores(perm, head, label, score))


def test_misuse_is_refused_and_nothing_is_written():
    perm, head, label, weight, _ = layout([([3, 3, 4], None, None), ([5] * 70, None, None), ([6], None, None)])
    n = len(perm)
    with Engine(segments=1) as e:
        def refused(call, name):
            out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            with pytest.raises(FqdError, match=name) as err:
                call(out)
            assert err.value.code == _lib.ERR_ARG
            assert bool((out == -1).all())
        d_perm, d_head, d_label, d_score = dev(perm), dev(head), dev(label), dev(np.arange(n, dtype=np.uint32))
        no_head = head.copy(); no_head[0] = 0
        refused(lambda out: e.subcluster_sizes(d_perm, dev(no_head), d_label, n, out), "fqd_subcluster_sizes")
        refused(lambda out: e.subcluster_scores(d_perm, dev(no_head), d_label, d_score, n, out), "fqd_subcluster_scores")
        for at in (0, n - 1):
            far = label.copy(); far[at] = n
            refused(lambda out: e.subcluster_sizes(d_perm, d_head, dev(far), n, out), "fqd_subcluster_sizes")
        wild = perm.copy(); wild[5] = n
        refused(lambda out: e.subcluster_sizes(dev(wild), d_head, d_label, n, out), "fqd_subcluster_sizes")
        refused(lambda out: e.subcluster_scores(dev(wild), d_head, d_label, d_score, n, out), "fqd_subcluster_scores")
        # 2^31 records: refused before anything is allocated or launched (the arrays hold n entries only)
        before = torch.cuda.mem_get_info()[0]
        refused(lambda out: e.subcluster_sizes(d_perm, d_head, d_label, 1 << 31, out), "fqd_subcluster_sizes")
        refused(lambda out: e.subcluster_scores(d_perm, d_head, d_label, d_score, 1 << 31, out), "fqd_subcluster_scores")
        assert torch.cuda.mem_get_info()[0] >= before - (1 << 20)
        refused(lambda out: e.subcluster_sizes(d_perm, d_head, d_label, n, d_label), "fqd_subcluster_sizes")   # abundance = an input
        assert np.array_equal(host(d_label), label)
        refused(lambda out: e.subcluster_sizes(None, d_head, d_label, n, out), "fqd_subcluster_sizes")
        # no record: fine, and no launch touches the arrays
        out = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        got = e.subcluster_sizes(None, None, None, 0, out)
        assert (got.clusters, got.subclusters, got.largest, list(got.tier_clusters)) == (0, 0, 0, [0] * 5)
        e.subcluster_scores(None, None, None, None, 0, out)
        assert bool((out == -1).all())
        on_device, want = check_sizes(e, perm, head, label, None)   # the engine is as good as before
