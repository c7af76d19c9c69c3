"""GPU checks of FQD_SEQ_KEEP=best's primitives (fqd_seq_scores, fqd_seq_pick_best: csrc/fqd_seq_pick.hip) through
ctypes, against the plain-Python rule (tests/seq_keep_reference.py).

- fqd_seq_scores: quality lines of 0 to 300 bytes ending at every place of a word, records starting at every offset
  mod 8 (the first at the very start of the text), CRLF, bytes below 33 and above 126, a '+' line that repeats the ID,
  single-line records, pairs whose mates differ in length
- fqd_seq_pick_best on hand-made scores and head flags: clusters of 1 to 257 members, one of 70 000 over many
  workgroups with its best member first, last and on both sides of a tile boundary and singletons right behind it, equal
  scores (nothing moves), several maxima (the earliest), n = 0 and n = 1, bad arguments.  perm must come back exactly as
  the restatement leaves it, so every entry outside the swapped pairs is untouched."""
import random

import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine
from fastq_dupaway_amd._lib import FqdError
import seq_keep_reference as keep

pytestmark = pytest.mark.gpu
TILE = 2048                                                  # places per workgroup of the pick (kPickTile)


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_u32(t, n):
    return t.cpu().numpy().view(np.uint32)[:n]


def spans(recs):
    lens = np.array([len(r) for r in recs], dtype=np.uint32)
    offs = np.zeros(len(recs), np.uint64)
    offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    data = np.frombuffer(b"".join(recs) + b"\0" * 16, dtype=np.uint8).copy()
    return data, offs, lens


def quality(rng, q, crlf):
    body = bytes(rng.choice([33, 34, 40, 73, 126, 127, 200, 255, 32, 13, 11, 1]) if rng.random() < 0.3 else rng.randrange(33, 75) for _ in range(q))
    return body + (b"\r" if crlf else b"")


def score_records(rng):
    recs = []
    for q in (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 300):
        for idl in range(9):
            crlf = idl % 3 == 2
            eol = b"\r\n" if crlf else b"\n"
            ident = b"r" * idl
            plus = b"+" + (ident if idl % 2 else b"")        # the '+' line repeats the ID in every other record
            recs.append(b"@" + ident + eol + b"ACGT"[:q % 5] + eol + plus + eol + quality(rng, q, crlf) + b"\n")
    recs += [b"\n", b"II\n", b"~" * 64 + b"\n", b"@a\nAC\n+\n\n", b"@a\nAC\n+\n\r\n"]   # single lines, empty quality lines
    return recs


def test_scores_single_end():
    rng = random.Random(5)
    recs = score_records(rng)
    data, offs, lens = spans(recs)
    assert {int(o) % 8 for o in offs} == set(range(8)) and offs[0] == 0
    n = len(recs)
    score = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    with Engine(segments=1) as e:
        e.seq_scores((dev(data), dev(offs), dev(lens), n), score)
    assert host_u32(score, n).tolist() == [keep.score(r) for r in recs]


def test_scores_pairs_with_mates_of_different_lengths():
    rng = random.Random(6)
    one = score_records(rng)
    two = score_records(rng)
    rng.shuffle(two)                                         # a mate 1 of 300 beside a mate 2 of 0, and so on
    n = len(one)
    d1, o1, l1 = spans(one)
    d2, o2, l2 = spans(two)
    score = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    with Engine(segments=2) as e:
        e.seq_scores((dev(d1), dev(o1), dev(l1), n), score, (dev(d2), dev(o2), dev(l2), n))
    assert host_u32(score, n).tolist() == [keep.pair_score([a, b]) for a, b in zip(one, two)]


def run_pick(e, scores, head, perm):
    """scores per record (input order), head per place, perm = the order; returns (perm afterwards, moved)."""
    n = len(perm)
    d_perm = dev(np.asarray(perm, np.uint32)) if n else torch.empty(0, dtype=torch.int32, device="cuda")
    d_score = dev(np.asarray(scores, np.uint32)) if n else torch.empty(0, dtype=torch.int32, device="cuda")
    d_head = dev(np.asarray(head, np.uint8)) if n else torch.empty(0, dtype=torch.uint8, device="cuda")
    moved = e.seq_pick_best(d_score, d_head, n, d_perm)
    return host_u32(d_perm, n).tolist(), moved


def check_pick(e, rng, sizes, place_scores):
    """Clusters of the given sizes in this order; place_scores[k] = the score of the record at sorted place k.  The
    order is a random permutation, so the scores are gathered through it."""
    n = sum(sizes)
    head = np.zeros(n, np.uint8)
    head[np.cumsum([0] + sizes[:-1])] = 1
    perm = list(range(n))
    rng.shuffle(perm)
    scores = [0] * n
    for k, r in enumerate(perm):
        scores[r] = place_scores[k]
    got, moved = run_pick(e, scores, head, perm)
    exp, exp_moved = keep.pick(perm, head.tolist(), scores)
    assert got == exp
    assert moved == exp_moved
    return moved


@pytest.fixture(scope="module")
def engine():
    with Engine(segments=1) as e:
        yield e


def test_pick_small_clusters(engine):
    rng = random.Random(7)
    sizes = [1, 2, 3, 63, 64, 65, 255, 256, 257] * 3 + [1] * 50 + [2] * 50
    rng.shuffle(sizes)
    n = sum(sizes)
    for pool in ([0, 1, 2, 3], [5, 2 ** 32 - 1, 2 ** 32 - 2, 0], None):     # many ties; the largest scores; hardly any tie
        place_scores = [rng.choice(pool) if pool else rng.randrange(2 ** 32) for _ in range(n)]
        assert check_pick(engine, rng, sizes, place_scores) > 0


@pytest.mark.parametrize("where", ["first", "last", "tile_start", "tile_end", "ties"])
def test_pick_one_cluster_over_many_workgroups(engine, where):
    rng = random.Random(8)
    big = 70_000
    sizes = [3, 1, 300] + [big] + [1] * 40 + [2, 5, 1]       # the big cluster starts at place 304, singletons right behind it
    start = 304
    n = sum(sizes)
    place_scores = [rng.randrange(1000) for _ in range(n)]
    at = {"first": start, "last": start + big - 1, "tile_start": 20 * TILE, "tile_end": 20 * TILE - 1, "ties": None}[where]
    if at is None:
        for p in (start + 5000, 9 * TILE, 9 * TILE - 1, start + big - 1):   # several maxima: the earliest wins
            place_scores[p] = 5000
    else:
        place_scores[at] = 5000
    moved = check_pick(engine, rng, sizes, place_scores)
    assert moved >= (0 if where == "first" else 1)


def test_pick_equal_scores_move_nothing(engine):
    rng = random.Random(9)
    sizes = [1, 2, 3, 65, 257, 5000, 1, 1]
    n = sum(sizes)
    for value in (0, 77, 2 ** 32 - 1):
        assert check_pick(engine, rng, sizes, [value] * n) == 0


def test_pick_head_flag_of_place_0_may_be_clear(engine):
    # place 0 starts a cluster whatever its flag says
    got, moved = run_pick(engine, [1, 9, 3, 4], [0, 0, 1, 0], [0, 1, 2, 3])
    assert got == [1, 0, 3, 2] and moved == 2


def test_pick_empty_and_single(engine):
    assert run_pick(engine, [], [], []) == ([], 0)
    assert run_pick(engine, [12], [1], [0]) == ([0], 0)


def test_bad_arguments_are_refused(engine):
    one = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(FqdError, match="fqd_seq_pick_best"):
        engine.seq_pick_best(one, None, 4, one)
    with pytest.raises(FqdError, match="fqd_seq_scores"):
        engine.seq_scores((one, one, one, 4), None)
