"""Plain-Python restatement of FQD_SEQ_KEEP=best on top of tests/seq_reference.py: the score of a record, the
representative of a cluster and the outputs of a run, the yardstick of fqd_seq_scores / fqd_seq_pick_best
(csrc/fqd_seq_pick.hip), of the core header's CPU harness and of the CLI.

- score: the sum of (b - 33) over the bytes b >= 33 of the record's last line without the '\\n', saturating at 2^32-1;
  a pair's score is the saturating sum of its mates'
- clusters: the runs of the sorted order that start at a head of seq_reference.heads (place 0 starts one)
- representative: the member with the highest score, the earliest place on a tie; the order entries of the head's
  place and the representative's place are swapped, everything else stays
"""
import seq_reference as ref

SAT = 2 ** 32 - 1


def last_line(rec: bytes) -> bytes:
    if rec.endswith(b"\n"):
        rec = rec[:-1]
    return rec[rec.rfind(b"\n") + 1:]


def score(rec: bytes) -> int:
    return min(SAT, sum(b - 33 for b in last_line(rec) if b >= 33))


def pair_score(recs) -> int:
    return min(SAT, sum(score(r) for r in recs))


def pick(order, head, scores):
    """order: the sorted order (record indices); head: flags per place; scores: per record (input order).
    Returns (the order after the swaps, the number of clusters whose entry at the head's place changed)."""
    order = list(order)
    n, moved, k = len(order), 0, 0
    while k < n:
        end = k + 1
        while end < n and not head[end]:
            end += 1
        best = max(range(k, end), key=lambda p: (scores[order[p]], -p))
        if best != k:
            order[k], order[best] = order[best], order[k]
            moved += 1
        k = end
    return order, moved


def dedup_best(inputs, mode=ref.TIGHT, distance=2):
    """ref.dedup for FASTQ with the best member of every cluster written: (outputs, clusters, total, duplicates, moved)."""
    files = [ref.parse(x, False) for x in inputs]
    n = min(len(f) for f in files)
    seqs = [tuple(f[i][2] for f in files) for i in range(n)]
    order = ref.sorted_order(seqs)
    h = ref.heads(mode, distance, [seqs[i] for i in order])
    scores = [pair_score([f[i][0] for f in files]) for i in range(n)]
    order, moved = pick(order, h, scores)
    outputs, clusters = [], []
    for f in files:
        outputs.append(b"".join(f[i][0] for i, keep in zip(order, h) if keep))
        clusters.append(b"".join((b"" if keep else b"--") + f[i][1] for i, keep in zip(order, h)))
    return outputs, clusters, n, n - sum(h), moved
