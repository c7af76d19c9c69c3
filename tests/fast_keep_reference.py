"""Plain-Python restatement of FQD_FAST_KEEP / FQD_FAST_CLUSTERS of the `--fast` mode: the yardstick of
tests/test_fast_keep_cli.py and of the pick in tests/test_gpu_owners.py.

- a cluster = the records (pairs) with identical sequences, lengths included, over both mates; clusters stand in the
  order of their first member in the input, members in input order
- first: the first member is written.  best: the member with the highest score, the earliest on a tie, is written at
  its own place in the input; in the cluster list it changes places with the first member
- score of a record: the sum of (b - 33) over the bytes b >= 33 of its last line, saturating at 2^32-1; of a pair: the
  saturating sum of its mates'
- `<output>.clusters`: per cluster the ID line of the written record, then "--" + the ID line of every other member
"""
SAT = 2 ** 32 - 1


def parse(data: bytes, fasta: bool):
    """[(record bytes, ID line with '\\n', sequence without '\\n')] of the whole records of data."""
    per = 2 if fasta else 4
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    out = []
    for k in range(0, len(lines) - per + 1, per):
        rec = b"".join(x + b"\n" for x in lines[k:k + per])
        out.append((rec, lines[k] + b"\n", lines[k + 1]))
    return out


def score(rec: bytes) -> int:
    body = rec[:-1] if rec.endswith(b"\n") else rec
    return min(SAT, sum(b - 33 for b in body[body.rfind(b"\n") + 1:] if b >= 33))


def clusters_of(keys):
    """keys: one hashable per record (pair).  The clusters, each a list of indices in input order, ordered by first member."""
    groups = {}
    for i, k in enumerate(keys):
        groups.setdefault(k, []).append(i)
    return list(groups.values())                             # dicts keep insertion order: by first member


def pick(members, scores):
    """The written member of a cluster under `best`: the highest score, the earliest index on a tie."""
    return max(members, key=lambda i: (scores[i], -i))


def restate_pick(perm, head, scores):
    """What fqd_seq_pick_best does to an order grouped by owner: per run the best member changes places with the first."""
    perm = list(perm)
    n, k, moved = len(perm), 0, 0
    while k < n:
        end = k + 1
        while end < n and not head[end]:
            end += 1
        best = max(range(k, end), key=lambda p: (scores[perm[p]], -p))
        if best != k:
            perm[k], perm[best] = perm[best], perm[k]
            moved += 1
        k = end
    return perm, moved


def dedup(inputs, fasta=False, best=False):
    """inputs: file contents (1 or 2).  Returns (outputs, cluster files, total, duplicates, clusters whose member changed)."""
    files = [parse(x, fasta) for x in inputs]
    n = len(files[0])
    assert all(len(f) == n for f in files)
    groups = clusters_of([tuple(f[i][2] for f in files) for i in range(n)])
    scores = [min(SAT, sum(score(f[i][0]) for f in files)) for i in range(n)]
    written, moved, listing = set(), 0, []
    for g in groups:
        w = pick(g, scores) if best else g[0]
        moved += w != g[0]
        written.add(w)
        order = list(g)
        at = order.index(w)
        order[0], order[at] = order[at], order[0]             # the written member and the first change places
        listing.append(order)
    outputs = [b"".join(f[i][0] for i in range(n) if i in written) for f in files]
    cluster_files = [b"".join((b"" if k == 0 else b"--") + f[i][1] for order in listing for k, i in enumerate(order)) for f in files]
    return outputs, cluster_files, n, n - len(groups), moved
