"""Case builders for FQD_FAST_CENTROID=abundant: label patterns of one run, and layouts of runs over the places of an order.

A pattern gives the labels (and weights) of a run's members in order.  layout() deals records to runs — a run's members in
input order, the runs interleaved — and places chosen runs at, across and up to the scan's tile edges, with runs of one
member as filler."""
import numpy as np

TILE = 2048                                                    # places a block of the scans (csrc/fqd_record_scan.hpp: kOffTile)
W_MAX = 0x7FFFFFFF                                             # the largest weight FQD_FAST_SIZEIN reads

PATTERNS = ("one", "different", "tie_first_earlier", "tie_first_later", "last_alone")


def pattern(name, s, a, b):
    """(labels, weights or None) of a run of s members; a, b: two label values, and a + 1 .. a + s are free to use.
    one: a single sub-cluster.  different: s sub-clusters of one member — the first member stays.  tie_first_earlier / _later:
    a lone member in front, then two sub-clusters of equal abundance interleaved, the one that starts earlier holding the lower
    / the higher label value — it wins either way.  last_alone: the last member alone outweighs the rest."""
    if name == "one" or s == 1:
        return [a] * s, None
    if name == "different":
        return [a + 1 + i for i in range(s)], None
    if name in ("tie_first_earlier", "tie_first_later"):
        lo, hi = (a, b) if a < b else (b, a)
        first, second = (lo, hi) if name == "tie_first_earlier" else (hi, lo)
        body = [first if i % 2 == 0 else second for i in range((s - 1) // 2 * 2)]
        lone = [a + 1 + i for i in range(s - len(body))]       # one member in front (two where s is even)
        return lone + body, None
    if name == "last_alone":
        return [a] * (s - 1) + [b], [3] * (s - 1) + [3 * (s - 1) + 1]
    raise ValueError(name)


def layout(runs, rng=None):
    """runs: a list of (labels, weights or None, where) with where in (None, "at", "across", "upto"): the run starts at a tile
    edge, lies across one, or ends on one; filler runs of one member are put in front as needed.  Returns perm, head, label,
    weight (uint32 by record; weight all 1 where no run gives one) and the place every given run starts at."""
    seq, starts, at = [], [], 0                                # seq: (labels, weights) of every run in order of place
    for labels, weights, where in runs:
        s = len(labels)
        if where is not None:
            want = {"at": 0, "across": -(s // 2) if s > 1 else 0, "upto": -s}[where]
            target = ((at - want + TILE - 1) // TILE) * TILE + want
            for _ in range(target - at):
                seq.append((None, None))
            at = target
        starts.append(at)
        seq.append((list(labels), None if weights is None else list(weights)))
        at += s
    n = at
    # records to places: a run's members ascending, the runs' records interleaved
    order = np.arange(n) if rng is None else rng.permutation(n)
    perm, head = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    label, weight = np.zeros(n, np.uint32), np.ones(n, np.uint32)
    k = 0
    for labels, weights in seq:
        s = 1 if labels is None else len(labels)
        recs = np.sort(order[k:k + s])
        perm[k:k + s] = recs
        head[k] = 1
        label[recs] = recs if labels is None else np.asarray(labels, np.uint64) % n
        if weights is not None:
            weight[recs] = weights
        k += s
    return perm, head, label, weight, starts
