"""The sequential statement of FQD_FAST_HAMMING=D (fastq-dupaway_amd/csrc/fqd_near_core.hpp), in plain Python: exact clusters by
(seq1, seq2), all pairs of them compared, union-find, owner = the lowest record.  Also the segment bounds and the seed hash of
the header, restated, so that a test can say which nodes share a seed group and how large the largest group of an input is."""
from collections import defaultdict

import numpy as np

MAX_GROUP = 4096
NO_RECORD = 0xFFFFFFFFFFFFFFFF
M64 = (1 << 64) - 1
MUL = 0x9E3779B97F4A7C15
MIX = 0xD6E8FEB86659FD93


# ---- the rule ------------------------------------------------------------------------------------------------------------------

def mismatches(a: bytes, b: bytes) -> int:
    assert len(a) == len(b)
    return sum(x != y for x, y in zip(a, b))


def near(a, b, D: int) -> bool:
    """a, b: nodes as tuples of mates (1 or 2 byte strings)."""
    if len(a) != len(b) or any(len(x) != len(y) for x, y in zip(a, b)):
        return False
    return all(mismatches(x, y) <= D for x, y in zip(a, b))


def exact_owners(records):
    """records: a list of tuples of mates.  owner[i] = the first record with record i's mates."""
    first = {}
    return np.array([first.setdefault(r, i) for i, r in enumerate(records)], np.uint32)


class UnionFind:
    def __init__(self, items):
        self.up = {x: x for x in items}

    def find(self, x):
        while self.up[x] != x:
            self.up[x] = self.up[self.up[x]]
            x = self.up[x]
        return x

    def join(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.up[max(a, b)] = min(a, b)                     # the root of a set is its lowest member


def merged_owners(records, D: int):
    """owner_out[i] = the first record of record i's merged cluster; also the nodes and the merged clusters."""
    owner = exact_owners(records)
    nodes = [i for i in range(len(records)) if owner[i] == i]
    uf = UnionFind(nodes)
    by_shape = defaultdict(list)
    for v in nodes:
        by_shape[tuple(len(m) for m in records[v])].append(v)
    for same in by_shape.values():
        arrays = [np.frombuffer(b"".join(records[v][m] for v in same), np.uint8).reshape(len(same), len(records[same[0]][m]))
                  for m in range(len(records[same[0]]))]
        for k in range(len(same)):
            ok = np.ones(len(same) - k - 1, bool)
            for a in arrays:
                ok &= (a[k + 1:] != a[k]).sum(axis=1) <= D
            for j in np.nonzero(ok)[0]:
                uf.join(same[k], same[k + 1 + j])
    out = np.array([uf.find(int(owner[i])) for i in range(len(records))], np.uint32)
    return out, len(nodes), len({int(x) for x in out})


# ---- segments and seeds, restated ---------------------------------------------------------------------------------------------------

def bound(length: int, D: int, j: int) -> int:
    return j * length // (D + 1)


def mix(h: int) -> int:
    h ^= h >> 32
    h = h * MIX & M64
    h ^= h >> 32
    h = h * MIX & M64
    return h ^ (h >> 32)


def absorb(h: int, w: int) -> int:
    h = (h ^ w) * MUL & M64
    return h ^ (h >> 29)


def seed_key(len1: int, len2: int, j: int, segment: bytes) -> int:
    h = mix(mix(len1 | len2 << 32) ^ ((j + 1) * MUL & M64))
    for k in range(0, len(segment), 8):
        h = absorb(h, int.from_bytes(segment[k:k + 8], "little"))
    return mix(h)


def node_seeds(node, D: int, weak: bool = False):
    m1 = node[0]
    len2 = len(node[1]) if len(node) > 1 else 0
    keys = [seed_key(len(m1), len2, j, m1[bound(len(m1), D, j):bound(len(m1), D, j + 1)]) for j in range(D + 1)]
    return [k & 15 for k in keys] if weak else keys


def seed_groups(records, D: int, weak: bool = False):
    """key -> the nodes (first records) of its entries, a node once for every entry it has there."""
    owner = exact_owners(records)
    groups = defaultdict(list)
    for i, r in enumerate(records):
        if owner[i] == i:
            for key in node_seeds(r, D, weak):
                groups[key].append(i)
    return groups


def largest_group(records, D: int, weak: bool = False) -> int:
    return max((len(g) for g in seed_groups(records, D, weak).values()), default=0)


def over_limit(records, D: int):
    """(the lowest first record among the nodes of a group beyond the limit, that group's entries), or None."""
    worst = [(min(g), len(g)) for g in seed_groups(records, D).values() if len(g) > MAX_GROUP]
    return min(worst) if worst else None


# ---- the sweeps, as the header states them --------------------------------------------------------------------------------------------

def sweeps(n: int, edges):
    """(labels, sweeps) of the min-label sweeps with pointer jumping over an edge list on places 0 .. n-1."""
    labels = list(range(n))
    count = 0
    while True:
        nxt = list(labels)
        changed = False
        for a, b in edges:
            la, lb = labels[a], labels[b]
            if la < lb:
                nxt[b] = min(nxt[b], la)
                changed = True
            elif lb < la:
                nxt[a] = min(nxt[a], lb)
                changed = True
        if not changed:
            return labels, count
        labels = [nxt[nxt[v]] for v in range(n)]
        count += 1


def components(n: int, edges):
    uf = UnionFind(range(n))
    for a, b in edges:
        uf.join(a, b)
    return [uf.find(v) for v in range(n)]
