"""The sequential statement of FQD_FAST_UMI_HAMMING=D (fastq-dupaway_amd/csrc/fqd_near_umi_core.hpp), in plain Python.  A record
is (U, mates): its UMI field as it stands in the ID line, and a tuple of 1 or 2 byte strings.  Exact clusters by (tag, mates),
all pairs of equal tag and shape compared, union-find, then (v, link[v]) joined; owner = the lowest record.  Also the tag and the
tagged seed key of the header, restated, so that a test can say which nodes share a seed group, how many pairs are compared and
where the limit falls.  The CLI tests feed it umi_reference.bases (through the tag, which says the same) and
umi_merge_reference.merge's owners as links."""
from collections import Counter, defaultdict

import numpy as np

import near_reference as near

MAX_GROUP = near.MAX_GROUP
NO_RECORD = near.NO_RECORD
JOINERS = b"+-_"


# ---- the rule ------------------------------------------------------------------------------------------------------------------

def joiners_of(u: bytes) -> int:
    return sum(1 << p for p, c in enumerate(u) if c in JOINERS)


def tag(u: bytes, joiners: int) -> bytes:
    """T(U): U with every joiner place of the run's shape set to 0."""
    return bytes(0 if (joiners >> p) & 1 else c for p, c in enumerate(u))


def exact_owners(records, joiners: int):
    """owner[i] = the first record with record i's tag and mates (the run keyed B(U) ‖ mate 1, mate 2)."""
    first = {}
    return np.array([first.setdefault((tag(u, joiners), mates), i) for i, (u, mates) in enumerate(records)], np.uint32)


def molecules(records, D: int, joiners: int, link=None):
    """(owner_out, nodes, molecules, links): owner_out[i] = the first record of record i's molecule."""
    owner = exact_owners(records, joiners)
    nodes = [i for i in range(len(records)) if owner[i] == i]
    uf = near.UnionFind(nodes)
    by_tag_and_shape = defaultdict(list)
    for v in nodes:
        u, mates = records[v]
        by_tag_and_shape[(tag(u, joiners), tuple(len(m) for m in mates))].append(v)
    for same in by_tag_and_shape.values():
        mates0 = records[same[0]][1]
        arrays = [np.frombuffer(b"".join(records[v][1][m] for v in same), np.uint8).reshape(len(same), len(mates0[m])) for m in range(len(mates0))]
        for k in range(len(same)):
            ok = np.ones(len(same) - k - 1, bool)
            for a in arrays:
                ok &= (a[k + 1:] != a[k]).sum(axis=1) <= D
            for j in np.nonzero(ok)[0]:
                uf.join(same[k], same[k + 1 + j])
    links = 0
    if link is not None:
        for v in nodes:
            if int(link[v]) != v:
                assert int(link[v]) < v and owner[int(link[v])] == link[v], (v, link[v])
                uf.join(v, int(link[v]))
                links += 1
    out = np.array([uf.find(int(owner[i])) for i in range(len(records))], np.uint32)
    return out, len(nodes), len({int(x) for x in out}), links


# ---- the tagged seed key, restated --------------------------------------------------------------------------------------------------

def tag_words(u: bytes, joiners: int):
    t = tag(u, joiners)
    return [int.from_bytes(t[k:k + 8], "little") for k in range(0, len(t), 8)]


def seed_key(u: bytes, joiners: int, len1: int, len2: int, j: int, segment: bytes) -> int:
    h = near.mix(near.mix(len1 | len2 << 32) ^ ((j + 1) * near.MUL & near.M64))
    for w in tag_words(u, joiners):
        h = near.absorb(h, w)
    for k in range(0, len(segment), 8):
        h = near.absorb(h, int.from_bytes(segment[k:k + 8], "little"))
    return near.mix(h)


def node_seeds(record, D: int, joiners: int, weak: bool = False):
    u, mates = record
    m1 = mates[0]
    len2 = len(mates[1]) if len(mates) > 1 else 0
    keys = [seed_key(u, joiners, len(m1), len2, j, m1[near.bound(len(m1), D, j):near.bound(len(m1), D, j + 1)]) for j in range(D + 1)]
    return [k & 15 for k in keys] if weak else keys


def seed_groups(records, D: int, joiners: int, weak: bool = False):
    """key -> the nodes (first records) of its entries, a node once for every entry it has there."""
    owner = exact_owners(records, joiners)
    groups = defaultdict(list)
    for i, r in enumerate(records):
        if owner[i] == i:
            for key in node_seeds(r, D, joiners, weak):
                groups[key].append(i)
    return groups


def expected_pairs(records, D: int, joiners: int, weak: bool = False) -> int:
    """The pairs of entries of two different nodes, over all seed groups."""
    total = 0
    for g in seed_groups(records, D, joiners, weak).values():
        total += len(g) * (len(g) - 1) // 2 - sum(c * (c - 1) // 2 for c in Counter(g).values())
    return total


def over_limit(records, D: int, joiners: int):
    """(the lowest first record among the nodes of a group beyond the limit, that group's entries), or None."""
    worst = [(min(g), len(g)) for g in seed_groups(records, D, joiners).values() if len(g) > MAX_GROUP]
    return min(worst) if worst else None
