"""The sequential statement of FQD_FAST_PREFIX=L (fastq-dupaway_amd/csrc/fqd_prefix_core.hpp), in plain Python: exact clusters by
(seq1, seq2), every eligible node b cut to every shape that occurs and the cut looked up among the nodes (all_pairs asks every pair instead, for
small inputs), the parent rule (least span, then lowest record), the trees,
owner = the lowest record of a tree.  Also the seed hash of the header, restated, so that a test can say which nodes share a seed
group, how many pairs a group makes the device compare and how large the largest group of an input is."""
from collections import defaultdict

import numpy as np

from near_reference import absorb, exact_owners, mix            # the hash's two steps are fqd_near_core.hpp's

MAX_GROUP = 4096
NO_RECORD = 0xFFFFFFFFFFFFFFFF
NO_PARENT = (1 << 64) - 1
TAG = 0x7072656669780000


# ---- the rule --------------------------------------------------------------------------------------------------------------------

def span(node) -> int:
    return sum(len(m) for m in node)


def eligible(node, L: int) -> bool:
    return all(len(m) >= L for m in node)


def is_prefix(a, b) -> bool:
    """a ⊑ b for two nodes (tuples of 1 or 2 mates): different nodes, and every mate of a begins the same mate of b."""
    return a != b and all(len(x) <= len(y) and y[:len(x)] == x for x, y in zip(a, b))


def pack(span_: int, node: int) -> int:
    return span_ << 32 | node


def supersequences(records, fit):
    """For every eligible node b the eligible nodes a with a ⊑ b, as pairs (a, b): every cut of b to a shape that occurs is looked
    up among the nodes (no seed, no hash of the device's: a dictionary of whole nodes)."""
    by_node = {records[v]: v for v in fit}
    shapes = sorted({tuple(len(m) for m in records[v]) for v in fit})
    pairs = []
    for b in fit:
        node = records[b]
        lens = tuple(len(m) for m in node)
        for shape in shapes:
            if shape != lens and all(x <= y for x, y in zip(shape, lens)):
                a = by_node.get(tuple(m[:k] for m, k in zip(node, shape)))
                if a is not None:
                    pairs.append((a, b))
    return pairs


def all_pairs(records, fit):
    """The same pairs by asking every pair (small inputs)."""
    return [(a, b) for a in fit for b in fit if is_prefix(records[a], records[b])]


def parents(records, L: int, pairs_of=supersequences):
    """(owner, nodes, parent): parent[v] for every node v (v itself for a root or a node that is not eligible)."""
    owner = exact_owners(records)
    nodes = [i for i in range(len(records)) if owner[i] == i]
    fit = [v for v in nodes if eligible(records[v], L)]
    best = {}
    for a, b in pairs_of(records, fit):
        best[a] = min(best.get(a, NO_PARENT), pack(span(records[b]), b))
    parent = {v: best[v] & 0xFFFFFFFF if v in best else v for v in nodes}
    return owner, nodes, parent


def depth_of(parent, v) -> int:
    d = 0
    while parent[v] != v:
        v, d = parent[v], d + 1
    return d


def root_of(parent, v) -> int:
    while parent[v] != v:
        v = parent[v]
    return v


def jumps_for(deepest: int) -> int:
    """The pointer jumps that change something: a jump doubles what a pointer spans."""
    return (deepest - 1).bit_length() if deepest > 1 else 0


def merged_owners(records, L: int):
    """owner_out[i] = the first record of record i's merged cluster, and what the info counts but the seed groups' figures: a dict."""
    owner, nodes, parent = parents(records, L)
    root = {v: root_of(parent, v) for v in nodes}
    first = {}
    for v in nodes:                                             # ascending: the first one seen is the lowest
        first.setdefault(root[v], v)
    out = np.array([first[root[int(owner[i])]] for i in range(len(records))], np.uint32)
    deepest = max((depth_of(parent, v) for v in nodes), default=0)
    counts = {"nodes": len(nodes), "eligible": sum(eligible(records[v], L) for v in nodes), "merged": len(set(root.values())),
              "children": sum(parent[v] != v for v in nodes), "deepest": deepest, "jumps": jumps_for(deepest)}
    assert counts["merged"] + counts["children"] == counts["nodes"] and counts["merged"] == len({int(x) for x in out})
    return out, counts


def spans(records):
    return np.array([span(r) for r in records], np.uint32)


def check_the_theorems(records, L: int):
    """What fqd_prefix_core.hpp proves, asked of one input: parents grow in span, every member of a tree is ⊑ its root, and no two
    roots are in one cluster."""
    owner, nodes, parent = parents(records, L)
    for v in nodes:
        if parent[v] != v:
            assert span(records[parent[v]]) > span(records[v])
            assert is_prefix(records[v], records[root_of(parent, v)])
    out, _ = merged_owners(records, L)
    roots = [v for v in nodes if parent[v] == v]
    assert len({int(out[v]) for v in roots}) == len(roots)
    return len(roots)


# ---- the seeds, restated -----------------------------------------------------------------------------------------------------------

def seed_bytes(h: int, segment: bytes) -> int:
    for k in range(0, len(segment), 8):
        h = absorb(h, int.from_bytes(segment[k:k + 8], "little"))
    return mix(h)


def node_seed(node, L: int, weak: bool = False) -> int:
    paired = len(node) > 1
    key = seed_bytes(mix(mix(L | int(paired) << 32) ^ TAG), node[0][:L])
    if paired:
        key = seed_bytes(key, node[1][:L])
    return key & 15 if weak else key


def seed_groups(records, L: int, weak: bool = False):
    """key -> the eligible nodes (first records) with that key."""
    owner = exact_owners(records)
    groups = defaultdict(list)
    for i, r in enumerate(records):
        if owner[i] == i and eligible(r, L):
            groups[node_seed(r, L, weak)].append(i)
    return groups


def compared_pairs(records, group) -> int:
    """The pairs of a group whose lengths give a direction."""
    lens = np.array([[len(m) for m in records[v]] for v in group], np.int64)
    le = np.all(lens[:, None, :] <= lens[None, :, :], axis=2)
    same = np.all(lens[:, None, :] == lens[None, :, :], axis=2)
    return int((le & ~same).sum())                              # (an ordered pair (short, long) for every unordered one with a direction)


def group_counts(records, L: int, weak: bool = False):
    """(groups, largest group, pairs compared, pairs related) as the device counts them.  Related nodes share a key, weak or not,
    so the related pairs of the groups are the related pairs of the input."""
    groups = seed_groups(records, L, weak)
    pairs = sum(compared_pairs(records, g) for g in groups.values() if len(g) > 1)
    owner = exact_owners(records)
    fit = [i for i in range(len(records)) if owner[i] == i and eligible(records[i], L)]
    found = supersequences(records, fit)
    key = {v: k for k, g in groups.items() for v in g}
    assert all(key[a] == key[b] for a, b in found)
    return len(groups), max((len(g) for g in groups.values()), default=0), pairs, len(found)


def largest_group(records, L: int, weak: bool = False) -> int:
    return max((len(g) for g in seed_groups(records, L, weak).values()), default=0)


def over_limit(records, L: int):
    """(the lowest first record among the nodes of a group beyond the limit, that group's entries), or None."""
    worst = [(min(g), len(g)) for g in seed_groups(records, L).values() if len(g) > MAX_GROUP]
    return min(worst) if worst else None


# ---- the jumps, as the header states them ------------------------------------------------------------------------------------------

def jump(up):
    """(roots, the jumps that changed something) of pointer jumping over up[v] (a root points at itself)."""
    up, count = list(up), 0
    while True:
        nxt = [up[up[v]] for v in range(len(up))]
        if nxt == up:
            return up, count
        up, count = nxt, count + 1
