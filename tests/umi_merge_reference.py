"""Plain-Python statement of FQD_FAST_UMI_MISMATCH=1|2: the yardstick of tests/test_umi_merge_core.py,
tests/test_gpu_umi_merge.py and tests/test_fast_umi_merge_cli.py.  Written from the rule's text the SEQUENTIAL way —
UMI-tools' directional method: rank sort, then a breadth-first search from every unclaimed node — not as the label sweeps of
csrc/fqd_umi_merge_core.hpp.

- sequence group: the records whose sequences (the caller's `seqkey`: mate 1, mate 2, canonical where asked) are identical.
- node: one distinct string of UMI bases in a group; count = its records, first = its first record in input order.
- edge a -> b: hamming(a, b) <= D and count(a) >= 2 * count(b) - 1.
- rank: count descending, then first ascending.  Nodes are visited in rank order; an unclaimed node starts a component of
  everything it reaches through unclaimed nodes; a reached node belongs to the first component that reached it.
- a merged cluster = the records of a component's nodes; its owner = its first record in input order.
- sweeps = the deepest level any search reached (the most label sweeps a parallel fixed point needs).
"""
from collections import OrderedDict

import numpy as np

NO_RECORD = 0xFFFFFFFFFFFFFFFF


def directional(umis, counts, firsts, D):
    """One group's nodes (equal-length byte strings, in any order) -> (root index per node, deepest level)."""
    s = len(umis)
    U = np.frombuffer(b"".join(umis), np.uint8).reshape(s, -1) if s else np.zeros((0, 1), np.uint8)
    c = np.asarray(counts, np.int64)
    order = sorted(range(s), key=lambda v: (-counts[v], firsts[v]))
    root = [-1] * s
    deepest = 0
    for start in order:
        if root[start] >= 0:
            continue
        root[start] = start
        level, depth = [start], 0
        while level:
            reached = []
            for a in level:
                near = (U != U[a]).sum(axis=1) <= D
                allowed = c[a] >= 2 * c - 1
                for b in np.nonzero(near & allowed)[0]:
                    if root[b] < 0:
                        root[b] = start
                        reached.append(int(b))
            if reached:
                depth += 1
            level = reached
        deepest = max(deepest, depth)
    return root, deepest


def merge(umis, seqkeys, D, max_group):
    """umis[i] = record i's UMI bases (joiners taken out), seqkeys[i] = what its sequence group is told by (hashable).
    Returns (owner_out as uint32 array or None where a group is over the limit, info dict, owner_exact, owner_seq, size):
    the last three are what the device entry takes."""
    n = len(umis)
    exact, by_seq = OrderedDict(), OrderedDict()
    owner_exact, owner_seq, size = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i, (u, k) in enumerate(zip(umis, seqkeys)):
        node = exact.setdefault((k, u), [i, 0])
        node[1] += 1
        owner_exact[i] = node[0]
        group = by_seq.setdefault(k, [i, []])
        owner_seq[i] = group[0]
        if node[0] == i:
            group[1].append((u, node))
    for first, count in exact.values():
        size[first] = count
    info = dict(nodes=len(exact), groups=0, merged=0, largest=1 if n else 0, sweeps=0, max_group=max_group, over_limit_nodes=0, over_limit_first=NO_RECORD)
    given = {}
    over = None
    for _, nodes in by_seq.values():
        s = len(nodes)
        info["largest"] = max(info["largest"], s)
        if s > 1:
            info["groups"] += 1
        if s > max_group:
            first = nodes[0][1][0]
            if over is None or first < over[0]:
                over = (first, s)
    if over is not None:
        info.update(over_limit_first=over[0], over_limit_nodes=over[1])
        return None, info, owner_exact, owner_seq, size
    for _, nodes in by_seq.values():
        firsts = [node[0] for _, node in nodes]
        if len(nodes) == 1:
            given[firsts[0]] = firsts[0]
            continue
        root, deepest = directional([u for u, _ in nodes], [node[1] for _, node in nodes], firsts, D)
        info["sweeps"] = max(info["sweeps"], deepest)
        lowest = {}
        for v, r in enumerate(root):
            lowest[r] = min(lowest.get(r, firsts[v]), firsts[v])
            info["merged"] += r != v
        for v, r in enumerate(root):
            given[firsts[v]] = lowest[r]
    owner_out = np.array([given[int(o)] for o in owner_exact], np.uint32)
    return owner_out, info, owner_exact, owner_seq, size


def clusters_of(owner_out):
    """The merged clusters as lists of records, in the order of their first records, members in input order."""
    groups = OrderedDict()
    for i, o in enumerate(owner_out):
        groups.setdefault(int(o), []).append(i)
    assert all(g[0] == o for o, g in groups.items())
    return [groups[o] for o in sorted(groups)]
