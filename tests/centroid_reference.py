"""FQD_FAST_CENTROID=abundant as a sequential statement (csrc/fqd_centroid_core.hpp says the same with proofs): dicts over
(run, label) and a loop.  The yardstick of tests/test_centroid_core.py's cases, tests/test_gpu_centroid.py and
tests/test_fast_centroid_cli.py.

A run of (perm, head) is a cluster, its members in input order.  label[r] is record r's exact owner, weight[r] what it stands
for.  The abundance of a member is the summed weight of the members OF ITS RUN with its label; the centroid of a run is the
member of the largest abundance, the earliest among equals."""
import numpy as np

SATURATED = 0xFFFFFFFF
SMALL, WAVE, BLOCK = 8, 64, 2048                               # csrc/fqd_centroid_core.hpp: kSmall, kWave, kBlockLimit


def runs_of(head):
    """The run every place lies in, counted from 0."""
    return np.cumsum(np.asarray(head) != 0) - 1


def abundances(perm, head, label, weight=None):
    """(abundance by record as uint32, saturated; the unsaturated sums by record as Python ints; fqd_centroid_info as a dict)."""
    n = len(perm)
    # (plain lists of Python ints, and a place's key kept for the second loop: two million places take half the time)
    perm, label, run = np.asarray(perm).tolist(), np.asarray(label).tolist(), runs_of(head).tolist()
    weight = None if weight is None else np.asarray(weight).tolist()
    total, keys = {}, [None] * n
    for k in range(n):
        r = perm[k]
        key = keys[k] = (run[k], label[r])
        total[key] = total.get(key, 0) + (1 if weight is None else weight[r])
    exact = [0] * n
    for k in range(n):
        exact[perm[k]] = total[keys[k]]
    members, subs = {}, {}
    for c in run:
        members[c] = members.get(c, 0) + 1
    for c, _ in total:
        subs[c] = subs.get(c, 0) + 1
    tiers = [0] * 5
    for s in members.values():
        tiers[0 if s == 1 else 1 if s <= SMALL else 2 if s <= WAVE else 3 if s <= BLOCK else 4] += 1
    info = dict(clusters=len(members), mixed=sum(1 for v in subs.values() if v > 1), subclusters=len(total), tier_clusters=tiers,
                largest=max(members.values(), default=0))
    return np.array([min(a, SATURATED) for a in exact], np.uint32), exact, info


def pick(perm, head, value):
    """What fqd_seq_pick_best does over value (by record): per run the member of the highest value, the earliest place among
    equals, changes places with the first.  Returns (the new order, the runs that changed)."""
    perm = np.array(perm, np.uint32)
    n, moved, k = len(perm), 0, 0
    while k < n:
        end = k + 1
        while end < n and not head[end]:
            end += 1
        best = k
        for j in range(k + 1, end):
            if int(value[perm[j]]) > int(value[perm[best]]):
                best = j
        if best != k:
            perm[k], perm[best] = perm[best], perm[k]
            moved += 1
        k = end
    return perm, moved


def masked_scores(perm, head, label, score):
    """fqd_subcluster_scores: min(score, 2^32 - 2) + 1 for the members that share the label of the record at their run's head
    place, 0 for the others; by record."""
    out = np.zeros(len(perm), np.uint32)
    at_head = None
    for k in range(len(perm)):
        r = int(perm[k])
        if k == 0 or head[k]:
            at_head = int(label[r])
        out[r] = min(int(score[r]), SATURATED - 1) + 1 if int(label[r]) == at_head else 0
    return out


def written(perm, head, label, weight=None, score=None, stored=None):
    """The record every run is written by: its centroid, or with scores (FQD_FAST_KEEP=best) the best-scored member of the
    centroid's sub-cluster, the earliest among equals.  Straight from the definition, without the exchanges."""
    if stored is None:
        stored = abundances(perm, head, label, weight)[0]
    out, k, n = [], 0, len(perm)
    while k < n:
        end = k + 1
        while end < n and not head[end]:
            end += 1
        members = [int(perm[j]) for j in range(k, end)]
        centroid = members[max(range(len(members)), key=lambda i: (int(stored[members[i]]), -i))]
        if score is not None:
            sub = [r for r in members if label[r] == label[centroid]]
            # (scores 2^32 - 1 and 2^32 - 2 fall together: fqd_seq_scores saturates at the former, the masked score at the latter)
            centroid = sub[max(range(len(sub)), key=lambda i: (min(int(score[sub[i]]), SATURATED - 1), -i))]
        out.append(centroid)
        k = end
    return out
