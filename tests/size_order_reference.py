"""Plain-Python statement of FQD_FAST_SORT=size / FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE on top of tests/size_reference.py and
tests/fast_keep_reference.py: the yardstick of tests/test_size_order_core.py, tests/test_gpu_size_order.py and
tests/test_fast_sort_cli.py.  Written from the rule's text, not from csrc/fqd_size_order_core.hpp.

- a cluster of fewer than MINSIZE or more than MAXSIZE members is not written at all (MAXSIZE none: no upper bound)
- under SORT=size the written records come in order of decreasing cluster size; among clusters of one size the cluster whose
  FIRST member in input order stands earlier comes first, whichever member is written
- `;size=N` sits on the written record wherever it is written
- with a filter, `-v` says one more line: how many clusters holding how many reads (read pairs) were not written
"""
import fast_keep_reference as fast
import size_reference as sizes


def filtered(size, keep, lo, hi):
    """What fqd_size_filter makes of the flags: (keep, clusters taken out, their records).  hi = 0 or None: no upper bound."""
    out, clusters, records = list(keep), 0, 0
    for r, k in enumerate(keep):
        if k and (size[r] < lo or (hi and size[r] > hi)):
            out[r] = 0
            clusters += 1
            records += size[r]
    return out, clusters, records


def written_order(perm, head, size, keep):
    """What fqd_size_order writes: the head places whose record is kept, in place order, sorted stably by size descending.
    (An entry of perm outside 0 .. n-1, which no grouping produces, names no record: its place is not a kept one.)"""
    places = [s for s in range(len(perm)) if head[s] and perm[s] < len(perm) and keep[perm[s]]]
    return [perm[s] for s in sorted(places, key=lambda s: -size[perm[s]])]       # sorted() is stable


def not_written_line(clusters, records, paired, lo, hi):
    return f"{clusters} clusters holding {records} {'read pairs' if paired else 'reads'} were not written " \
           f"(FQD_FAST_MINSIZE={lo}, FQD_FAST_MAXSIZE={hi if hi else 'none'}).\n"


def dedup_ordered(inputs, fasta=False, best=False, keys=None, by_size=False, lo=1, hi=None, sizeout=False):
    """inputs: file contents (1 or 2); keys as in size_reference.dedup_sized.  Returns (outputs, clusters not written, their
    records, the sizes of the written clusters in written order)."""
    files = [fast.parse(x, fasta) for x in inputs]
    n = len(files[0])
    assert all(len(f) == n for f in files)
    if keys is None:
        keys = [tuple(f[i][2] for f in files) for i in range(n)]
    groups = fast.clusters_of(keys)                           # by first member
    scores = [min(fast.SAT, sum(fast.score(f[i][0]) for f in files)) for i in range(n)]
    def outside(g):
        return len(g) < lo or bool(hi and len(g) > hi)

    stay = [g for g in groups if not outside(g)]
    gone = [g for g in groups if outside(g)]
    written = [(fast.pick(g, scores) if best else g[0], len(g), g[0]) for g in stay]
    if by_size:
        written.sort(key=lambda t: (-t[1], t[2]))            # decreasing size, then the first member's place
    else:
        written.sort(key=lambda t: t[0])                      # the input's order, of the records that are written
    outputs = [b"".join(sizes.labelled(f[w][0], size) if sizeout else f[w][0] for w, size, _ in written) for f in files]
    return outputs, len(gone), sum(len(g) for g in gone), [size for _, size, _ in written]
