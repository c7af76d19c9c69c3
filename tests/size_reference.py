"""Plain-Python statement of FQD_FAST_SIZEOUT / FQD_FAST_LEVELS on top of tests/fast_keep_reference.py: the yardstick of
tests/test_size_core.py, tests/test_gpu_sizes.py and tests/test_fast_sizes_cli.py.  Written from the rule's text, not from
csrc/fqd_size_core.hpp.

- size of a cluster = the number of its members; the written record carries it, every other record carries nothing
- label(N) = b";size=" + N in decimal, no padding
- the label goes in at the end of the first word of the ID line: the word begins with '@' / '>' and ends in front of the first
  of ' ', '\\t', '\\r', '\\n' behind the leading byte (at the line's end where there is none).  A `;size=` that is already
  there is not looked at
- `<output 1>.duplevels`: "#level clusters records", the sixteen rows 1 .. 9, 10-49, 50-99, 100-499, 500-999, 1000-4999,
  5000-9999, 10000+ (all always present), "#total clusters records", "#largest N"; tab-separated
"""
import fast_keep_reference as fast

ROWS = ["1", "2", "3", "4", "5", "6", "7", "8", "9", "10-49", "50-99", "100-499", "500-999", "1000-4999", "5000-9999", "10000+"]
LOWER = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000]      # the smallest size of every row
WORD_ENDS = b" \t\r\n"


def level(size: int) -> int:
    """The row (0 .. 15) a cluster of `size` >= 1 members counts in."""
    return max(k for k, lo in enumerate(LOWER) if size >= lo)


def label(size: int) -> bytes:
    return b";size=" + str(size).encode()


def first_word_end(line: bytes) -> int:
    """The length of '@' + the first word: the position of the first word end behind the leading byte, len(line) for none."""
    ends = [k for k in range(1, len(line)) if line[k] in WORD_ENDS]
    return ends[0] if ends else len(line)


def labelled(record: bytes, size: int) -> bytes:
    """The record with its label: nothing else changes.  The ID line is the record's first line."""
    nl = record.find(b"\n")
    at = first_word_end(record[:nl + 1] if nl >= 0 else record)
    return record[:at] + label(size) + record[at:]


def sizes_from(perm, head):
    """What fqd_cluster_sizes writes: size[perm[k]] = the length of the run that starts at k where head[k], 0 elsewhere."""
    n = len(perm)
    size = [0] * n
    k = 0
    while k < n:
        end = k + 1
        while end < n and not head[end]:
            end += 1
        size[perm[k]] = end - k
        k = end
    return size


def levels_of(sizes):
    """(clusters per row, records per row, largest) of the cluster sizes (zeros are no clusters)."""
    clusters, records, largest = [0] * 16, [0] * 16, 0
    for s in sizes:
        if s:
            clusters[level(s)] += 1
            records[level(s)] += s
            largest = max(largest, s)
    return clusters, records, largest


def duplevels_text(sizes) -> bytes:
    clusters, records, largest = levels_of(sizes)
    lines = ["#level\tclusters\trecords"]
    lines += [f"{ROWS[k]}\t{clusters[k]}\t{records[k]}" for k in range(16)]
    lines += [f"#total\t{sum(clusters)}\t{sum(records)}", f"#largest\t{largest}"]
    return ("\n".join(lines) + "\n").encode()


def dedup_sized(inputs, fasta=False, best=False, keys=None):
    """inputs: file contents (1 or 2); keys: one hashable per record (pair) where another statement decides what a cluster is
    (strand_reference / umi_reference), default: the sequences.  Returns (outputs with the labels, the `.duplevels` text,
    total, duplicates, the plain outputs, the cluster files — those of a run without the labels)."""
    files = [fast.parse(x, fasta) for x in inputs]
    n = len(files[0])
    assert all(len(f) == n for f in files)
    if keys is None:
        keys = [tuple(f[i][2] for f in files) for i in range(n)]
    groups = fast.clusters_of(keys)
    scores = [min(fast.SAT, sum(fast.score(f[i][0]) for f in files)) for i in range(n)]
    size_at, listing = {}, []
    for g in groups:
        w = fast.pick(g, scores) if best else g[0]
        size_at[w] = len(g)
        order = list(g)
        at = order.index(w)
        order[0], order[at] = order[at], order[0]
        listing.append(order)
    outputs = [b"".join(labelled(f[i][0], size_at[i]) for i in range(n) if i in size_at) for f in files]
    plain = [b"".join(f[i][0] for i in range(n) if i in size_at) for f in files]
    cluster_files = [b"".join((b"" if k == 0 else b"--") + f[i][1] for order in listing for k, i in enumerate(order)) for f in files]
    return outputs, duplevels_text(list(size_at.values())), n, n - len(groups), plain, cluster_files
