"""Plain-Python restatement of the reference's sequence-based modes (`--compare-seq tight|loose|tail-hamming`), the
yardstick of the device sort and heads (csrc/fqd_seq.hip) and of the CLI.

- records: FASTQ = 4 lines, FASTA = 2 lines, a truncated last record is dropped (fastqview.cpp:92-138,
  fastaview.cpp:78-100); the sequence is its line without the '\\n'
- order: FastqView::cmp (fastqview.cpp:56-67): strncmp over the shorter sequence line counted with its '\\n', the
  shorter first; without bytes below '\\n' that is the byte order of seq + b'\\n'.  Pairs by (mate 1, mate 2)
  (RecordPair::operator<, paired_external_sort.hpp:20-33); pairing stops with the shorter file (sort_buckets,
  paired_external_sort.hpp:128-135).  Equal keys keep their input order (a stable sort: the documented divergence)
- scan: seq_dup_remover.hpp:54-109 (SE) and 131-218 (PE) with the comparators of comparator.cpp:45-91 and
  SeqUtils::hammingDistance (seq_utils.cpp:65-72)
- clusters: file_utils.cpp:98-112 (head's ID line, "--" + ID line of every duplicate)
"""

TIGHT, LOOSE, HAMMING = 0, 1, 2
MODES = {"tight": TIGHT, "loose": LOOSE, "tail-hamming": HAMMING}


def parse(data: bytes, fasta: bool):
    """[(record bytes, id line with '\\n', sequence without '\\n')] of the whole records of data."""
    per = 2 if fasta else 4
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    else:
        lines = lines[:-1] if lines else lines               # a last line without '\n' belongs to a truncated record
    out = []
    for k in range(0, len(lines) - per + 1, per):
        rec = lines[k:k + per]
        out.append((b"".join(x + b"\n" for x in rec), rec[0] + b"\n", rec[1]))
    return out


def sort_key(mates):
    return tuple(m + b"\n" for m in mates)


def sorted_order(seqs):
    """seqs: list of tuples of mates (1 or 2 sequences); the stable sorted order of indices."""
    return sorted(range(len(seqs)), key=lambda i: sort_key(seqs[i]))


def _ham(a, b):
    return sum(x != y for x, y in zip(a, b))


def matches(mode, d, ref, x):
    """comparator.cpp:45-91 on sequences without '\\n' (len-1 of the reference's lengths)."""
    if mode == TIGHT:
        return all(r == y for r, y in zip(ref, x))
    if mode == LOOSE:
        for r, y in zip(ref, x):
            n = min(len(r), len(y))
            if r[:n] != y[:n]:
                return False
        if len(ref) == 2:                                   # comparator.cpp:73: both overlaps same-sided
            (r1, r2), (x1, x2) = ref, x
            return (len(r1) <= len(x1) and len(r2) <= len(x2)) or (len(r1) > len(x1) and len(r2) > len(x2))
        return True
    return all(len(r) == len(y) and _ham(r, y) <= d for r, y in zip(ref, x))


def heads(mode, d, sorted_seqs):
    """The reference's scan over records in sorted order: head[k] = record k is written."""
    out = []
    ref = None
    for x in sorted_seqs:
        if ref is None or not matches(mode, d, ref, x):
            out.append(1)
            ref = x
        else:
            out.append(0)
            if mode == LOOSE and all(len(r) <= len(y) for r, y in zip(ref, x)):   # seq_dup_remover.hpp:93-98,194-202
                ref = x
    return out


def dedup(inputs, fasta=False, mode=TIGHT, distance=2):
    """inputs: file contents (1 or 2).  Returns (outputs, clusters, total, duplicates) as the reference writes them."""
    files = [parse(x, fasta) for x in inputs]
    n = min(len(f) for f in files)
    seqs = [tuple(f[i][2] for f in files) for i in range(n)]
    order = sorted_order(seqs)
    h = heads(mode, distance, [seqs[i] for i in order])
    outputs, clusters = [], []
    for f in files:
        outputs.append(b"".join(f[i][0] for i, keep in zip(order, h) if keep))
        clusters.append(b"".join((b"" if keep else b"--") + f[i][1] for i, keep in zip(order, h)))
    return outputs, clusters, n, n - sum(h)


def verbose_line(total, dups, paired):
    what = "read pairs" if paired else "reads"
    return f"{total} {what} processed, out of which {dups} duplicates were removed.\n"
