"""The rule of FQD_FAST_CONSENSUS=1 (fastq-dupaway_amd/csrc/fqd_consensus_core.hpp), stated sequentially: a column's vote, a
cluster's consensus lines, and a whole text with its record arrays gone through cluster by cluster.  Plain Python over bytes;
nothing here knows of lanes, tiers or atomics.  The tests hold the header's host compile (tests/test_consensus_core.py), the
device code (tests/test_gpu_consensus.py) and the run (tests/test_fast_consensus_cli.py) against it."""

LETTERS = b"ACGTN"                                             # the order of the tie rule
N = 4
BASE = 33
MAX_Q = 93


def letter(b):
    """0 .. 3 for A, C, G, T; every other byte stands for N."""
    at = LETTERS.find(bytes([b]))
    return at if 0 <= at < N else N


def weight(b, q):
    return 0 if letter(b) == N or q < BASE else q - BASE


def column(bases, quals, own):
    """The members' bases and quality bytes of one column and the written member's own base byte: (winner 0 .. 4, the quality
    byte written, whether the winner is not the written member's letter)."""
    S = [0] * 5
    present = [False] * 5
    for b, q in zip(bases, quals):
        S[letter(b)] += weight(b, q)
        present[letter(b)] = True
    top = max(S[x] for x in range(5) if present[x])
    tied = [x for x in range(5) if present[x] and S[x] == top]
    win = letter(own) if letter(own) in tied else tied[0]
    Q = min(max(S[win] - (sum(S) - S[win]), 0), MAX_Q)
    return win, BASE + Q, win != letter(own)


def vote(members):
    """members: (sequence, quality) of one mate, the written member FIRST, all of one length.  Returns (the sequence line
    written, the quality line written, the columns changed)."""
    seq0, qual0 = members[0]
    assert all(len(s) == len(seq0) == len(q) for s, q in members)
    seq, qual, changed = bytearray(seq0), bytearray(qual0), 0
    for p in range(len(seq0)):
        win, q, differs = column([s[p] for s, _ in members], [q[p] for _, q in members], seq0[p])
        if differs:
            seq[p] = LETTERS[win]
            changed += 1
        qual[p] = q
    return bytes(seq), bytes(qual), changed


def clusters_of(perm, head):
    """The runs of (perm, head) as lists of records, the written member first."""
    out = []
    for r, h in zip(perm, head):
        if h:
            out.append([])
        out[-1].append(int(r))
    return out


def apply(text, start, size, seq_off, seq_len, clusters, changed=None):
    """One file: text (a bytearray, changed in place) with the record arrays of the record scan; clusters as clusters_of gives
    them.  changed: a bytearray of a flag a record shared by the two files' calls, or None.  Returns the info as a dict."""
    info = dict(clusters=0, members=0, bases_changed=0, reads_changed=0, largest=max((len(c) for c in clusters), default=0))
    for c in clusters:
        if len(c) < 2:
            continue
        L = int(seq_len[c[0]])
        assert all(int(seq_len[r]) == L for r in c)
        rows = []
        for r in c:
            s, q = int(seq_off[r]), int(start[r]) + int(size[r]) - 1 - L
            rows.append((bytes(text[s:s + L]), bytes(text[q:q + L])))
        seq, qual, n = vote(rows)
        w = c[0]
        s, q = int(seq_off[w]), int(start[w]) + int(size[w]) - 1 - L
        text[s:s + L] = seq
        text[q:q + L] = qual
        info["clusters"] += 1
        info["members"] += len(c)
        info["bases_changed"] += n
        if n:
            if changed is None or not changed[w]:
                info["reads_changed"] += 1
            if changed is not None:
                changed[w] = 1
    return info


def lines_fit(start, size, seq_off, seq_len):
    if size < seq_len + 1 or seq_off < start:
        return False
    q = start + size - 1 - seq_len
    return seq_off + seq_len < q or (seq_len == 0 and seq_off <= q)


# ---- FASTQ files as the run sees them ------------------------------------------------------------------------------------------

def parse_fastq(data):
    """[(id line, sequence, plus line, quality)] of a well-formed four-line FASTQ text."""
    lines = data.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [tuple(lines[k:k + 4]) for k in range(0, len(lines) - 1, 4)]


def format_fastq(records):
    return b"".join(b"\n".join(r) + b"\n" for r in records)


def consensus_records(files, clusters):
    """files: one or two lists of parse_fastq records; clusters: lists of record numbers, the written member first.  Returns
    (the files with the written members' lines replaced, bases changed, records (pairs) changed)."""
    out = [list(f) for f in files]
    bases, touched = 0, set()
    for c in clusters:
        if len(c) < 2:
            continue
        for s, f in enumerate(files):
            seq, qual, n = vote([(f[r][1], f[r][3]) for r in c])
            out[s][c[0]] = (f[c[0]][0], seq, f[c[0]][2], qual)
            bases += n
            if n:
                touched.add(c[0])
    return out, bases, len(touched)
