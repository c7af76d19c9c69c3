"""Plain-Python statement of FQD_FAST_STRAND=both: the yardstick of tests/test_strand_core.py, tests/test_gpu_strand.py and
tests/test_fast_strand_cli.py.  Written from the rule's text, not from csrc/fqd_strand_core.hpp.

- comp: A<->T, C<->G, every other byte (N included) as it is; rc(s) = comp of s read backwards
- single-end: canon(s) = min(s, rc(s)) as bytes; flipped = rc(s) < s
- pairs: canon(a, b) = (a, b) if a <= b else (b, a) in the order of Python's bytes; flipped = b < a; nothing is complemented
- two records are strand-duplicates iff their canonical forms are identical; the first occurrence is kept
"""
import numpy as np

COMP = bytes.maketrans(b"ACGT", b"TGCA")
_COMP_NP = np.frombuffer(COMP, dtype=np.uint8)


def rc(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


def canon_se(s: bytes):
    """(canonical read, flipped)."""
    r = rc(s)
    return (r, True) if r < s else (s, False)


def canon_pe(a: bytes, b: bytes):
    """((first mate, second mate), flipped)."""
    return ((b, a), True) if b < a else ((a, b), False)


def canon_key(record):
    """record: a bytes (single-end) or a tuple of two (pair).  The hashable that strand-duplicates share."""
    return canon_se(record)[0] if isinstance(record, bytes) else canon_pe(*record)[0]


def expected_keep(records):
    """uint8 flags: 1 at the first occurrence of every canonical key."""
    seen, keep = set(), np.zeros(len(records), np.uint8)
    for i, r in enumerate(records):
        k = canon_key(r)
        if k not in seen:
            seen.add(k)
            keep[i] = 1
    return keep


def expected_layout(mates):
    """mates: one list of reads (single-end) or two (pairs).  What fqd_canonical_reads writes: (buffer bytes,
    [off0, off1], [len0, len1], flipped) with numpy arrays of the ABI's types."""
    n = len(mates[0])
    parts, flipped = [], np.zeros(n, np.uint8)
    lens = [np.zeros(n, np.uint32) for _ in mates]
    for i in range(n):
        if len(mates) == 1:
            c, f = canon_se(mates[0][i])
            c = (c,)
        else:
            c, f = canon_pe(mates[0][i], mates[1][i])
        flipped[i] = f
        for m, x in enumerate(c):
            lens[m][i] = len(x)
            parts.append(x)
    total = sum(l.astype(np.uint64) for l in lens)
    start = np.zeros(n, np.uint64)
    start[1:] = np.cumsum(total)[:-1]
    offs = [start] if len(mates) == 1 else [start, start + lens[0].astype(np.uint64)]
    return b"".join(parts), offs, lens, flipped


# ---- numpy forms for batches of reads of one length (rows of a 2-D uint8 array) ------------------------------------------

def rc_rows(a: np.ndarray) -> np.ndarray:
    return _COMP_NP[a[:, ::-1]]


def _first_diff_less(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """Per row: y < x in byte order (rows of equal length)."""
    d = x != y
    any_d = d.any(axis=1)
    at = d.argmax(axis=1)
    rows = np.arange(len(x))
    return any_d & (y[rows, at] < x[rows, at])


def canon_se_rows(a: np.ndarray):
    """(canonical rows, flipped) of an (n, L) array."""
    r = rc_rows(a)
    f = _first_diff_less(a, r)
    return np.where(f[:, None], r, a), f.astype(np.uint8)


def canon_pe_rows(a: np.ndarray, b: np.ndarray):
    """((first rows, second rows), flipped) of two (n, L) arrays of ONE length (no prefix case)."""
    assert a.shape == b.shape
    f = _first_diff_less(a, b)
    return (np.where(f[:, None], b, a), np.where(f[:, None], a, b)), f.astype(np.uint8)


def first_occurrence_rows(*cols: np.ndarray) -> np.ndarray:
    """uint8 flags: 1 at the first row with its content (the columns side by side)."""
    rows = np.ascontiguousarray(np.concatenate(cols, axis=1))
    _, first = np.unique(rows.view(np.dtype((np.void, rows.shape[1]))).ravel(), return_index=True)
    keep = np.zeros(len(rows), np.uint8)
    keep[first] = 1
    return keep
