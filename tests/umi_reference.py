"""Plain-Python statement of FQD_FAST_UMI=colon|underscore: the yardstick of tests/test_umi_core.py, tests/test_gpu_umi.py
and tests/test_fast_umi_cli.py.  Written from the rule's text, not from csrc/fqd_umi_core.hpp.

- ID line: '@' or '>' first, '\\n' last.  First word W: the bytes behind the leading byte up to, not including, the first of
  ' ', '\\t', '\\r', '\\n' (the line's end where there is none).
- UMI field U: the bytes of W behind the LAST separator byte in W (b':' or b'_').
- joiners '+', '-', '_' inside U; every other byte of U is one of ACGTN.  shape(U) = (len(U), places of the joiners);
  B(U) = U without its joiners.
- a record is refused for the first of: no separator in W, U empty, U longer than 64 bytes, a byte outside ACGTN+-_ in U,
  no base in U, shape(U) != shape(U of record 0); a run at its lowest refused record.
- key of a record = B(U) + mate 1's sequence (, mate 2's sequence); the first occurrence of a key is kept.
"""
import numpy as np

OK, NO_SEPARATOR, EMPTY, TOO_LONG, BAD_BYTE, NO_BASE, SHAPE_DIFFERS = range(7)
NO_RECORD = 0xFFFFFFFFFFFFFFFF
WORD_ENDS = b" \t\r\n"
JOINERS = b"+-_"
BASES = b"ACGTN"


def umi_of(id_line: bytes, sep: bytes):
    """(offset of U inside the line, U) or, where the record is refused on its own, (offset, reason): the offset is 0
    where W holds no separator."""
    body = id_line[1:]
    ends = [body.index(bytes([c])) for c in WORD_ENDS if bytes([c]) in body]
    word = body[:min(ends)] if ends else body
    at = word.rfind(sep)
    if at < 0:
        return 0, NO_SEPARATOR
    off = 1 + at + 1
    u = word[at + 1:]
    if not u:
        return off, EMPTY
    if len(u) > 64:
        return off, TOO_LONG
    if any(c not in JOINERS + BASES for c in u):
        return off, BAD_BYTE
    if all(c in JOINERS for c in u):
        return off, NO_BASE
    return off, u


def shape(u: bytes):
    """(length, joiner set as the ABI's 64-bit word)."""
    return len(u), sum(1 << p for p, c in enumerate(u) if c in JOINERS)


def bases(u: bytes) -> bytes:
    return bytes(c for c in u if c not in JOINERS)


def find(id_lines, sep: bytes):
    """What fqd_umi_find leaves: (umi_off as uint32 array, info dict with n_bases, umi_len, joiners, bad_record, bad_reason)."""
    offs = np.zeros(len(id_lines), np.uint32)
    info = dict(n_bases=0, umi_len=0, joiners=0, bad_record=NO_RECORD, bad_reason=OK)
    shape0 = None
    for i, line in enumerate(id_lines):
        off, u = umi_of(line, sep)
        offs[i] = off
        reason = u if isinstance(u, int) else OK
        if i == 0 and reason == OK:
            shape0 = shape(u)
            info.update(umi_len=shape0[0], joiners=shape0[1], n_bases=len(bases(u)))
        if reason == OK and shape0 is not None and shape(u) != shape0:
            reason = SHAPE_DIFFERS
        if reason != OK and info["bad_record"] == NO_RECORD:
            info.update(bad_record=i, bad_reason=reason)
    return offs, info


def keyed(id_lines, seqs, sep: bytes):
    """Mate 1's keyed bytes record by record: B(U) + seq.  Every record must be one the rule takes."""
    out = []
    for line, s in zip(id_lines, seqs):
        _, u = umi_of(line, sep)
        assert not isinstance(u, int)
        out.append(bases(u) + s)
    return out


def expected_layout(id_lines, seqs, sep: bytes):
    """What fqd_umi_reads writes: (buffer bytes, offsets uint64, lengths uint32)."""
    parts = keyed(id_lines, seqs, sep)
    lens = np.array([len(p) for p in parts], np.uint32)
    offs = np.zeros(len(parts), np.uint64)
    if len(parts) > 1:
        offs[1:] = np.cumsum(lens.astype(np.uint64))[:-1]
    return b"".join(parts), offs, lens


def key_of(id_line: bytes, sep: bytes, *seqs):
    _, u = umi_of(id_line, sep)
    assert not isinstance(u, int), (id_line, u)
    return (bases(u),) + tuple(seqs)


def expected_keep(keys):
    """uint8 flags: 1 at the first occurrence of every key (any hashables)."""
    seen, keep = set(), np.zeros(len(keys), np.uint8)
    for i, k in enumerate(keys):
        if k not in seen:
            seen.add(k)
            keep[i] = 1
    return keep


def first_occurrence_rows(*cols: np.ndarray) -> np.ndarray:
    """uint8 flags: 1 at the first row with its content (2-D uint8 columns side by side)."""
    rows = np.ascontiguousarray(np.concatenate(cols, axis=1))
    _, first = np.unique(rows.view(np.dtype((np.void, rows.shape[1]))).ravel(), return_index=True)
    keep = np.zeros(len(rows), np.uint8)
    keep[first] = 1
    return keep
