"""Plain-Python statement of FQD_FAST_SIZEIN on top of tests/size_reference.py and tests/fast_keep_reference.py: the yardstick
of tests/test_sizein_core.py, tests/test_gpu_sizein.py and tests/test_fast_sizein_cli.py.  Written from the rule's text, not
from csrc/fqd_sizein_core.hpp.

- W = the first word of the ID line: the bytes behind position 0 up to the first of ' ', '\\t', '\\r', '\\n' (the line's end
  where there is none).  Nothing behind W is looked at
- a candidate = a position p >= 1 in W at which the six bytes `;size=` stand (all six inside W), compared exactly
- no candidate: weight 1, no annotation.  Otherwise the FIRST candidate decides, by the first of these that holds:
  no digit behind it -> NO_DIGITS; eleven digits or more -> TOO_LARGE; a byte other than ';' behind the digits (inside W)
  -> BAD_END; the value 0 -> ZERO; a value above 2^31-1 -> TOO_LARGE; a second candidate in W -> TWICE; else the record's
  weight is the value and its annotation the bytes `;size=<digits>` (a ';' behind them is not part of it)
- file 2 of a pair: parsed by the same rule; an annotation there must say file 1's weight (1 where file 1 has none), else
  MATES_DIFFER; none is fine.  The run is refused at the LOWEST refused record of file 1, else of file 2
- a cluster's size = the sum of its members' weights; above 2^31-1 the run is refused
- the written record: the label at the annotation's place with the annotation's bytes left out; at the first word's end
  where the record has none
"""
import re

import fast_keep_reference as fast
import size_reference as sizes

OK, NO_DIGITS, BAD_END, ZERO, TOO_LARGE, TWICE, MATES_DIFFER = range(7)
NO_RECORD = 2 ** 64 - 1
MAX = 2 ** 31 - 1


def parse(line: bytes):
    """(weight, label_at, cut, reason) of one ID line."""
    wend = sizes.first_word_end(line)
    word = line[:wend]
    cands = [m.start() for m in re.finditer(b"(?=;size=)", word) if m.start() >= 1]
    if not cands:
        return 1, wend, 0, OK
    p = cands[0]
    digits = re.match(rb"[0-9]*", word[p + 6:]).group()
    behind = word[p + 6 + len(digits):p + 7 + len(digits)]
    if not digits:
        reason = NO_DIGITS
    elif len(digits) > 10:
        reason = TOO_LARGE
    elif behind not in (b"", b";"):
        reason = BAD_END
    elif int(digits) == 0:
        reason = ZERO
    elif int(digits) > MAX:
        reason = TOO_LARGE
    elif len(cands) > 1:
        reason = TWICE
    else:
        return int(digits), p, 6 + len(digits), OK
    return None, None, None, reason


def annotations(lines, expect=None):
    """What fqd_size_annotations says of one file's ID lines: (weights, label_at, cut, bad_record, bad_reason); the arrays are
    None where a record is refused."""
    out, bad = [], None
    for r, line in enumerate(lines):
        w, at, cut, reason = parse(line)
        if reason == OK and cut and expect is not None and expect[r] != w:
            reason = MATES_DIFFER
        if reason != OK and bad is None:
            bad = (r, reason)
        out.append((w, at, cut))
    if bad:
        return None, None, None, bad[0], bad[1]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], NO_RECORD, OK


def weighted_sizes(perm, head, weight):
    """What fqd_cluster_weights writes: size[perm[s]] = the sum of weight[perm[k]] over the run that starts at s where head[s],
    0 elsewhere; and (record at the head place, sum) of the run above 2^31-1 with the lowest such record, None for none."""
    n = len(perm)
    size, over = [0] * n, None
    k = 0
    while k < n:
        end = k + 1
        while end < n and not head[end]:
            end += 1
        total = sum(int(weight[perm[j]]) for j in range(k, end))
        if total > MAX:
            if over is None or perm[k] < over[0]:
                over = (int(perm[k]), total)
        else:
            size[perm[k]] = total
        k = end
    return size, over


def relabelled(record: bytes, size: int) -> bytes:
    """The record with the label in its annotation's place (at the first word's end where it has none)."""
    nl = record.find(b"\n")
    _, at, cut, reason = parse(record[:nl + 1] if nl >= 0 else record)
    assert reason == OK
    return record[:at] + sizes.label(size) + record[at + cut:]


def dedup_weighted(inputs, fasta=False, best=False, keys=None, sizeout=True, by_size=False, lo=1, hi=None):
    """inputs: file contents (1 or 2) whose ID lines may carry annotations; keys as in size_reference.dedup_sized.  Returns
    (outputs, the `.duplevels` text, total, duplicates, clusters not written, their weighted records, the weighted sizes of
    the written clusters in written order)."""
    files = [fast.parse(x, fasta) for x in inputs]
    n = len(files[0])
    assert all(len(f) == n for f in files)
    weight, _, _, bad, _ = annotations([r[1] for r in files[0]])
    assert bad == NO_RECORD
    if len(files) == 2:
        assert annotations([r[1] for r in files[1]], weight)[3] == NO_RECORD
    if keys is None:
        keys = [tuple(f[i][2] for f in files) for i in range(n)]
    groups = fast.clusters_of(keys)
    scores = [min(fast.SAT, sum(fast.score(f[i][0]) for f in files)) for i in range(n)]
    total_of = [sum(weight[i] for i in g) for g in groups]
    assert max(total_of, default=0) <= MAX

    def outside(t):
        return t < lo or bool(hi and t > hi)

    written = [(fast.pick(g, scores) if best else g[0], t, g[0]) for g, t in zip(groups, total_of) if not outside(t)]
    gone = [t for t in total_of if outside(t)]
    if by_size:
        written.sort(key=lambda t: (-t[1], t[2]))
    else:
        written.sort(key=lambda t: t[0])
    outputs = [b"".join(relabelled(f[w][0], size) if sizeout else f[w][0] for w, size, _ in written) for f in files]
    return outputs, sizes.duplevels_text(total_of), n, n - len(groups), len(gone), sum(gone), [size for _, size, _ in written]
