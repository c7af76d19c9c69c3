"""Lists of reads for hamming_walk_kernel (csrc/fqd_seq.hip), laid out so that their sorted order and their heads are
known by construction.  A wave of the kernel compares the 64 sorted places after the current one with the head at once
and jumps by ballot; fqdseq::mismatches (csrc/fqd_seq_core.hpp) counts eight bytes a step and the rest byte by byte.

Every list is built IN SORTED ORDER as (record, head flag) and handed out shuffled.  A record is a tuple of one or two
mates.  A read is a fixed-width prefix — its cluster's number in base 4 over ACGT, ascending — and a body.  A cluster's
head body is made of 'A' and 'C'; a member substitutes 'G' at chosen body positions, which makes it sort after every
read whose first substitution comes later.  With an 8-byte prefix and a 29-byte body (reads of 37 bytes) the body
positions 0, 7, 8 are the edges of the second and third 8-byte word, 23 is the last word's last byte, 24 the first tail
byte, 28 the last byte.

tests/test_edge_inputs.py holds the lists to these claims with tests/seq_reference.py; tests/test_gpu_hamming_walk.py
holds the device sort and heads to the same reference on them."""
import numpy as np

SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 200)
LEADS = (0, 1, 62, 63)                                       # single-record clusters in front
N_MODS = (0, 1, 63)
DISTANCES = (0, 1, 2, 5)
LARGE_DISTANCES = (37, 1000, 2**31 - 1, 2**31, 2**32 - 1)
SPECIAL = (0, 7, 8, 23, 24, 28)                              # body positions, 29-byte body behind an 8-byte prefix


def prefix(c: int, width: int) -> bytes:
    assert 0 <= c < 4 ** width
    return bytes(b"ACGT"[(c >> (2 * (width - 1 - k))) & 3] for k in range(width))


def sub(read: bytes, positions, offset: int = 0, letter: bytes = b"G") -> bytes:
    s = bytearray(read)
    for p in positions:
        assert s[offset + p] in b"AC"
        s[offset + p] = letter[0]
    return bytes(s)


def ham(a: bytes, b: bytes) -> int:
    assert len(a) == len(b)
    return sum(x != y for x, y in zip(a, b))


def head_body(rng, c: int, length: int) -> bytearray:
    """'A'/'C' at random; a stretch that is all 'A' in even clusters and all 'C' in odd ones keeps the first read of a
    cluster more than any tested distance from every read of the cluster before it."""
    body = bytearray(np.frombuffer(b"AC", np.uint8)[rng.integers(0, 2, length)].tobytes())
    lo, hi = (9, 23) if length >= 24 else (0, length)
    body[lo:hi] = (b"A" if c % 2 == 0 else b"C") * (hi - lo)
    return body


def plan(length: int, d: int, rot: int):
    """Positions of a cluster: A and A2 (d each, A2 before A), e2 < e before both, x a spare late one."""
    if length >= 29:
        late = (28, 24, 23)[rot % 3]
        e, e2 = ((8, 7), (7, 0), (8, 0))[rot % 3]
    else:
        assert d <= 1 and length >= 3
        late, e, e2 = length - 1, 0, None
    a = [late - i for i in range(d)]
    a2 = [late - d - i for i in range(d)]
    assert not a2 or min(a2) > e
    x = next(p for p in range(length - 1, e, -1) if p not in a)
    return a, a2, e, e2, x


def cluster(read: bytes, w: int, m: int, d: int, rot: int):
    """m records under one prefix, ascending, with their head flags.  From five (six with Z) records on:

        H            the head
        H ...        copies of it
        D1 = H+A     exactly d from H: a member
        D2 = H+A2    exactly d from H and 2d from its neighbour D1, which is no certain cut: a member
        H2 = H+e+A   d + 1 from H, 2d + 1 from its neighbour D2 (a certain cut): a head
        X  = H2+x    1 from H2 and d + 2 from H: a member of H2 (for d = 0 a head)
        Z  = H+e2    1 from H but d + 2 from H2, the head it is measured from: a head
        Z+...        Z with up to d more substitutions: members of Z
    """
    body_len = len(read) - w
    a, a2, e, e2, x = plan(body_len, d, rot)
    S = lambda pos: sub(read, pos, w)
    H, D1, D2, H2, X = read, S(a), S(a2), S([e] + a), S([e] + a + [x])
    core = [(H, 1), (D1, 0), (D2, 0), (H2, 1), (X, 1 if d == 0 else 0)]
    if e2 is not None:
        core.append((S([e2]), 1))
    if m == 2:
        return [(H, 1), (H2, 1)]
    if m < len(core):
        return [(H, 1)] + [(H, 0)] * (m - 1)
    fill = m - len(core)
    out = [(H, 1)] + [(H, 0)] * (fill // 2) + core[1:]
    rest = fill - fill // 2
    if e2 is None:
        out += [(X, 0)] * rest
    else:
        out += sorted((S([e2] + a[:j % (d + 1)]), 0) for j in range(rest))
    assert len(out) == m
    return out


def main_list(d: int, lead: int, n_mod: int, seed: int, w: int = 8, body: int = 29, sizes=SIZES, walk_d=None):
    """`lead` single-record clusters, then the sizes in a seeded order, then one cluster that brings n to n_mod (mod 64).
    Built for distance d; walk_d (default d) is the distance the flags are for: any walk_d >= the read length makes
    the whole list one cluster."""
    rng = np.random.default_rng(seed)
    ms = [1] * lead + [int(s) for s in rng.permutation(sizes)]
    tail = (n_mod - sum(ms)) % 64
    if tail:
        ms.append(tail)
    out = []
    for c, m in enumerate(ms):
        read = prefix(c, w) + bytes(head_body(rng, c, body))
        out += cluster(read, w, m, d, rot=c)
    assert len(out) % 64 == n_mod
    if walk_d is not None and walk_d >= w + body:
        out = [(r, 1 if k == 0 else 0) for k, (r, _) in enumerate(out)]
    return [((r,), f) for r, f in out]


def short_list(d: int, n_mod: int, seed: int):
    """Reads of 5 bytes (a 2-byte prefix, a 3-byte body): less than one 8-byte word, so only the tail loop counts."""
    return main_list(d, 0, n_mod, seed, w=2, body=3, sizes=(1, 2, 63, 64, 65))


def drift_list(d: int, seed: int = 5):
    """Chains: record i substitutes i positions, one more than record i - 1, so neighbours are 1 apart (never a head by
    a neighbour's measure for d >= 1) while the distance to the head grows by one a record: every (d + 1)-th is a head."""
    rng = np.random.default_rng(seed)
    orders = [list(SPECIAL) + [p for p in range(28, 0, -1) if p not in SPECIAL], list(range(28, -1, -1)), list(range(29))]
    out = []
    for c, order in enumerate(orders):
        read = prefix(c, 8) + bytes(head_body(rng, c, 29))
        for i in range(len(order) + 1):
            out.append(((sub(read, order[:i], 8),), 1 if i % (d + 1) == 0 else 0))
    return out


def neighbour_heads(d: int, records):
    """The WRONG rule the drift chains tell apart: a record is a head iff it does not match the record before it."""
    out = [1]
    for p, x in zip(records, records[1:]):
        out.append(0 if all(len(a) == len(b) and ham(a, b) <= d for a, b in zip(p, x)) else 1)
    return out


def mixed_length_list(d: int, seed: int = 6):
    """Reads of 36 and 37 bytes under one prefix: 'b' sorts before 'b' + a letter.  A change of length is a head."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(40):
        b36 = prefix(c, 8) + bytes(head_body(rng, c, 28))
        later = sub(b36, [SPECIAL[c % 5]], 8)                # 36 bytes again, after every 37-byte read that starts with b36
        out += [((b36,), 1), ((b36,), 0),
                ((b36 + b"A",), 1), ((b36 + b"A",), 0), ((b36 + b"C",), 0 if d >= 1 else 1),
                ((later,), 1), ((later + b"A",), 1), ((later + b"A",), 0)]
    return out


def pair_list(d: int, seed: int = 7):
    """Pairs of 37-byte mates, one scenario per cluster of two, the cluster's number in mate 1's prefix:
        0  mate 1 at d, mate 2 at d + 1                 a head
        1  mate 1 at d + 1, mate 2 at d                 a head
        2  mate 1 identical, mate 2 one byte longer     a head
        3  both mates at exactly d (2d in all)          a member
        4  mate 2 empty on both, mate 1 at d            a member
    with single pairs between them so that the clusters straddle the 64-place chunks at every offset."""
    rng = np.random.default_rng(seed)
    out, c = [], 0
    for rep in range(60):
        kind = rep % 5
        m1 = prefix(c, 8) + bytes(head_body(rng, c, 29))
        m2 = bytes(head_body(rng, c + 1, 37))
        a, a2, e, e2, x = plan(29, d, rep)
        p1, p2 = [q + 8 for q in a], [q + 8 for q in a2]     # mate 2 has no prefix: any of its 37 bytes will do
        if kind == 0:
            second, flag = (sub(m1, a, 8), sub(m2, p2 + [e])), 1
        elif kind == 1:
            second, flag = (sub(m1, a + [e], 8), sub(m2, p2)), 1
        elif kind == 2:
            m2 = m2[:36]
            second, flag = (m1, m2 + b"A"), 1
        elif kind == 3:
            second, flag = (sub(m1, a, 8), sub(m2, p1)), 0
        else:
            m2 = b""
            second, flag = (sub(m1, a, 8), b""), 0
        out += [((m1, m2), 1), (second, flag)]
        c += 1
        for _ in range(rep % 3):                             # 0, 1 or 2 single pairs: the clusters' places drift over the chunks
            out.append(((prefix(c, 8) + bytes(head_body(rng, c, 29)), bytes(head_body(rng, c + 1, 37))), 1))
            c += 1
    return out


def shuffled(layout, seed: int = 99):
    """The records of a layout in a seeded input order."""
    order = np.random.default_rng(seed).permutation(len(layout))
    return [layout[i][0] for i in order]


def records(layout):
    return [r for r, _ in layout]


def flags(layout):
    return [f for _, f in layout]


def main_lists(d: int, walk_d=None):
    """(name, layout) of the main list at every lead and total, each in another order of the cluster sizes."""
    for lead in LEADS:
        for n_mod in N_MODS:
            yield f"lead{lead}_mod{n_mod}", main_list(d, lead, n_mod, seed=100 * d + 10 * lead + n_mod, walk_d=walk_d)


def all_lists(d: int):
    """Every (name, layout) that is walked at distance d (one of DISTANCES)."""
    yield from main_lists(d)
    if d <= 1:
        for n_mod in N_MODS:
            yield f"short_mod{n_mod}", short_list(d, n_mod, seed=40 + n_mod)
    if d >= 1:
        yield "drift", drift_list(d)
    yield "mixed_lengths", mixed_length_list(d)
    yield "pairs", pair_list(d)


def large_distance_lists(d: int):
    """(name, layout) for a distance no read can exceed: lists built for d = 2, one cluster per run of equal lengths."""
    yield "main", main_list(2, 1, 63, seed=8, walk_d=d)
    yield "mixed_lengths", mixed_length_list(d)
    pairs = pair_list(2)
    out, prev = [], None
    for r, _ in pairs:                                       # a pair is a head iff a mate's length changes
        lens = tuple(len(m) for m in r)
        out.append((r, 1 if lens != prev else 0))
        prev = lens
    yield "pairs", out
