"""The ID join (csrc/fqd_join.hip) restated on the host, and tag lists built around its structure: the code width of a
position on both sides of every power of two, the END code on both sides of min_len, fields across the 64-bit key words,
the census' LDS rows, whole-tag compares around 32 and 64 bytes, the radix tiles, and runs of one tag laid on the edges
of the join's tiles.  Plain Python and numpy: tests/test_edge_inputs.py holds every list to its own claims on the host,
tests/test_gpu_join_edges.py runs them on the device.

The coding, from the header comment of fqd_join.hip and not from its kernels: position p of a tag has the codes 0 = "the
tag has ended" (only where p >= min_len, the shortest tag's length) and then the byte values that occur at p, in byte
order; a position's field is as wide as the number of its codes needs, and no field where there is one code; the key is
the fields side by side, position 0 most significant.  Byte 0 is a byte like any other."""
from functools import lru_cache
import random

NONE = 0xFFFFFFFF
SORT_TILE, JOIN_TILE, PAIR_TILE, CENSUS_LDS = 4096, 2048, 2048, 160


# ---- the rule ----------------------------------------------------------------------------------------------------------
class CodeTable(tuple):
    """(min_len, max_len, width[], lsb[], B); .rank[p] maps a byte value at p to its code (END included where it exists)."""
    min_len = property(lambda s: s[0]); max_len = property(lambda s: s[1])
    width = property(lambda s: s[2]); lsb = property(lambda s: s[3]); B = property(lambda s: s[4])


def code_table(tags):
    lens = [len(t) for t in tags]
    min_len, max_len = min(lens), max(lens)
    width, rank = [], []
    for p in range(max_len):
        present = sorted({t[p] for t in tags if len(t) > p})
        end = 1 if p >= min_len else 0
        codes = len(present) + end
        width.append(0 if codes <= 1 else (codes - 1).bit_length())
        rank.append({c: k + end for k, c in enumerate(present)})
    lsb, bits = [0] * max_len, 0
    for p in reversed(range(max_len)):
        lsb[p] = bits
        bits += width[p]
    table = CodeTable((min_len, max_len, width, lsb, bits))
    table.rank = rank
    return table


def key_of(tag, table):
    key = 0
    for p, w in enumerate(table.width):
        if w and p < len(tag):
            key |= table.rank[p][tag[p]] << table.lsb[p]
    return key


def reference_sort(tags):
    """The order of fqd_sort_tags: bytes over the shorter length, shorter first, equal tags in input order."""
    return sorted(range(len(tags)), key=tags.__getitem__)


def reference_join(a, b):
    perm_a, perm_b = reference_sort(a), reference_sort(b)
    where_a, where_b = {}, {}                                  # tag -> its sorted positions, ascending
    for k, r in enumerate(perm_a):
        where_a.setdefault(a[r], []).append(k)
    for k, r in enumerate(perm_b):
        where_b.setdefault(b[r], []).append(k)
    match_a, match_b = [NONE] * len(a), [NONE] * len(b)
    for tag, ka in where_a.items():
        for x, y in zip(ka, where_b.get(tag, ())):             # the k-th with the k-th
            match_a[x], match_b[y] = y, x
    pairs = [(perm_a[x], perm_b[y]) for x, y in enumerate(match_a) if y != NONE]      # sorted positions of file 1 = tag order
    return dict(perm_a=perm_a, perm_b=perm_b, match_a=match_a, match_b=match_b, pairs=pairs)


def sorted_union(a, b):
    """(tag, file, record) of the union in the join's order: by tag, file 1 first, then input order."""
    u = [(t, 0, i) for i, t in enumerate(a)] + [(t, 1, i) for i, t in enumerate(b)]
    return sorted(u, key=lambda x: x[0])                       # stable: the union lists file 1 first


def ref_tag(line: bytes):
    """FastqViewWithId::read_new restated: (offset, length) of the tag in the ID line (tests/test_gpu_join.py's)."""
    dot = line.find(b".")
    start = dot + 1 if dot >= 0 else 1
    sp = line.find(b" ", start)
    return start, (sp if sp >= 0 else len(line)) - start


def deciders(tags, table, pos, bit):
    """Which part of the field at `pos`, cut at key bit `bit`, and which neighbour position first tells two tags that
    are neighbours in sorted order apart: a subset of {"high", "low", "before", "after"}."""
    keys = sorted({key_of(t, table) for t in tags})
    lo, hi = table.lsb[pos], table.lsb[pos] + table.width[pos]
    varying = [p for p, w in enumerate(table.width) if w]
    before, after = varying[varying.index(pos) - 1], varying[varying.index(pos) + 1]
    seen = set()
    for x, y in zip(keys, keys[1:]):
        top = (x ^ y).bit_length() - 1                         # the most significant bit that differs decides
        if bit <= top < hi:
            seen.add("high")
        elif lo <= top < bit:
            seen.add("low")
        elif table.lsb[before] <= top < table.lsb[before] + table.width[before]:
            seen.add("before")
        elif table.lsb[after] <= top < table.lsb[after] + table.width[after]:
            seen.add("after")
    return seen


def tag_arrays(tags):
    """(bytes with 16 of slack, offsets, lengths) as the library and the oracle take them."""
    import numpy as np
    lens = np.array([len(t) for t in tags], dtype=np.uint32)
    offs = np.zeros(len(tags), dtype=np.uint64)
    if len(tags):
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(tags) + b"\0" * 16, dtype=np.uint8).copy(), offs, lens


def shuffled(items, seed):
    items = list(items)
    random.Random(seed).shuffle(items)
    return items


def spread(k):
    """k byte values in order, bytes 0 and 255 among them (k >= 2)."""
    return sorted({(i * 255) // (k - 1) for i in range(k)})


def bits_for(codes):
    return 0 if codes <= 1 else (codes - 1).bit_length()


# ---- code widths -------------------------------------------------------------------------------------------------------
FIXED_KS = sorted({k for w in range(1, 9) for k in (2 ** (w - 1) + 1, 2 ** w)})   # 2, 3, 4, 5, 8, 9, ..., 129, 256
RAGGED_KS = sorted({k for w in range(1, 9) for k in (2 ** w - 1, 2 ** w)})       # 1, 2, 3, 4, 7, 8, ..., 255, 256
MINLEN_KS = [3, 4, 7, 8, 255, 256]


def width_fixed(k):
    """Three bytes, the middle one with k values, no END anywhere."""
    vals = spread(k)
    tags = [bytes([65 + (i // k) % 3, vals[i % k], 97 + (i // (3 * k) + i) % 3]) for i in range(max(4 * k, 60))]
    return shuffled(tags, k), dict(min_len=3, max_len=3, widths={0: 2, 1: bits_for(k), 2: 2}, B=4 + bits_for(k))


def width_ragged(k):
    """Lengths 1, 2 and 3: position 1 has k values and END."""
    vals = spread(k) if k > 1 else [0]
    tags = [bytes([65 + i % 3]) for i in range(7)]
    tags += [bytes([65 + (i // k) % 3, vals[i % k]]) + (bytes([97 + i % 3]) if i % 4 else b"") for i in range(max(4 * k, 60))]
    return shuffled(tags, 1000 + k), dict(min_len=1, max_len=3, widths={0: 2, 1: bits_for(k + 1), 2: 2}, B=4 + bits_for(k + 1))


def width_at_min_len(k, at_min_len):
    """min_len = 3, held by exactly one record; every other tag has 5 bytes.  The probe with k values lies at position 2
    (no END) or at position 3 (END)."""
    vals, probe = spread(k), 3 if at_min_len else 2
    tags = []
    for i in range(max(3 * k, 40)):
        t = bytearray([97 + (i // k) % 2, 98, 99, 100, 48 + i % 3])
        t[probe] = vals[i % k]
        tags.append(bytes(t))
    tags.append(tags[k // 2][:3])
    widths = {0: 1, 1: 0, 2: 0, 3: 1, 4: 2}                    # positions 3 and 4: one and three byte values, and END
    widths[probe] = bits_for(k + (1 if at_min_len else 0))
    return shuffled(tags, 2000 + 2 * k + at_min_len), dict(min_len=3, max_len=5, widths=widths, B=sum(widths.values()), n_min_len=1)


def prefix_chain():
    """Every prefix of two chains of 20 bytes that part at byte 10, the empty tag among them, some twice."""
    rnd = random.Random(20)
    one = bytes([0, 255] + [rnd.randrange(256) for _ in range(18)])
    two = one[:10] + bytes([one[10] ^ 1]) + one[11:]
    tags = [one[:k] for k in range(21)] + [two[:k] for k in range(11, 21)] + [one[:k] for k in range(0, 21, 3)] + [b"", two]
    widths = {p: 1 for p in range(20)}
    widths.update({10: 2})
    return shuffled(tags, 21), dict(min_len=0, max_len=20, widths=widths, B=21)


# ---- key-word edges ----------------------------------------------------------------------------------------------------
def crossing_ts(w, bit):
    every = list(range(bit - w + 1, bit))
    return every if w in (2, 5, 8) else sorted({every[0], every[-1]})


CROSSINGS = [(w, t, bit) for bit in (64, 128) for w in range(2, 9) for t in crossing_ts(w, bit)]
END_CROSSINGS = [56, 60, 63]


def crossing(w, t, bit):
    """[position 0: 8 bits][position 1: w bits][t positions of one bit], all tags 2 + t bytes: the field of position 1
    has its lowest bit at key bit t and so lies across `bit`.  Random records, and beside them pairs that differ in one
    place alone: the field's highest bit, its lowest bit, the position before and the position after."""
    rnd = random.Random(w * 1000 + t)
    k = 2 ** w

    def tail():
        return bytes(rnd.choice(b"01") for _ in range(t))
    tags = [bytes([(i * 37 + 11) % 256, i % k]) + tail() for i in range(300)]
    tags += [bytes([0, 0]) + b"0" * t, bytes([255, k - 1]) + b"1" * t]
    for i in range(4):
        base = bytearray(tags[i * 17])
        base[1] &= (k - 1) ^ 1 ^ (k >> 1)                      # room to raise the field's lowest and highest bit
        for place, flip in ((1, 1), (1, k >> 1), (0, 1), (2, 1)):
            v = bytearray(base)
            v[place] ^= flip
            tags += [bytes(base), bytes(v)]
    claims = dict(min_len=2 + t, max_len=2 + t, widths={0: 8, 1: w, 2: 1, 1 + t: 1}, B=8 + w + t, crosses=(1, bit),
                  decided_by={"high", "low", "before", "after"})
    return shuffled(tags, t), claims


def end_crossing(t):
    """[position 0: 8 bits][position 1: all 256 values and END = 9 bits][t positions of one byte value or END]: tags of 1
    byte, and of 2 .. 2 + t bytes that are all 'x' behind position 1."""
    rnd = random.Random(9000 + t)
    tags = [bytes([i % 256]) for i in range(0, 256, 5)]
    tags += [bytes([(i * 37 + 11) % 256, i % 256]) + b"x" * rnd.randrange(t + 1) for i in range(600)]
    tags += [bytes([7, c]) + b"x" * n for c in (0, 127, 128, 255) for n in (0, 1, t - 1, t)]
    tags += [bytes([7]), bytes([8]) + b"\0" + b"x" * t]
    claims = dict(min_len=1, max_len=2 + t, widths={0: 8, 1: 9, 2: 1, 1 + t: 1}, B=17 + t, crosses=(1, 64),
                  decided_by={"high", "low", "before", "after"})
    return shuffled(tags, t), claims


KEY_BITS = [63, 64, 65, 127, 128, 129, 130]


def one_bit_fields(bits):
    """Tags of `bits` bytes over '0' and '1': a field of one bit per position (130: 64 fields in a word, three words)."""
    rnd = random.Random(bits)
    tags = [bytes(rnd.choice(b"01") for _ in range(bits)) for _ in range(200)] + [b"0" * bits, b"1" * bits]
    for i in range(0, 40, 4):                                  # neighbours that differ in the last, the first, the 64th-last bit
        for place in {bits - 1, 0, bits - 64 if bits > 64 else 1, bits - 65 if bits > 65 else 2}:
            v = bytearray(tags[i]); v[place] ^= 1
            tags.append(bytes(v))
    tags += tags[:30]
    return shuffled(tags, bits + 1), dict(min_len=bits, max_len=bits, widths={0: 1, bits - 1: 1}, B=bits)


def no_bits():
    return [("all_equal", [b"same tag"] * 300, dict(B=0)), ("all_empty", [b""] * 300, dict(B=0, max_len=0)),
            ("one_record", [b"alone"], dict(B=0)), ("one_empty_record", [b""], dict(B=0, max_len=0))]


# ---- census ------------------------------------------------------------------------------------------------------------
CENSUS_LENGTHS = [159, 160, 161, 162]


def census_last(length):
    """Constant but for the last position, which takes 200 values."""
    body = bytes((7 * p) % 251 + 1 for p in range(length - 1))
    tags = [body + bytes([c]) for c in spread(200)] + [body + bytes([c]) for c in (0, 255, 128)]
    return shuffled(tags, length), dict(min_len=length, max_len=length, widths={0: 0, length - 2: 0, length - 1: 8}, B=8)


def census_four():
    """162 bytes, five values at each of the positions 158 .. 161 and nowhere else."""
    rnd = random.Random(158)
    body = bytes((5 * p) % 250 + 3 for p in range(158))
    vals = [0, 64, 65, 200, 255]
    tags = [body + bytes(rnd.choice(vals) for _ in range(4)) for _ in range(500)]
    return tags, dict(min_len=162, max_len=162, widths={157: 0, 158: 3, 159: 3, 160: 3, 161: 3}, B=12)


# ---- heads -------------------------------------------------------------------------------------------------------------
HEAD_LENGTHS = [31, 32, 33, 39, 40, 41, 63, 64, 65, 96, 97]


def head_groups(length):
    """256 groups of tags of `length` bytes with the group's own first 8 bytes (every byte value at each of them); within
    a group the tags differ in the last byte alone, in byte length - 9 alone, or not at all.  Returns (file 1, file 2)."""
    a, b = [], []
    for g in range(256):
        base = bytearray(bytes((g * (2 * j + 1) + j) % 256 for j in range(8)) + bytes(range(100, 100 + length - 8)))
        place = (length - 1, length - 9, None)[g % 3]
        for v in range(3):
            t = bytearray(base)
            if place is not None:
                t[place] = (0, 128, 255)[v]
            (a if (g + v) % 4 else b).append(bytes(t))
            (b if (g * 3 + v) % 5 else a).append(bytes(t))
    return shuffled(a, length), shuffled(b, length + 500)


def head_claims(length):
    return dict(min_len=length, max_len=length, widths={0: 8, 7: 8, 8: 0, length - 9: 2, length - 1: 2}, B=68)


def head_lengths_differ():
    """Equal first bytes and different lengths: a tag, the tag without its last byte, and the tag with one byte more."""
    a, b = head_groups(40)
    a, b = a[:300], b[:300]
    t = a[0]
    a += [t[:-1], t + b"\0", t, t + b"\0"]
    b += [t + b"\0", t[:-1], t[:-1]]
    return a, b


# ---- stability and tiles of the radix passes ---------------------------------------------------------------------------
STABLE_NS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289]
STABLE_KINDS = ["all_equal", "period_1", "period_64", "period_1024", "bytes_256", "last_pass_3_bits"]


@lru_cache(maxsize=None)
def stable_tags(n, kind):
    rnd = random.Random(n)
    if kind == "all_equal":
        return [b"equal"] * n
    if kind.startswith("period_"):
        period = int(kind[7:])
        return [(b"b", b"a")[(i // period) % 2] for i in range(n)]
    if kind == "bytes_256":                                    # every digit of a pass, each n / 256 times (the first n % 256 once more)
        return shuffled([bytes([i % 256]) for i in range(n)], n)
    return [bytes([rnd.randrange(8) * 31, rnd.randrange(256)]) for _ in range(n)]         # 3 + 8 bits: passes of 8 and of 3


def stable_claims(n, kind):
    if kind == "all_equal" or n == 1:
        return dict(B=0)
    if kind.startswith("period_"):
        return dict(B=1 if n > int(kind[7:]) else 0)
    if kind == "bytes_256":
        return dict(B=bits_for(min(n, 256)))
    return dict(B=11) if n >= 4095 else {}


# ---- run placement -----------------------------------------------------------------------------------------------------
# (singletons below, [(records of file 1, records of file 2) of each hot tag, in tag order]); the run of the first hot tag
# starts at union place s, its file-2 part at s + ra
RUN_LAYOUTS = [
    (2047, [(5, 3)]), (2048, [(3, 5)]), (2049, [(4, 4)]),                          # the run starts around a tile's edge
    (2040, [(8, 6)]), (3000, [(1096, 10)]),                                        # file 2's part starts a tile
    (2040, [(8, 2048 + 10)]), (2040, [(8, 4096 + 10)]),                            # ... and covers one and two tiles without a head
    (1000, [(500, 5000)]), (1000, [(5000, 600)]),                                  # whole tiles inside either part
    (7, [(1, 3)]), (8, [(3, 1)]), (9, [(2, 2)]), (5, [(3, 2)]),                    # a thread's 8 elements
    (511, [(1, 3)]), (512, [(3, 1)]), (513, [(2, 2)]), (500, [(12, 20)]),          # a wave's 512
    (2040, [(8, 0), (0, 5)]), (2043, [(0, 5), (8, 0)]),                            # one file only, then the other file only
    (2048, [(6, 0), (0, 2048)]), (0, [(0, 2048), (3, 0)]),
    (10, [(2, 1), (1, 2), (0, 1), (1, 0), (3, 3)]),
]
RUN_STYLES = ["short", "hex30"]


@lru_cache(maxsize=None)
def run_case(which, style):
    s, runs = RUN_LAYOUTS[which]
    rnd = random.Random(which * 2 + (style == "hex30"))
    above = 300
    if style == "short":
        low = [b"a%05d" % k for k in range(s)]
        hot = [b"h%02d" % k for k in range(len(runs))]
        high = [b"z%05d" % k for k in range(above)]
    else:
        def draw(lead, count):
            out = set()
            while len(out) < count:
                out.add(bytes([rnd.choice(lead)]) + bytes(rnd.choice(b"0123456789abcdef") for _ in range(29)))
            return sorted(out)
        low, high = draw(b"0123456", s), draw(b"9abcdef", above)
        hot = [b"8" + b"%x" % k + b"7" * 28 for k in range(len(runs))]
    a, b = [], []
    for t in low + high:                                       # singletons: dealt to the two files
        (a if rnd.random() < 0.5 else b).append(t)
    for t, (ra, rb) in zip(hot, runs):
        a += [t] * ra
        b += [t] * rb
    ra, rb = runs[0]
    claims = dict(run_start=s, b_start=(s + ra) if rb else None, hot=hot[0])
    return shuffled(a, which), shuffled(b, which + 100), claims


# ---- pair compaction ---------------------------------------------------------------------------------------------------
PAIR_NS = [2047, 2048, 2049, 4097]
PAIR_PATTERNS = ["all", "none", "alternating", "last_of_tile", "first_of_next_tile"]


def pair_matched(n_a, pattern):
    """The sorted places of file 1 that have a partner.  last_of_tile: 2047, 4095, ... — and where file 1 ends before its
    first tile does, its last place; first_of_next_tile: 2048, 4096, ... — and where there is no second tile, place 0."""
    if pattern == "all":
        return list(range(n_a))
    if pattern == "none":
        return []
    if pattern == "alternating":
        return list(range(0, n_a, 2))
    if pattern == "last_of_tile":
        return list(range(PAIR_TILE - 1, n_a, PAIR_TILE)) or [n_a - 1]
    return list(range(PAIR_TILE, n_a, PAIR_TILE)) or [0]


@lru_cache(maxsize=None)
def pair_case(n_a, pattern):
    a = [b"p%05d" % k for k in range(n_a)]
    matched = pair_matched(n_a, pattern)
    b = [a[k] for k in matched] + [b"p%05d+" % k for k in range(0, n_a, 7)]       # and records of file 2 alone, in between
    return shuffled(a, n_a), shuffled(b, n_a + 1), dict(matched=matched)


# ---- limits ------------------------------------------------------------------------------------------------------------
def all_values_everywhere(length):
    """256 tags of `length` bytes, all 256 values at every position: tag i is the i-th smallest."""
    import numpy as np
    i, p = np.arange(256, dtype=np.int64)[:, None], np.arange(length, dtype=np.int64)[None, :]
    rows = ((i + (7 * p) * (p > 0)) % 256).astype(np.uint8)    # position 0 holds i: the order is known
    return [rows[k].tobytes() for k in range(256)]


# ---- extract_tags ------------------------------------------------------------------------------------------------------
NEAR = bytes([0x2F, 0x21, 0xAE, 0xA0])                         # '.' and ' ' with their lowest or their highest bit turned


def id_line(length, dot, space, phase, second_dot=None):
    """An ID line of `length` bytes, '\\n' included: near-miss bytes, a '.' at `dot` and a ' ' at `space` (None: none)."""
    if length == 1:
        return b"\n"
    line = bytearray(b"@" + bytes(NEAR[(k + phase) % 4] for k in range(1, length - 1)) + b"\n")
    for at, c in ((dot, 0x2E), (space, 0x20), (second_dot, 0x2E)):
        if at is not None:
            line[at] = c
    return bytes(line)


@lru_cache(maxsize=None)
def extract_lines():
    """The distinct ID lines; tests put each at every offset mod 8."""
    lines = []
    for length in range(1, 27):
        inner = [None] + list(range(1, length - 1))            # between the lead and the newline
        for dot in inner:
            for space in inner:
                if space is None or space != dot:
                    lines += [id_line(length, dot, space, phase) for phase in range(4)]
    for length in (64, 65, 66):
        for dot in range(56, length - 1):
            for space in (None, dot + 1 if dot + 1 < length - 1 else None, length - 2 if dot < length - 2 else None, 3):
                lines.append(id_line(length, dot, space, dot % 4, second_dot=None if dot + 2 >= length - 1 else length - 2))
    return sorted(set(lines))


@lru_cache(maxsize=None)
def extract_text():
    """(text, id_start[], id_len[], expected tag offset in the line [], expected tag length []): every line of
    extract_lines() at every start offset mod 8, a stretch of newlines between two lines."""
    parts, starts, lens, exp_off, exp_len, at = [], [], [], [], [], 0
    for k, line in enumerate(extract_lines()):
        o, n = ref_tag(line)
        for shift in range(8):
            pad = (shift - at) % 8 or 8
            parts.append(b"\n" * pad); at += pad
            starts.append(at); lens.append(len(line)); exp_off.append(o); exp_len.append(n)
            parts.append(line); at += len(line)
    return b"".join(parts), starts, lens, exp_off, exp_len


# ---- every sort case by name -------------------------------------------------------------------------------------------
def sort_cases():
    """(name, tags, claims) of every list that is sorted on its own (the stability lists and the limits excepted)."""
    for k in FIXED_KS:
        yield ("fixed_%d" % k, *width_fixed(k))
    for k in RAGGED_KS:
        yield ("ragged_%d" % k, *width_ragged(k))
    for k in MINLEN_KS:
        yield ("below_min_len_%d" % k, *width_at_min_len(k, False))
        yield ("at_min_len_%d" % k, *width_at_min_len(k, True))
    yield ("prefix_chain", *prefix_chain())
    for w, t, bit in CROSSINGS:
        yield ("cross_%d_w%d_t%d" % (bit, w, t), *crossing(w, t, bit))
    for t in END_CROSSINGS:
        yield ("end_cross_t%d" % t, *end_crossing(t))
    for bits in KEY_BITS:
        yield ("bits_%d" % bits, *one_bit_fields(bits))
    yield from no_bits()
    for length in CENSUS_LENGTHS:
        yield ("census_last_%d" % length, *census_last(length))
    yield ("census_158_161", *census_four())
    for length in HEAD_LENGTHS:
        a, b = head_groups(length)
        yield ("heads_%d" % length, a + b, head_claims(length))
    a, b = head_lengths_differ()
    yield ("heads_lengths_differ", a + b, dict(min_len=39, max_len=41))


def join_cases():
    """(name, file 1, file 2, claims) of every join case."""
    for length in HEAD_LENGTHS:
        yield ("heads_%d" % length, *head_groups(length), {})
    yield ("heads_lengths_differ", *head_lengths_differ(), {})
    for style in RUN_STYLES:
        for which in range(len(RUN_LAYOUTS)):
            yield ("run_%02d_%s" % (which, style), *run_case(which, style))
    for n_a in PAIR_NS:
        for pattern in PAIR_PATTERNS:
            yield ("pairs_%d_%s" % (n_a, pattern), *pair_case(n_a, pattern))
