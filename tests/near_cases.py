"""Inputs for the tests of FQD_FAST_HAMMING=D: edge lists for the label sweeps (tests/test_near_core.py and the native harness)
and builders of reads whose differences fall where the seed join can go wrong (tests/test_gpu_near.py).  A record is a tuple
of mates (1 or 2 byte strings); every builder takes its random.Random, so a case is the same in every run."""
import near_reference as ref

LETTERS = b"ACGT"
LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 151, 255, 256, 257]     # and D, D + 1, D + 2: lengths_for(D)
GROUP_SIZES = [1, 2, 3, 8, 9, 63, 64, 65, 255, 256, 257, 4096]
PREFIX = 16                                                    # group_records: the constant bytes in front, which cover segment 0
DIGITS = 7                                                     # base-4 digits of a node's number: 4^7 > 4097


def lengths_for(D):
    return sorted(set(LENGTHS + [D, D + 1, D + 2]))


# ---- edge lists ------------------------------------------------------------------------------------------------------------------

def graph_cases():
    """(name, places, edges)."""
    chain = [(k, k + 1) for k in range(39)]
    middle = list(range(20, 0, -1)) + list(range(0, 1)) + list(range(21, 40))      # place 0 stands in the middle of the chain
    return [
        ("nothing", 0, []),
        ("one place", 1, []),
        ("no edge", 5, []),
        ("one edge", 2, [(1, 0)]),
        ("chain of 40", 40, chain),
        ("chain of 40, edges turned and shuffled", 40, [(b, a) for a, b in chain[::3] + chain[1::3] + chain[2::3]]),
        ("chain of 40, the lowest place at the far end", 40, [(39 - a, 39 - b) for a, b in chain]),
        ("chain of 40, the lowest place in the middle", 40, [(middle[k], middle[k + 1]) for k in range(39)]),
        ("chain whose labels fall against the order", 40, [((k * 7) % 40, ((k + 1) * 7) % 40) for k in range(39)]),
        ("star", 31, [(0, k) for k in range(1, 31)]),
        ("star, the centre is the highest place", 31, [(30, k) for k in range(30)]),
        ("two components", 10, [(0, 2), (2, 4), (1, 3), (3, 5), (5, 9)]),
        ("every edge three times", 6, [(0, 1), (1, 2), (4, 5)] * 3),
        ("ring", 17, [(k, (k + 1) % 17) for k in range(17)]),
        ("places no edge names", 12, [(3, 7), (7, 11)]),
    ]


def random_graph(rng, places, edges):
    return [(rng.randrange(places), rng.randrange(places)) for _ in range(edges)] if places else []


# ---- reads -------------------------------------------------------------------------------------------------------------------------

def template(rng, length):
    return bytes(rng.choice(LETTERS) for _ in range(length))


def substituted(seq, positions, rng=None, letter=None):
    """seq with another letter at every position."""
    s = bytearray(seq)
    for p in positions:
        s[p] = letter if letter is not None else rng.choice([c for c in LETTERS if c != s[p]])
    return bytes(s)


def position_sets(rng, length, D):
    """(name, positions): where the differences of a pair fall.  Only sets of distinct positions inside the read come back."""
    b = [ref.bound(length, D, j) for j in range(D + 2)]
    sets = []
    edges = sorted({p for p in [0, length - 1] + [x - 1 for x in b] + b if 0 <= p < length})
    for p in edges:                                            # one edge position, filled up to D and to D + 1 differences
        others = [q for q in range(length) if q != p]
        rng.shuffle(others)
        for count in (1, D, D + 1):
            sets.append((f"byte {p} and {count - 1} more", [p] + others[:count - 1]))
    for count in (D, D + 1):
        sets.append((f"the first {count}", list(range(count))))
        sets.append((f"the last {count}", list(range(length - count, length))))
        sets.append((f"{count} anywhere", rng.sample(range(length), count) if length >= count else [-1]))
    for j in range(D + 1):                                     # all D in one segment
        sets.append((f"all in segment {j}", list(range(b[j], b[j] + D)) if b[j + 1] - b[j] >= D else [-1]))
        sets.append((f"all at the end of segment {j}", list(range(b[j + 1] - D, b[j + 1])) if b[j + 1] - b[j] >= D else [-1]))
    for j in range(D + 1):                                     # one in each segment but j: only seed j finds the pair
        rest = [s for s in range(D + 1) if s != j]
        if all(b[s + 1] > b[s] for s in range(D + 1)):
            for pick in (lambda s: b[s], lambda s: b[s + 1] - 1, lambda s: rng.randrange(b[s], b[s + 1])):
                clean = [pick(s) for s in rest]
                sets.append((f"only segment {j} clean", clean))
                sets.append((f"one in every segment, segment {j} the last", clean + [pick(j)]))
    return [(name, ps) for name, ps in sets if len(set(ps)) == len(ps) and all(0 <= p < length for p in ps)]


def mate2_length(length):
    """The length of mate 2 in difference_pairs' pairs whose mate 1 has `length` bytes."""
    return (length * 7 + 3) % 41


def difference_pairs(rng, length, D, paired):
    """(name, record a, record b, near): pairs of one shape, each on a template of its own."""
    out = []
    len2 = mate2_length(length) if paired else 0
    def rec(m1, m2):
        return (m1, m2) if paired else (m1,)
    for name, ps in position_sets(rng, length, D):
        t1, t2 = template(rng, length), template(rng, len2)
        out.append((name, rec(t1, t2), rec(substituted(t1, ps, rng), t2), len(ps) <= D))
    for at in sorted({0, length // 2, length - 1} & set(range(length))):       # 'N' is a letter
        t1, t2 = substituted(template(rng, length), [at], letter=ord("N")), template(rng, len2)
        others = [q for q in range(length) if q != at]
        rng.shuffle(others)
        if len(others) >= D:
            out.append((f"N at {at} in both, {D} elsewhere", rec(t1, t2), rec(substituted(t1, others[:D], rng), t2), True))
            out.append((f"N at {at} against a base, {D} elsewhere", rec(t1, t2), rec(substituted(substituted(t1, [at], rng), others[:D], rng), t2), False))
        out.append((f"N at {at} against a base", rec(t1, t2), rec(substituted(t1, [at], rng), t2), True))
    if paired and len2 >= D + 1:
        for name, ps1, ps2 in [("D in each mate", range(D), range(D)), ("D + 1 in mate 2 alone", [], range(D + 1)),
                               ("mate 2's first and last byte", [], sorted({0, len2 - 1})[:D]), ("mate 2's last bytes", [], range(len2 - D, len2)),
                               ("D in mate 1, D + 1 in mate 2", range(D), range(len2 - D - 1, len2))]:
            if length < len(ps1):
                continue
            t1, t2 = template(rng, length), template(rng, len2)
            out.append((name, rec(t1, t2), rec(substituted(t1, ps1, rng), substituted(t2, ps2, rng)), len(ps1) <= D and len(ps2) <= D))
    return out


def every_short_read(length):
    """All reads of a length over ACGN (625 at most)."""
    reads = [b""]
    for _ in range(length):
        reads = [r + bytes([c]) for r in reads for c in b"ACGN"]
    return reads


def scattered(rng, nodes, copies=(0, 1, 1, 2)):
    """The nodes in a random order with copies of each scattered through the input."""
    records = list(nodes)
    for v in nodes:
        records += [v] * rng.choice(copies)
    rng.shuffle(records)
    return records


def chain_nodes(rng, D, links=40, length=150):
    """Node k differs from node k + 1 in exactly D positions and from every other node in at least 2 D."""
    assert links * D <= length
    t = template(rng, length)
    nodes = [t]
    for k in range(links - 1):
        nodes.append(substituted(nodes[-1], range(k * D, k * D + D), rng))
    return nodes


def star_nodes(rng, D, leaves=30, length=150):
    t = template(rng, length)
    return [t] + [substituted(t, range(k * D, k * D + D), rng) for k in range(leaves)]


def group_records(rng, D, size, paired=False, near_copy=True):
    """`size` nodes that agree on segment 0 (PREFIX constant bytes) and differ pairwise in more than D places behind it: every
    base-4 digit of a node's number is written D + 1 times.  near_copy (size >= 2): the last node is node 0 with an 'N' in its
    tail instead — one place from node 0, more than D from every other.  In a shuffled order."""
    prefix = template(rng, PREFIX)
    def tail(k):
        return b"".join(bytes([LETTERS[(k >> (2 * d)) & 3]]) * (D + 1) for d in range(DIGITS))
    assert ref.bound(PREFIX + DIGITS * (D + 1), D, 1) <= PREFIX
    nodes = [prefix + tail(k) for k in range(size - (1 if near_copy and size >= 2 else 0))]
    if near_copy and size >= 2:
        nodes.append(substituted(nodes[0], [PREFIX + 2], letter=ord("N")))
    mate2 = template(rng, 9)
    records = [(m, mate2) if paired else (m,) for m in nodes]
    rng.shuffle(records)
    return records


def random_records(rng, D, nodes=3000, templates=300, paired=False, lengths=(30, 31, 32, 47, 48, 49, 100, 150)):
    """Nodes made of `templates` templates with 0 .. D + 2 substitutions a mate, copies scattered among them."""
    made = []
    for _ in range(templates):
        length = rng.choice(lengths)
        made.append((template(rng, length), template(rng, rng.choice(lengths))))
    out = []
    for _ in range(nodes):
        t1, t2 = rng.choice(made)
        m1 = substituted(t1, rng.sample(range(len(t1)), rng.randrange(D + 3)), rng)
        m2 = substituted(t2, rng.sample(range(len(t2)), rng.randrange(D + 3)), rng)
        out.append((m1, m2) if paired else (m1,))
    return scattered(rng, out, copies=(0, 0, 1, 2))
