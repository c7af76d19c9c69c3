"""The edge list of FQD_FAST_UMI_MISMATCH, shared by tests/test_umi_merge_core.py, tests/test_gpu_umi_merge.py and
tests/test_fast_umi_merge_cli.py.  A case is (name, D, records); a record is (UMI field as it stands in the ID line, (mate 1,
mate 2 or None)); all records of a case have one UMI shape.  `spread` turns (field, count) nodes into records so that the
nodes' first records stand in the listed order and the copies follow interleaved."""
import random

import strand_reference as strand

LETTERS = b"ACGTN"
LBS = (1, 15, 16, 17, 21, 22, 32, 33, 42, 43, 48, 49, 64)          # the word edges of 4-bit (16 a word) and 3-bit (21 a word) packings
SEQ_A, SEQ_B = b"ACGTACGTTGCATGCAGGAT", b"ACGTACGTTGCATGCAGGAA"
MATE_2, MATE_2B = b"TTGACCATGA", b"TTGACCATGC"


def hamming(a, b):
    assert len(a) == len(b)
    return sum(x != y for x, y in zip(a, b))


def bases(field):
    return bytes(c for c in field if c not in b"+-_")


def spread(nodes, seqs=(SEQ_A, None)):
    """[(field, count)] -> records: every node once in the listed order, then the further copies round-robin."""
    out = [(f, seqs) for f, _ in nodes]
    left = [[f, c - 1] for f, c in nodes]
    while any(c for _, c in left):
        for x in left:
            if x[1]:
                out.append((x[0], seqs))
                x[1] -= 1
    return out


def chain(length, L):
    """`length` strings of L letters: neighbours differ in ONE base, all others in two at least (laps of a thermometer:
    lap by lap every place moves on to the next letter, place after place)."""
    assert length <= 5 * L - 1
    out = []
    for t in range(length):
        lap, k = divmod(t, L)
        out.append(bytes([LETTERS[(lap + 1) % 5]] * k + [LETTERS[lap % 5]] * (L - k)))
    for i in range(length):
        for j in range(i + 1, length):
            assert (hamming(out[i], out[j]) == 1) == (j == i + 1), (length, L, i, j)
    return out


def mutate(u, *places, shift=1):
    v = bytearray(u)
    for p in places:
        v[p] = LETTERS[(LETTERS.index(v[p]) + shift) % 5]
    return bytes(v)


def lb_network(lb, rng):
    """A hub of count 9 with leaves one base off at the first, the last and the word-edge places, two bases off, and a
    second hub two bases off the first one's leaf."""
    hub = bytes(rng.choice(LETTERS) for _ in range(lb))
    places = sorted({p for p in (0, 14, 15, 16, 20, 21, 31, 32, 41, 42, 47, 48, 62, 63, lb - 1) if p < lb})
    nodes = [(hub, 9)] + [(mutate(hub, p), 1 + (k % 2) * 4) for k, p in enumerate(places)]
    if lb >= 2:
        nodes.append((mutate(hub, 0, lb - 1), 1))
        nodes.append((mutate(hub, 0, lb - 1, shift=2), 3))
    return nodes


def edge_cases():
    rng = random.Random(71)
    cases = []
    A = b"ACGTACGT"
    B, C2 = mutate(A, 3), mutate(A, 3, 5)
    for b in (1, 2, 3, 50):
        cases.append((f"threshold: {2 * b - 1} takes {b}", 1, spread([(A, 2 * b - 1), (B, b)])))
        if b > 1:                                                 # (no node has count 0)
            cases.append((f"threshold: {2 * b - 2} does not take {b}", 1, spread([(A, 2 * b - 2), (B, b)])))
            cases.append((f"threshold: {b} first, then {2 * b - 2}", 1, spread([(B, b), (A, 2 * b - 2)])))
        cases.append((f"threshold: {b} first, then {2 * b - 1}", 1, spread([(B, b), (A, 2 * b - 1)])))
    for D in (1, 2):
        far = mutate(A, *range(2 * D)) if D == 1 else mutate(A, 0, 1, 2, 3)
        mid = mutate(A, *range(D))
        assert hamming(A, mid) == D and hamming(mid, far) == D and hamming(A, far) == 2 * D
        cases.append((f"chain 10/5/3 at D={D}: all three", D, spread([(A, 10), (mid, 5), (far, 3)])))
        cases.append((f"chain 10/5/4 at D={D}: the last stays", D, spread([(A, 10), (mid, 5), (far, 4)])))
        cases.append((f"chain 3/5/10 in reversed input order at D={D}", D, spread([(far, 3), (mid, 5), (A, 10)])))
    X, V, Y = b"AAAAAAAA", b"AAACAAAA", b"AAACCAAA"
    cases.append(("two roots reach one node: the higher count wins", 1, spread([(Y, 8), (V, 2), (X, 10)])))
    cases.append(("two roots reach one node: equal counts, the earlier first wins", 1, spread([(Y, 8), (V, 2), (X, 8)])))
    cases.append(("two roots reach one node: equal counts, the other order", 1, spread([(X, 8), (V, 2), (Y, 8)])))
    for length, L in ((2, 8), (3, 8), (64, 16), (65, 16), (300, 64)):
        c = chain(length, L)
        cases.append((f"singleton chain of {length}", 1, spread([(u, 1) for u in c])))
        cases.append((f"singleton chain of {length}, reversed", 1, spread([(u, 1) for u in reversed(c)])))
        cases.append((f"singleton chain of {length} at D=2", 2, spread([(u, 1) for u in c])))
    cases.append(("N against a base", 1, spread([(b"ACGTACGN", 3), (b"ACGTACGT", 1), (b"NCGTACGT", 1), (b"NNNNNNNN", 1), (b"NNNNNNNA", 1)])))
    cases.append(("D=2: two off merges, three off does not", 2, spread([(A, 7), (mutate(A, 1, 6), 2), (mutate(A, 0, 2, 4), 2), (mutate(A, 7), 4)])))
    cases.append(("D=1: two off does not merge", 1, spread([(A, 7), (mutate(A, 1, 6), 2), (mutate(A, 7), 4)])))
    net = [(A, 6), (B, 2), (C2, 1), (mutate(A, 0), 3)]
    cases.append(("one UMI set under two sequences", 1, spread(net, (SEQ_A, None)) + spread(net, (SEQ_B, None))))
    cases.append(("one UMI set under two lengths of one sequence", 1, spread(net, (SEQ_A, None)) + spread(net, (SEQ_A[:-1], None))))
    cases.append(("pairs that differ only in mate 2", 1, spread(net, (SEQ_A, MATE_2)) + spread(net[:2], (SEQ_A, MATE_2B)) + spread(net[2:], (SEQ_A, MATE_2))))
    cases.append(("a fragment's two strands", 1, spread(net[:2], (SEQ_A, None)) + spread(net[1:], (strand.rc(SEQ_A), None))))
    cases.append(("a pair and the pair with its mates exchanged", 1, spread(net[:2], (SEQ_A, MATE_2)) + spread(net[1:], (MATE_2, SEQ_A))))
    dual = [(b"ACGT+TGCA", 5), (b"ACGT+TGCC", 2), (b"CCGT+TGCC", 1), (b"ACGA+TGCA", 1), (b"TTTT+TTTT", 2), (b"TTTT+TTTA", 2)]
    cases.append(("dual UMIs joined by '+'", 1, spread(dual)))
    cases.append(("dual UMIs joined by '+' at D=2", 2, spread(dual)))
    cases.append(("dual UMIs joined by '_' and '-'", 1, spread([(f.replace(b"+", b"_-"), c) for f, c in dual])))
    for lb in LBS:
        cases.append((f"Lb = {lb}", 1, spread(lb_network(lb, rng))))
        cases.append((f"Lb = {lb} at D=2", 2, spread(lb_network(lb, rng))))
    return cases


def dense_networks(seed, groups, D_choices=(1, 2)):
    """Random dense networks: 4-base UMIs over a few sequences, so that most nodes have neighbours: [(name, D, records)]."""
    rng = random.Random(seed)
    cases = []
    for g in range(groups):
        seqs = [bytes(rng.choice(b"ACGT") for _ in range(12)) for _ in range(rng.choice([1, 2, 3]))]
        n = rng.choice([1, 2, 5, 9, 30, 70, 200, 600])
        records = []
        for _ in range(n):
            u = bytes(rng.choice(b"ACGTN" if rng.random() < 0.2 else b"ACG") for _ in range(4))
            records += [(u, (rng.choice(seqs), None))] * rng.choice([1, 1, 1, 2, 3, 8])
        rng.shuffle(records)
        cases.append((f"dense {g}", rng.choice(D_choices), records))
    return cases


def seqkey(seqs, both=False):
    if not both:
        return seqs
    c = strand.canon_key(seqs[0] if seqs[1] is None else seqs)
    return (c, None) if seqs[1] is None else tuple(c)
