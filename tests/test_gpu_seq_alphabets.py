"""fqd_sort_seqs / fqd_seq_heads (csrc/fqd_seq.hip) at every code width and with the mate boundary inside a key word.

run_sort codes the K byte values present in w = max(1, bits_for(K)) bits and packs P = 64 / w positions into a key word;
the other sequence tests only reach w = 3 (ACGT, ACGTNa) and w = 5 (16 letters).  Here the alphabets are drawn from the
bytes 11..255 with K at both ends of every width 1..8; lengths run to 3P + 2 with records planted at every word edge; two
fifths of the records are prefixes of a pool of strings that share roots, so that duplicates, prefix chains and runs that
stay mixed over several levels are the rule; in pairs the longest mate 1 is forced to 0, 1, P-1, P, P+1 and 2P+3 (mate 2
then starts at the first, the last and a middle position of a key word); record counts lie around the 4096-element tile
of the radix passes and the flag scans.  Yardstick: tests/seq_reference.py (stable sorted order, heads of every mode over
the records in the order the device returned).

An input of fewer than 16 records has no room for 128 byte values (2 mates x 26 bytes a record at w = 8): the record-count
cases n = 1, 2 at K = 128 take the width of what fits, all the others assert that every one of the K values occurs."""
import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine
import seq_reference as ref
from test_gpu_seq import MODE, dev, host_u32, spans

pytestmark = pytest.mark.gpu

WIDTH_K = [1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 245]       # both ends of every width 1..8
COUNTS = [1, 2, 63, 64, 65, 4095, 4096, 4097, 9000]
HEAD_MODES = [(ref.TIGHT, 0), (ref.LOOSE, 0), (ref.HAMMING, 0), (ref.HAMMING, 1)]
N_POOL = 50


@pytest.fixture(scope="module")
def engine():
    with Engine(segments=2) as e:
        yield e


def bits_for(v):
    return int(v).bit_length()


def width(K):
    """(w, P) as run_sort takes them from the census."""
    w = max(1, bits_for(K))
    return w, 64 // w


def alphabet(rng, K):
    """K byte values of 11..255, ascending: always 0x0B (the lowest the census accepts), from K = 2 on also 0xFF."""
    fixed = [11] if K == 1 else [11, 255]
    rest = rng.choice(np.arange(12, 255), size=K - len(fixed), replace=False).tolist() if K > len(fixed) else []
    return np.array(sorted(fixed + rest), dtype=np.uint8)


def random_seq(rng, alpha, length):
    return rng.choice(alpha, size=int(length)).astype(np.uint8).tobytes()


def make_pool(rng, alpha, P, cap, cover):
    """About 50 strings of `cap` bytes.  With `cover` the first ones walk the alphabet, so that all K values occur; the
    others share a root up to a word edge (or anywhere) and go on at random: records that agree on whole key words and
    differ in a later one, in every combination."""
    pool = []
    if cover:
        for at in range(0, len(alpha), max(cap, 1)):
            chunk = alpha[at:at + cap].tobytes()
            pool.append(chunk + random_seq(rng, alpha, cap - len(chunk)))
    roots = [random_seq(rng, alpha, cap) for _ in range(4)]
    edges = [e for e in (P, P + 1, 2 * P, 2 * P + 1) if e <= cap]
    while len(pool) < N_POOL:
        root = roots[int(rng.integers(0, len(roots)))]
        cut = edges[int(rng.integers(0, len(edges)))] if edges and rng.random() < 0.7 else int(rng.integers(0, cap + 1))
        pool.append(root[:cut] + random_seq(rng, alpha, cap - cut))
    return pool


def make_mate(rng, alpha, P, n, cap=None, cover=True):
    """n sequences of at most cap (default 3P + 2) bytes, the longest exactly cap.  In this order, cut to n: the covering
    strings whole, one record of each planted length (prefixes of one string: a chain across the word edges), then 40 %
    prefixes of pool strings (a quarter of them whole) and 60 % random strings of uniform length."""
    cap = 3 * P + 2 if cap is None else cap
    if cap == 0:
        return [b""] * n
    pool = make_pool(rng, alpha, P, cap, cover)
    n_cover = -(-len(alpha) // cap) if cover else 1
    out = pool[:n_cover]
    out += [pool[-1][:L] for L in (0, 1, P - 1, P, P + 1, 2 * P, 2 * P + 1, 3 * P) if L <= cap]
    while len(out) < n:
        if rng.random() < 0.4:
            s = pool[int(rng.integers(0, len(pool)))]
            out.append(s if rng.random() < 0.25 else s[:int(rng.integers(0, cap + 1))])
        else:
            out.append(random_seq(rng, alpha, rng.integers(0, cap + 1)))
    return out[:n]


def boundary_pairs(alpha, m1):
    """Pairs that differ only in mate 2, at its first position = the first position after mate 1's end when mate 1 is the
    longest one: empty, lowest and highest byte, alone and before a common tail.  Given in descending order."""
    lo, hi = alpha[:1].tobytes(), alpha[-1:].tobytes()
    tail = lo * 3
    return [(m1, hi + tail), (m1, lo + tail), (m1, hi), (m1, lo), (m1, b"")]


def make_input(seed, K, n, paired, longest1=None, mate2_empty=False):
    """(records, w, P).  Records are tuples of 1 or 2 mates in a random order; every planted record is there when n >= 16."""
    rng = np.random.default_rng(seed)
    alpha = alphabet(rng, K)
    w, P = width(K)
    if not paired:
        mates = [(s,) for s in make_mate(rng, alpha, P, n)]
    elif mate2_empty:
        mates = [(s, b"") for s in make_mate(rng, alpha, P, n)]
    else:
        m1 = make_mate(rng, alpha, P, n, cap=longest1, cover=False)
        m2 = make_mate(rng, alpha, P, n, cover=True)
        mates = list(zip(m1, m2))
        if n >= 16:
            # behind the covering strings of mate 2 (the last slots are random fill)
            mates[n - 5:] = boundary_pairs(alpha, max(m1, key=len))
    order = rng.permutation(len(mates))
    mates = [mates[i] for i in order]
    present = set(b"".join(b"".join(m) for m in mates))
    assert present <= set(alpha.tolist())
    if n >= 16:
        assert len(present) == K, f"only {len(present)} of {K} byte values occur: the width reached is not the width named"
        assert max(len(m[0]) for m in mates) == (longest1 if paired and not mate2_empty and longest1 is not None else 3 * P + 2)
        if paired:
            assert max(len(m[1]) for m in mates) == (0 if mate2_empty else 3 * P + 2)
    return mates, w, P


def check_order_and_heads(e, mates):
    n = len(mates)
    ds = [tuple(dev(x) for x in spans([m[k] for m in mates])) for k in range(len(mates[0]))]
    t = [(d, o, l, n) for d, o, l in ds]
    t2 = t[1] if len(t) > 1 else None
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    e.sort_seqs(t[0], perm, t2)
    p = host_u32(perm, n)
    exp = np.array(ref.sorted_order(mates), dtype=np.uint32)
    wrong = np.nonzero(p != exp)[0]
    assert wrong.size == 0, (f"{wrong.size} of {n} places differ, the first at {wrong[0]}: got record {p[wrong[0]]} "
                             f"{mates[p[wrong[0]]]!r}, expected {exp[wrong[0]]} {mates[exp[wrong[0]]]!r}")
    in_order = [mates[i] for i in p]
    for mode, d in HEAD_MODES:
        head = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        got = e.seq_heads(t[0], perm, MODE[mode], d, head, t2)
        want = np.array(ref.heads(mode, d, in_order), dtype=np.uint8)
        assert np.array_equal(head.cpu().numpy(), want), (mode, d)
        assert got == int(want.sum()), (mode, d)
    return p


@pytest.mark.parametrize("K", WIDTH_K)
def test_single_end_at_every_width(engine, K):
    n = 5000
    mates, w, P = make_input(1000 + K, K, n, paired=False)
    assert (w, P) == {1: (1, 64), 2: (2, 32), 3: (2, 32), 4: (3, 21), 7: (3, 21), 8: (4, 16), 15: (4, 16), 16: (5, 12), 31: (5, 12),
                      32: (6, 10), 63: (6, 10), 64: (7, 9), 127: (7, 9), 128: (8, 8), 245: (8, 8)}[K]
    lens = {len(m[0]) for m in mates}
    assert {0, 1, P - 1, P, P + 1, 2 * P, 2 * P + 1, 3 * P, 3 * P + 2} <= lens and max(lens) <= 194
    p = check_order_and_heads(engine, mates)
    if K == 1:                                               # by length alone, equal lengths in input order
        assert p.tolist() == sorted(range(n), key=lambda i: len(mates[i][0]))


# the longest mate 1 ("0": every mate 1 is empty); "no2": every mate 2 is empty and mate 1 has the full length
@pytest.mark.parametrize("longest1", ["0", "1", "P-1", "P", "P+1", "2P+3", "no2"])
@pytest.mark.parametrize("K", WIDTH_K)
def test_paired_with_the_mate_boundary_inside_a_word(engine, K, longest1):
    n = 5000
    w, P = width(K)
    if longest1 == "no2":
        mates, _, _ = make_input(2000 + K, K, n, paired=True, mate2_empty=True)
    else:
        m1 = {"0": 0, "1": 1, "P-1": P - 1, "P": P, "P+1": P + 1, "2P+3": 2 * P + 3}[longest1]
        mates, _, _ = make_input(3000 + 16 * K + len(longest1) + m1, K, n, paired=True, longest1=m1)
        firsts = {}                                          # of one longest mate 1: the first bytes of its mates 2
        for a, b in mates:
            if len(a) == m1:
                firsts.setdefault(a, set()).add(b[:1])
        assert max(map(len, firsts.values())) >= (3 if K > 1 else 2)   # pairs that differ only at mate 2's first position
    p = check_order_and_heads(engine, mates)
    if longest1 == "0":                                      # mate 2's order alone
        assert p.tolist() == ref.sorted_order([(m[1],) for m in mates])


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("K", [4, 128])
def test_record_counts_around_the_tile(engine, K, n, paired):
    mates, _, _ = make_input(5000 + 3 * n + K + int(paired), K, n, paired=paired)
    assert len(mates) == n
    check_order_and_heads(engine, mates)


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_every_read_empty(engine, paired):
    # K == 0: no key word at all, a sort of zero bits
    n = 5000
    mates = [(b"", b"") if paired else (b"",)] * n
    ds = [tuple(dev(x) for x in spans([m[k] for m in mates])) for k in range(len(mates[0]))]
    t = [(d, o, l, n) for d, o, l in ds]
    t2 = t[1] if paired else None
    perm = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    engine.sort_seqs(t[0], perm, t2)
    assert np.array_equal(host_u32(perm, n), np.arange(n, dtype=np.uint32))
    for mode, d in HEAD_MODES:
        head = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        assert engine.seq_heads(t[0], perm, MODE[mode], d, head, t2) == 1
        h = head.cpu().numpy()
        assert h[0] == 1 and not h[1:].any()
    check_order_and_heads(engine, mates)


@pytest.mark.parametrize("full", [False, True], ids=["K3", "K245"])
def test_bytes_from_0x80_sort_as_unsigned(engine, full):
    """Twins that differ in one byte, 0x7F in one and 0x80 in the other, at position 0, P - 1 and P: the 0x80 twin sorts
    after (strncmp compares unsigned chars).  Once with three byte values (w = 2) and once with all of 11..255 present
    (w = 8, the rank of 0x80 is 118 and that of 0xFF 245: a rank cut to 7 bits or compared signed reverses them)."""
    K = 245 if full else 3
    w, P = width(K)
    base = b"A" * (2 * P)
    mates, twins = [], []
    for pos in (0, P - 1, P):
        hi, lo = bytearray(base), bytearray(base)
        hi[pos], lo[pos] = 0x80, 0x7F
        twins.append((len(mates), len(mates) + 1))
        mates += [(bytes(hi),), (bytes(lo),)]                # the 0x80 twin first: the input order is the wrong one
    if full:
        mates.append((bytes(range(11, 256)),))
        mates += [(b"\xff" + base,), (b"\xfe" + base,), (base[:P - 1] + b"\xff",), (base[:P - 1] + b"\x81",)]
    assert len(set(b"".join(m[0] for m in mates))) == K
    p = check_order_and_heads(engine, mates)
    place = {int(r): k for k, r in enumerate(p)}
    for hi, lo in twins:
        assert place[lo] < place[hi]
