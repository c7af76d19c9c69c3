"""Inputs for the tests of FQD_FAST_CONSENSUS=1: the columns that are gone through by exhaustion and the named tie and clamp
columns (tests/test_consensus_core.py and the native harness), and builders of clusters, FASTQ texts and their record arrays
(tests/test_gpu_consensus.py, tests/test_fast_consensus_cli.py).  Every builder takes its random.Random, so a case is the same
in every run."""
import itertools

import numpy as np

LETTERS = b"ACGTN"
QUALS = b"!#5I~" + b" "                                        # Phred 0, 2, 20, 40, 93 and one byte below 33
LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 150, 151, 255, 256, 257]
SIZES = [1, 2, 3, 7, 8, 9, 63, 64, 65, 66, 129]                # with the small tiers: both bounds +- 1 and several workgroups
FILL = 0xEE


# ---- columns -------------------------------------------------------------------------------------------------------------------

def small_columns(members=4):
    """Every column of 1 .. members members over LETTERS x QUALS, as (bases, quals); member 0 is the written one.  The native
    harness goes through them in this order: the first member's symbol changes slowest, a symbol = letter * 6 + quality."""
    symbols = [(b, q) for b in LETTERS for q in QUALS]
    for m in range(1, members + 1):
        for combo in itertools.product(symbols, repeat=m):
            yield bytes(b for b, _ in combo), bytes(q for _, q in combo)


def named_columns():
    """(name, own base, bases, quals, (winner letter, quality byte, changed)): every kind of tie, both clamps."""
    return [
        ("two letters tie, the own one among them", b"C", b"CA", b"55", (b"C", b"!", False)),
        ("two letters tie, the own one the later", b"T", b"TA", b"II", (b"T", b"!", False)),
        ("two letters tie without the own one", b"T", b"TGC", b"!55", (b"C", b"!", True)),
        ("three letters tie without the own one", b"N", b"NTGA", b"~555", (b"A", b"!", True)),
        ("all four tie with the own one", b"G", b"GACT", b"IIII", (b"G", b"!", False)),
        ("weightless letters tie with N, own N", b"N", b"NAC", b"~!!", (b"N", b"!", False)),
        ("weightless letters tie with N, own a base", b"C", b"CNA", b"!~!", (b"C", b"!", False)),
        ("two letters tie above the own one", b"T", b"TCA", b"!##", (b"A", b"!", True)),
        ("N wins where nothing else is present", b"N", b"NNN", b"~I5", (b"N", b"!", False)),
        ("own N keeps a tie with a weightless base", b"N", b"NG", b"~ ", (b"N", b"!", False)),
        ("own N, one base with weight", b"N", b"NG", b"~#", (b"G", b"#", True)),
        ("a quality below 33 weighs nothing", b"A", b"AC", b" #", (b"C", b"#", True)),
        ("the others weigh as much as the winner: 0", b"A", b"ACG", b"I55", (b"A", b"!", False)),
        ("the others outweigh the winner: 0", b"A", b"ACG", b"I5I", (b"A", b"!", False)),
        ("exactly 93", b"A", b"AAA", b"II.", (b"A", b"~", False)),
        ("92", b"A", b"AAA", b"II-", (b"A", b"}", False)),
        ("sums cross 93", b"A", b"AAA", b"~~~", (b"A", b"~", False)),
        ("one vote of 93 against one of 92", b"C", b"CA", b"}~", (b"A", b'"', True)),
        ("a lower-case base stands for N", b"a", b"aA", b"~5", (b"A", b"5", True)),
        ("a byte above '~' weighs what it says", b"A", b"AC", b"\xff5", (b"A", b"~", False)),
    ]


# ---- clusters ------------------------------------------------------------------------------------------------------------------

def template(rng, length):
    return bytes(rng.choice(b"ACGT") for _ in range(length))


def qualities(rng, length, pool=b"!#+5:?DIIII~ "):
    return bytes(rng.choice(pool) for _ in range(length))


def noisy_cluster(rng, members, length, error_rate=0.08, n_rate=0.03, pool=b"!#+5:?DIIII~ "):
    """`members` (sequence, quality) of one length: copies of one template with substitutions and N's."""
    t = template(rng, length)
    out = []
    for _ in range(members):
        s = bytearray(t)
        for p in range(length):
            x = rng.random()
            if x < error_rate:
                s[p] = rng.choice(b"ACGT")
            elif x < error_rate + n_rate:
                s[p] = ord("N")
        out.append((bytes(s), qualities(rng, length, pool)))
    return out


def special_clusters(length):
    """(name, members) whose every column is of one kind; the written member is member 0."""
    L = length
    return [
        ("ties with the written member's letter", [(b"C" * L, b"5" * L), (b"A" * L, b"5" * L)]),
        ("ties without it", [(b"T" * L, b"!" * L), (b"G" * L, b"5" * L), (b"C" * L, b"5" * L)]),
        ("all N", [(b"N" * L, b"~" * L), (b"N" * L, b"I" * L), (b"N" * L, b"!" * L)]),
        ("all '!'", [(b"G" * L, b"!" * L), (b"A" * L, b"!" * L), (b"G" * L, b"!" * L)]),
        ("sums cross 93", [(b"A" * L, b"~" * L), (b"A" * L, b"~" * L), (b"A" * L, b"I" * L)]),
        ("the others outweigh the winner", [(b"A" * L, b"I" * L), (b"C" * L, b"5" * L), (b"G" * L, b"5" * L)]),
        ("an error copy first, two good copies behind", [(b"T" * L, b"#" * L), (b"G" * L, b"I" * L), (b"G" * L, b"I" * L)]),
    ]


# ---- a FASTQ text and its record arrays ----------------------------------------------------------------------------------------

def record_bytes(k, seq, qual, name=None):
    return b"@" + (name if name is not None else b"r%d" % k) + b"\n" + seq + b"\n+\n" + qual + b"\n"


def laid_out(rows, align=0, rng=None, names=None):
    """rows: (sequence, quality) per record, in record order.  The text — `align` FILL bytes, the records with up to 3 FILL bytes
    between them where rng is given, 32 FILL bytes of guard — and the record scan's arrays: (text bytearray, start, size,
    seq_off, seq_len)."""
    n = len(rows)
    start, size, seq_off, seq_len = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    text = bytearray([FILL]) * align
    for k, (seq, qual) in enumerate(rows):
        name = names[k] if names else None
        rec = record_bytes(k, seq, qual, name)
        start[k], size[k], seq_len[k] = len(text), len(rec), len(seq)
        seq_off[k] = len(text) + rec.index(b"\n") + 1
        text += rec
        if rng:
            text += bytearray([FILL]) * rng.randrange(4)
    text += bytearray([FILL]) * 32
    return text, start, size, seq_off, seq_len


def scattered(rng, clusters, written="first", mates=None):
    """clusters: lists of (sequence, quality), member 0 the written one.  The members dealt to record numbers in a random order;
    returns (rows by record, perm, head): each cluster a run of perm, its members by ascending record number but for the
    written one, which stands first — the lowest record (written="first") or any member (written="any", the order behind a
    best-quality pick).  mates: the same clusters' second mates, put where the first went; then the rows are (rows of
    file 1, rows of file 2)."""
    n = sum(len(c) for c in clusters)
    numbers = list(range(n))
    rng.shuffle(numbers)
    rows, rows2, runs, at = [None] * n, [None] * n, [], 0
    for i, c in enumerate(clusters):
        mine = sorted(numbers[at:at + len(c)])
        at += len(c)
        w = mine[0] if written == "first" else rng.choice(mine)
        order = [w] + [r for r in mine if r != w]
        for k, (r, member) in enumerate(zip(order, c)):
            rows[r] = member
            if mates:
                rows2[r] = mates[i][k]
        runs.append(order)
    runs.sort(key=lambda run: min(run))                        # clusters in the order of their first member, as fqd_group_owners gives them
    perm = np.array([r for run in runs for r in run], np.uint32)
    head = np.array([1 if k == 0 else 0 for run in runs for k in range(len(run))], np.uint8)
    return (rows, rows2) if mates else rows, perm, head
