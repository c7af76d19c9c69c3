"""Seeded random inputs on which the oracle is pinned to the reference's own object code.

tests/golden/make_golden.py records the reference's answers on these inputs in
tests/golden/ref_fuzz.json; tests/test_oracle.py replays them against the oracle.
"""
import random

from oracle.binding import FASTA, FASTQ


def pack_cases():
    """Sequences for seq2hash: mostly ACGTN at the lengths around a 17-mer word, some with unknown bytes."""
    rnd = random.Random(7)
    out = []
    for _ in range(3000):
        n = rnd.choice((0, 1, 16, 17, 18, 34, 75, 150, 151, rnd.randrange(0, 400)))
        alphabet = b"ACGTN" if rnd.random() < 0.9 else b"ACGTNacgtnRY-\r"
        out.append(bytes(rnd.choice(alphabet) for _ in range(n)))
    return out


def parse_cases():
    """(format, block) pairs for the record walkers: whole blocks and blocks cut anywhere."""
    rnd = random.Random(11)
    out = []
    for _ in range(300):
        fmt = rnd.choice((FASTQ, FASTA))
        lead = b"@" if fmt == FASTQ else b">"
        buf = b""
        for i in range(rnd.randrange(1, 12)):
            L = rnd.randrange(0, 40)
            seq = bytes(rnd.choice(b"ACGTN") for _ in range(L))
            rec = lead + b"id%d" % i + (b" c" if rnd.random() < 0.5 else b"") + b"\n" + seq + b"\n"
            if fmt == FASTQ:
                rec += b"+\n" + b"I" * L + b"\n"
            buf += rec
        cut = rnd.randrange(0, len(buf) + 1) if rnd.random() < 0.5 else len(buf)
        out.append((fmt, buf[:cut]))
    return out


def tag_order_cases():
    """Pairs of one-base FASTQ records whose ID lines the reference orders."""
    rnd = random.Random(13)
    pool = [b"SRR%d.%d c" % (rnd.randrange(3), rnd.randrange(200)) for _ in range(40)]
    pool += [b"M:%d:%d %d:N" % (rnd.randrange(3), rnd.randrange(50), rnd.randrange(1, 3)) for _ in range(40)]
    pool += [b"q%d" % rnd.randrange(30) for _ in range(20)]
    out = []
    for _ in range(2000):
        a, b = rnd.choice(pool), rnd.choice(pool)
        out.append((b"@" + a + b"\nA\n+\nI\n", b"@" + b + b"\nA\n+\nI\n"))
    return out
