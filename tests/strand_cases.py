"""The edge list of FQD_FAST_STRAND=both, shared by tests/test_strand_core.py (the core header on the CPU) and
tests/test_gpu_strand.py (fqd_canonical_reads).  Reads are bytes; every case is named."""
import random

from strand_reference import rc

LENGTHS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 150, 151, 255, 256, 257, 1000]
DECIDING = [0, 1, 7, 8, 15, 16, 31, 32, 63, 64]


def random_read(rng, L, alphabet="ACGTN"):
    return "".join(rng.choice(alphabet) for _ in range(L)).encode()


def deciding_read(rng, L, pos, flip):
    """A read of L bytes that equals its reverse complement before position pos and differs from it there, the reverse
    complement being the smaller one iff flip.  pos <= (L-1)/2."""
    assert pos <= (L - 1) // 2
    s = bytearray(random_read(rng, L))
    for i in range(pos):
        s[i] = ord(rng.choice("ACGT"))
        s[L - 1 - i] = rc(bytes([s[i]]))[0]
    if pos == L - 1 - pos:
        s[pos] = ord("T" if flip else "A")                     # the centre of an odd read: rc has A (T) there
    else:
        s[pos] = s[L - 1 - pos] = ord("G" if flip else "C")    # rc has C (G) at pos
    s = bytes(s)
    r = rc(s)
    assert s[:pos] == r[:pos] and s[pos] != r[pos] and (r < s) == flip
    return s


def single_end_cases():
    """[(name, read)]."""
    rng = random.Random(21)
    out = []
    for L in LENGTHS:
        out.append((f"random {L}", random_read(rng, L)))
        out.append((f"random {L} acgt", random_read(rng, L, "ACGT")))
    for pos in DECIDING:
        for L in sorted({2 * pos + 1, 2 * pos + 2, 150, 151, 257, 1000}):
            if pos <= (L - 1) // 2:
                for flip in (False, True):
                    out.append((f"decided at {pos} of {L} {'turned' if flip else 'kept'}", deciding_read(rng, L, pos, flip)))
    for L in LENGTHS:
        if L >= 1:
            for flip in (False, True):
                out.append((f"decided at the middle of {L} {'turned' if flip else 'kept'}", deciding_read(rng, L, (L - 1) // 2, flip)))
    for k in (1, 4, 8, 16, 38, 64, 250):
        out.append((f"palindrome {4 * k}", b"ACGT" * k))
    for w in (0, 1, 7, 8, 15, 16, 31, 32, 75, 128):
        half = random_read(rng, w, "ACGT")
        out.append((f"own reverse complement around N, {2 * w + 1}", half + b"N" + rc(half)))
    for L in (2, 17, 32, 33, 150, 257):
        s = bytearray(random_read(rng, L, "ACGT"))
        for i in (0, L // 3, (L - 1) // 2):
            s[i] = s[L - 1 - i] = ord("N")
        out.append((f"N at mirrored places, {L}", bytes(s)))
    for L in (1, 16, 33, 150, 256):
        out.append((f"all A {L}", b"A" * L))
        out.append((f"all T {L}", b"T" * L))
    return out


def paired_cases():
    """[(name, mate 1, mate 2)]."""
    rng = random.Random(22)
    out = []
    for L in (1, 15, 16, 17, 150, 300):
        a, b = sorted((random_read(rng, L), random_read(rng, L)))
        if a != b:
            out.append((f"a < b, {L}", a, b))
            out.append((f"a > b, {L}", b, a))
        out.append((f"a == b, {L}", a, a))
    for la, lb in ((0, 0), (0, 1), (1, 0), (1, 1), (0, 150), (150, 0), (1, 150), (150, 1)):
        out.append((f"lengths {la} and {lb}", random_read(rng, la), random_read(rng, lb)))
    for short, long_ in ((1, 2), (15, 16), (16, 17), (16, 150), (64, 65), (100, 150), (150, 1000)):
        s = random_read(rng, long_)
        out.append((f"mate 1 a prefix of mate 2, {short} of {long_}", s[:short], s))
        out.append((f"mate 2 a prefix of mate 1, {short} of {long_}", s, s[:short]))
    for at in (15, 16, 64, 256, 300, 511, 512):                # (from 256 on: decided in a later round of sixteen chunks)
        for la, lb in ((at + 1, at + 1), (150, 150), (at + 1, 150), (150, at + 1), (151, 97 if at < 97 else 151), (600, 600), (600, 1000)):
            if min(la, lb) <= at:
                continue
            a = bytearray(random_read(rng, la))
            b = bytearray(random_read(rng, lb))
            b[:at] = a[:at]
            a[at], b[at] = ord("C"), ord("G")
            out.append((f"first difference at {at}, lengths {la} and {lb}, kept", bytes(a), bytes(b)))
            out.append((f"first difference at {at}, lengths {la} and {lb}, turned", bytes(b), bytes(a)))
    for la, lb in ((10, 200), (200, 10), (149, 151), (151, 149), (33, 1000)):
        out.append((f"random, lengths {la} and {lb}", random_read(rng, la), random_read(rng, lb)))
    return out
