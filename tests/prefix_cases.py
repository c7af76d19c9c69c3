"""Inputs for the tests of FQD_FAST_PREFIX=L: builders of reads whose lengths and differences fall where the seed join and the
overlap compare can go wrong (tests/test_gpu_prefix.py, tests/test_prefix_core.py, tests/test_fast_prefix_cli.py).  A record is a
tuple of mates (1 or 2 byte strings); every builder takes its random.Random, so a case is the same in every run.  Every case
stands on templates of its own, so that nothing but what its name says is related."""
from near_cases import LETTERS, scattered, substituted, template      # noqa: F401  (scattered and template are the tests' too)

SHORT_LENGTHS = [15, 16, 17, 127, 128, 129, 143, 144, 145]     # and L, L + 1: short_lengths(L)
EXTRA = [1, 16, 129]                                           # the long node's bytes behind the overlap
GROUP_SIZES = [7, 8, 9, 63, 64, 65, 4095, 4096]
DIGITS = 7                                                     # base-4 digits of a node's number: 4^7 > 4097


def short_lengths(L):
    return sorted({k for k in SHORT_LENGTHS + [L, L + 1] if k >= L})


def other(rng, seq, at):
    return substituted(seq, [at], rng)


def truncations(rng, L, short, extra):
    """(name, nodes of mate-1 strings, related pairs among them): a read of `short` bytes and its long copy of short + extra,
    with a difference where it matters."""
    cases = []
    t = template(rng, short + extra)
    cases.append(("a prefix", [t[:short], t], 1))
    t = template(rng, short + extra)
    cases.append(("a difference at the overlap's last byte", [other(rng, t[:short], short - 1), t], 0))
    if short > L:
        t = template(rng, short + extra)
        cases.append(("a difference at byte L", [other(rng, t[:short], L), t], 0))           # same group, not related
    for at in sorted({0, L - 1}):
        t = template(rng, short + extra)
        cases.append((f"a difference at byte {at}, inside the first L", [other(rng, t[:short], at), t], 0))      # another group
    t = template(rng, short + extra)
    cases.append(("a difference in the first byte behind the overlap", [t[:short], t, other(rng, t, short)], 2))  # still related, to both
    return cases


def as_records(rng, L, cases, paired, cut_mate=0):
    """The cases' nodes as records.  Pairs: the case plays in mate `cut_mate`, the other mate is one read of the case's own
    (of L bytes or more), the same in all its nodes — "one mate equal, the other longer"."""
    out = []
    for _, nodes, _ in cases:
        if not paired:
            out += [(m,) for m in nodes]
            continue
        mate = template(rng, L + rng.randrange(40))
        out += [(m, mate) if cut_mate == 0 else (mate, m) for m in nodes]
    return out


def pair_directions(rng, L):
    """(records, merged clusters): same-sided, opposite-sided and one-mate-equal pairs, each in both input orders."""
    records, clusters = [], 0
    for turn in (False, True):
        def put(*nodes):
            records.extend(nodes[::-1] if turn else nodes)
        a, b = template(rng, L + 40), template(rng, L + 30)
        put((a[:L + 5], b[:L + 7]), (a, b)); clusters += 1                      # same-sided: related
        a, b = template(rng, L + 40), template(rng, L + 30)
        put((a[:L + 5], b), (a, b[:L + 7])); clusters += 2                      # opposite-sided: not related
        a, b = template(rng, L + 40), template(rng, L + 30)
        put((a, b[:L + 1]), (a, b)); clusters += 1                              # mate 1 equal, mate 2 longer
        a, b = template(rng, L + 40), template(rng, L + 30)
        put((a[:L], b), (a, b)); clusters += 1                                  # mate 2 equal, mate 1 longer
        a, b = template(rng, L + 40), template(rng, L + 30)
        put((a[:L + 5], b[:L + 7]), (a, other(rng, b, L + 6))); clusters += 2   # same-sided, mate 2 differs in its overlap
        a, b = template(rng, L + 40), template(rng, L + 30)
        put((a[:L + 5], b[:L + 7]), (other(rng, a, L + 4), b)); clusters += 2   # ... mate 1 does
    return records, clusters


def eligibility(rng, L, paired):
    """(records, merged clusters): a mate of exactly L bytes takes part, one of L - 1 does not — as a child or as a parent."""
    t, u = template(rng, L + 20), template(rng, L + 20)
    if not paired:
        return [(t[:L],), (t,), (u[:L - 1],), (u,)], 3
    records, clusters = [], 0
    for m in (0, 1):
        def rec(x, y):
            return (x, y) if m == 0 else (y, x)
        t, u, v, w = (template(rng, L + 20) for _ in range(4))
        records += [rec(t[:L], u), rec(t, u)]; clusters += 1                    # len == L in mate m: eligible
        records += [rec(v[:L - 1], w), rec(v, w)]; clusters += 2                # len == L - 1 in mate m: not
        x, y = template(rng, L + 20), template(rng, L + 20)
        records += [rec(x[:L + 3], y[:L - 1]), rec(x, y[:L - 1])]; clusters += 2     # the other mate below L in both: neither takes part
    return records, clusters


def star(rng, L, longs=5):
    """One short read under several long ones of spans L + 30, L + 20, L + 20, L + 25, ..: it goes to the first of the two
    shortest.  Returns (records, the place of the short read, the place of its parent)."""
    t = template(rng, L + 10)
    tails = [30, 20, 20, 25, 40][:longs]
    records = [(t + template(rng, k),) for k in tails] + [(t,)]
    return records, len(records) - 1, 1


def two_maximal(rng, L):
    """A ⊑ B and A ⊑ C with B and C different reads of one length: two clusters, A with the one that comes first."""
    a = template(rng, L)
    return [(a + template(rng, 118),), (a,), (a + template(rng, 118),)]


def chain(rng, L, depth, paired=False):
    """depth + 1 nodes, each the next one's prefix by one byte: a parent chain of `depth` links.  Shuffled by the caller."""
    t, u = template(rng, L + depth), template(rng, L + 3)
    return [(t[:L + k], u) if paired else (t[:L + k],) for k in range(depth + 1)]


def group_records(rng, L, size, paired=False):
    """`size` nodes that agree on their first L bytes and of which no one is a prefix of another — every node's number stands
    behind the L bytes in base 4, then 0 .. 2 more letters, so that lengths differ and pairs are compared — but for the last,
    which is node 0 with two letters more: one related pair.  In a shuffled order."""
    head = template(rng, L)
    def tail(k):
        return bytes(LETTERS[(k >> (2 * d)) & 3] for d in range(DIGITS)) + b"A" * (k % 3)
    nodes = [head + tail(k) for k in range(size - 1)] + [head + tail(0) + b"GT"]
    mate2 = template(rng, L + 2)
    records = [(m, mate2) if paired else (m,) for m in nodes]
    rng.shuffle(records)
    return records


def random_records(rng, L, nodes=3000, templates=300, paired=False, length=150):
    """Nodes cut from `templates` templates, a third of them with a substitution somewhere, copies scattered among them.
    Single-end: at random lengths from L - 2 on; pairs: each mate at one of nine lengths (the statement looks every node up
    at every shape that occurs)."""
    cuts = sorted({max(k, 0) for k in (L - 2, L - 1, L, L + 1, L + 7, 60, 100, length - 1, length)})
    made = [(template(rng, length), template(rng, length)) for _ in range(templates)]
    out = []
    for _ in range(nodes):
        t1, t2 = rng.choice(made)
        mates = []
        for t in (t1, t2):
            m = t[:rng.choice(cuts) if paired else rng.randrange(max(L - 2, 0), length + 1)]
            if m and rng.random() < 0.33:
                m = other(rng, m, rng.randrange(len(m)))
            mates.append(m)
        out.append(tuple(mates) if paired else (mates[0],))
    return scattered(rng, out, copies=(0, 0, 1, 2))
