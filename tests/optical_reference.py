"""The rule of FQD_FAST_OPTICAL=D (fastq-dupaway_amd/csrc/fqd_optical_core.hpp) stated sequentially in plain Python, exact:
the place of a record off its ID line, the optical groups of a cluster by union-find over its pairs, and the fields of
fqd_places_info / fqd_optical_info.  The yardstick of tests/test_optical_core.py, tests/test_gpu_optical.py and
tests/test_fast_optical_cli.py; tests/test_optical_core.py checks it by hand."""
import numpy as np

NO_RECORD = 0xFFFFFFFFFFFFFFFF
OK, FEW_FIELDS, EMPTY_FIELD, NOT_DIGIT, TOO_LONG, BAD_END = range(6)
SAME_SURFACE = 0x80000000
MAX_CLUSTER = 65536
ALL_PAIRS_UP_TO = 4096                                         # larger clusters: pairs by a sorted window (pairs())
DIGITS = b"0123456789"


def first_word(line: bytes) -> bytes:
    """What stands behind the line's first byte up to the first blank, tab, '\\r' or '\\n'."""
    end = len(line)
    for i in range(1, len(line)):
        if line[i] in b" \t\r\n":
            end = i
            break
    return line[1:end]


def parse(line: bytes):
    """(reason, tile, x, y, surface bytes) of one ID line; the values are None where the record is refused."""
    fields = first_word(line).split(b":")
    if len(fields) < 7:
        return FEW_FIELDS, None, None, None, None
    if any(len(f) == 0 for f in fields[:7]):
        return EMPTY_FIELD, None, None, None, None
    values = []
    for f in fields[4:6]:
        if any(b not in DIGITS for b in f):
            return NOT_DIGIT, None, None, None, None
        if len(f) > 9:
            return TOO_LONG, None, None, None, None
        values.append(int(f))
    y = fields[6]
    nd = 0
    while nd < len(y) and y[nd] in DIGITS:
        nd += 1
    if nd == 0:
        return NOT_DIGIT, None, None, None, None
    if nd > 9:
        return TOO_LONG, None, None, None, None
    if nd < len(y) and y[nd] not in b":_#/":
        return BAD_END, None, None, None, None
    return OK, values[0], values[1], int(y[:nd]), b":".join(fields[:4])


def read_places(lines):
    """fqd_read_places over ID lines: (tile, x, y, surface words, surfaces as bytes, info).  Entries of refused records are 0 /
    None: the library promises nothing about them."""
    n = len(lines)
    tile, x, y, word = (np.zeros(n, np.uint32) for _ in range(4))
    surfaces = [None] * n
    bad_record, bad_reason, other = NO_RECORD, OK, 0
    for i, line in enumerate(lines):
        reason, t, xx, yy, surface = parse(line)
        if reason:
            if bad_record == NO_RECORD:
                bad_record, bad_reason = i, reason
            continue
        c4 = 1 + len(surface)                                  # the fourth colon's position
        same = lines[0][1:c4 + 1] == line[1:c4 + 1]
        tile[i], x[i], y[i], word[i], surfaces[i] = t, xx, yy, len(surface) | (SAME_SURFACE if same else 0), surface
        other += not same
    return tile, x, y, word, surfaces, dict(bad_record=bad_record, bad_reason=bad_reason, other_surface=other)


def neighbours(a, b, D):
    """a, b = (surface bytes, tile, x, y)."""
    return a[0] == b[0] and a[1] == b[1] and abs(a[2] - b[2]) <= D and abs(a[3] - b[3]) <= D


def pairs(places, D):
    """The neighbour pairs (u, v), u < v, of one cluster's members.  Up to ALL_PAIRS_UP_TO members every pair is looked at; a
    larger cluster is sorted by (surface, tile, x) and a member is held against those behind it on its surface and tile
    whose x is at most D larger — every other pair fails the rule on surface, tile or x."""
    s = len(places)
    if s <= ALL_PAIRS_UP_TO:
        ids = {}
        S = np.array([ids.setdefault(p[0], len(ids)) for p in places], np.int64)
        T, X, Y = (np.array([p[k] for p in places], np.int64) for k in (1, 2, 3))
        A = (S[:, None] == S[None, :]) & (T[:, None] == T[None, :]) & (np.abs(X[:, None] - X[None, :]) <= D) & (np.abs(Y[:, None] - Y[None, :]) <= D)
        u, v = np.nonzero(np.triu(A, 1))
        return u, v
    order = sorted(range(s), key=lambda i: places[i][:3])
    us, vs = [], []
    for a, i in enumerate(order):
        for j in order[a + 1:]:
            if places[j][0] != places[i][0] or places[j][1] != places[i][1] or places[j][2] - places[i][2] > D:
                break
            if abs(places[j][3] - places[i][3]) <= D:
                us.append(min(i, j))
                vs.append(max(i, j))
    return np.array(us, np.int64), np.array(vs, np.int64)


def groups(s, u, v):
    """Union-find over the pairs: per member the lowest place of its connected component."""
    parent = list(range(s))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in zip(u.tolist(), v.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)                  # (the lower place stays the root)
    return np.array([find(a) for a in range(s)], np.int64)


def sweeps(s, u, v):
    """How many sweeps the parallel form takes (the header's min step and pointer jump, every member at once)."""
    L = np.arange(s, dtype=np.int64)
    a, b = np.concatenate([u, v]), np.concatenate([v, u])
    count = 0
    while True:
        low = L.copy()
        np.minimum.at(low, a, L[b])
        if np.array_equal(low, L):
            return count, L
        L = low[low]
        count += 1


def split(owner, places, D, max_cluster=MAX_CLUSTER):
    """fqd_optical_split: owner = the current owners (the first record of every record's cluster), places[i] = (surface
    bytes, tile, x, y).  Returns (owner_out or None where a cluster is refused, the info fields)."""
    n = len(owner)
    clusters = {}
    for i, o in enumerate(owner):
        clusters.setdefault(int(o), []).append(i)              # (members in input order)
    info = dict(clusters_in=len(clusters), clusters_out=0, split=0, largest=max((len(m) for m in clusters.values()), default=0), sweeps=0,
                max_cluster=max_cluster, over_limit_members=0, over_limit_first=NO_RECORD)
    over = [o for o, m in clusters.items() if len(m) > max_cluster]
    if over:
        info.update(over_limit_first=min(over), over_limit_members=len(clusters[min(over)]))
        return None, info
    out = np.zeros(n, np.uint32)
    for members in clusters.values():
        s = len(members)
        if s == 1:
            out[members[0]] = members[0]
            info["clusters_out"] += 1
            continue
        u, v = pairs([places[i] for i in members], D)
        lowest = groups(s, u, v)
        taken, fixed = sweeps(s, u, v)
        assert np.array_equal(fixed, lowest)                   # the header's (c): the sweeps end at the groups
        out[members] = np.array(members)[lowest]
        k = int(np.sum(lowest == np.arange(s)))
        info["clusters_out"] += k
        info["split"] += k > 1
        info["sweeps"] = max(info["sweeps"], taken)
    return out, info


def clusters_of(owner):
    """The clusters of an owner array as lists of records, in the order of their first records."""
    found = {}
    for i, o in enumerate(owner):
        found.setdefault(int(o), []).append(i)
    return [found[o] for o in sorted(found)]
