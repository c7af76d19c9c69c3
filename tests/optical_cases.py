"""The edge list of FQD_FAST_OPTICAL=D that tests/test_optical_core.py, tests/test_gpu_optical.py and
tests/test_fast_optical_cli.py share.  A cluster case is (name, D, members) with members = [(surface, tile, x, y), ...] in
input order: ONE cluster of identical reads.  A parse case is (name, ID line, expected reason)."""
import random

import optical_reference as ref

SURFACE = b"M01:7:FC1:1"
BIG = 2147483647


def id_line(surface, tile, x, y, behind=b"", comment=b" 1:N:0:ACGT"):
    return b"@%s:%s:%s:%s%s%s\n" % (surface, str(tile).encode(), str(x).encode(), str(y).encode(), behind, comment)


def chain(s, D=10, reverse=True, surface=SURFACE, tile=1101):
    """s members, each a neighbour of the next only (x steps of D, the next but one is 2 D away); reverse: the first member
    in input order comes last in x, so every label has the whole chain to travel."""
    xs = [1000 + D * i for i in range(s)]
    if reverse:
        xs.reverse()
    return [(surface, tile, x, 500) for x in xs]


def grid(w, h, step, surface=SURFACE, tile=7):
    return [(surface, tile, 100 + step * i, 100 + step * j) for j in range(h) for i in range(w)]


def shuffled(members, seed):
    members = list(members)
    random.Random(seed).shuffle(members)
    return members


def cluster_cases():
    S, other_lane, longer = SURFACE, b"M01:7:FC1:2", b"M01:7:FC1:10"
    cases = [
        ("one member", 5, [(S, 1, 10, 10)]),
        ("two neighbours", 5, [(S, 1, 10, 10), (S, 1, 12, 8)]),
        ("two apart", 5, [(S, 1, 10, 10), (S, 1, 100, 10)]),
        ("dx = D", 5, [(S, 1, 10, 10), (S, 1, 15, 10)]),
        ("dx = D + 1", 5, [(S, 1, 10, 10), (S, 1, 16, 10)]),
        ("dy = D", 5, [(S, 1, 10, 10), (S, 1, 10, 5)]),
        ("dy = D + 1", 5, [(S, 1, 10, 10), (S, 1, 10, 4)]),
        ("dx = D and dy = D", 5, [(S, 1, 10, 10), (S, 1, 5, 15)]),
        ("the corners with the largest D", BIG, [(S, 1, 0, 0), (S, 1, 999999999, 999999999), (S, 1, 0, 999999999), (S, 1, 999999999, 0)]),
        ("the corners with D one short", 999999998, [(S, 1, 0, 0), (S, 1, 999999999, 999999999), (S, 1, 0, 999999999), (S, 1, 999999999, 0)]),
        ("the corners with D just enough", 999999999, [(S, 1, 0, 0), (S, 1, 999999999, 999999999)]),
        ("equal coordinates on different tiles", 50, [(S, 1101, 10, 10), (S, 1102, 10, 10), (S, 1101, 10, 10), (S, 2101, 10, 10)]),
        ("surfaces that differ in the lane only", 50, [(S, 1, 10, 10), (other_lane, 1, 10, 10), (other_lane, 1, 11, 10), (S, 1, 11, 11)]),
        ("surfaces of different lengths", 50, [(S, 1, 10, 10), (longer, 1, 10, 10), (other_lane, 1, 10, 10), (longer, 1, 12, 10), (other_lane, 1, 10, 13)]),
        ("none on record 0's surface", 50, [(other_lane, 1, 10, 10), (longer, 1, 10, 10), (other_lane, 1, 10, 12), (b"M02:7:FC1:2", 1, 10, 12)]),
        ("all identical places, 7", 1, [(S, 3, 77, 88)] * 7),
        ("no neighbours at all, 8", 3, [(S, 3, 100 * i, 5) for i in range(8)]),
        ("a bridge that arrives last", 10, [(S, 1, 100, 100), (S, 1, 120, 100), (S, 1, 300, 100), (S, 1, 110, 100)]),
        ("transitive through y", 10, [(S, 1, 100, 100), (S, 1, 100, 120), (S, 1, 100, 110)]),
    ]
    for s in (2, 3, 8, 9, 40, 64, 65, 300):
        cases.append((f"chain of {s}, reversed", 10, chain(s)))
        cases.append((f"chain of {s}", 10, chain(s, reverse=False)))
        cases.append((f"chain of {s}, shuffled", 10, shuffled(chain(s), s)))
    cases.append(("grid 3 x 3, joined", 4, grid(3, 3, 4)))
    cases.append(("grid 3 x 3, apart", 3, grid(3, 3, 4)))
    cases.append(("grid 8 x 8, joined, shuffled", 4, shuffled(grid(8, 8, 4), 5)))
    cases.append(("grid 9 x 9, rows joined", 4, [(s, t, x, 10 * y) for s, t, x, y in shuffled(grid(9, 9, 4), 6)]))
    cases.append(("all identical places, 64", 1, [(S, 3, 77, 88)] * 64))
    cases.append(("all identical places, 100", 1, [(S, 3, 77, 88)] * 100))
    cases.append(("no neighbours at all, 100", 3, [(S, 3, 100 * i, 5) for i in range(100)]))
    return cases


def random_clusters(seed, count, sizes=(1, 2, 3, 5, 8, 9, 20, 64, 65, 130)):
    """Clusters of points thrown on two tiles of two surfaces, a span and a D that leave a few groups each."""
    rng = random.Random(seed)
    cases = []
    for k in range(count):
        s = rng.choice(sizes)
        span = rng.choice([30, 200, 2000])
        D = rng.choice([1, 5, 40, 300])
        members = [(rng.choice([SURFACE, SURFACE, SURFACE, b"M01:7:FC1:2"]), rng.choice([1101, 1101, 1102]), rng.randrange(span), rng.randrange(span))
                   for _ in range(s)]
        cases.append((f"random {k}: {s} members, span {span}", D, members))
    return cases


def parse_cases():
    """(name, ID line, reason)."""
    ok, few, empty, digit, long_, end = ref.OK, ref.FEW_FIELDS, ref.EMPTY_FIELD, ref.NOT_DIGIT, ref.TOO_LONG, ref.BAD_END
    filler = b"x" * 300
    return [
        ("Casava 1.8", b"@M01:7:FC1:1:1101:15589:1332 1:N:0:ACGT\n", ok),
        ("FASTA, no comment", b">M01:7:FC1:1:1101:15589:1332\n", ok),
        ("no line end", b"@M01:7:FC1:1:1101:15589:1332", ok),
        ("a tab ends the word", b"@M01:7:FC1:1:1101:15589:1332\tz:z:z\n", ok),
        ("'\\r' ends the word", b"@M01:7:FC1:1:1101:15589:1332\r\n", ok),
        ("UMI as 8th field", b"@M01:7:FC1:1:1101:15589:1332:ACGTAC 1:N:0\n", ok),
        ("fields behind the 8th", b"@M01:7:FC1:1:1101:15589:1332:ACGT:::x:: 1\n", ok),
        ("umi_tools extract", b"@M01:7:FC1:1:1101:15589:1332_ACGTAC 1:N:0\n", ok),
        ("'#0/1' behind y", b"@M01:7:FC1:1:1101:15589:1332#0/1\n", ok),
        ("'/1' behind y", b"@M01:7:FC1:1:1101:15589:1332/1\n", ok),
        ("leading zeros", b"@M01:7:FC1:1:0001:000000000:000000007 c\n", ok),
        ("nine digits each", b"@M01:7:FC1:1:999999999:999999999:999999999 c\n", ok),
        ("single bytes", b"@a:b:c:d:1:2:3\n", ok),
        ("colons in the comment do not count", b"@M01:7:FC1:1:1101:15589 1332:1:2:3\n", few),
        ("a long instrument name", b"@" + filler + b":7:FC1:1:1101:15589:1332 c\n", ok),
        ("a long comment", b"@M01:7:FC1:1:1101:15589:1332 " + filler + b"\n", ok),
        ("a long 8th field", b"@M01:7:FC1:1:1101:15589:1332:" + filler + b"\n", ok),
        ("y across a chunk's edge", b"@M01:7:FC1:1:11:5:12345678\n", ok),
        ("the word ends with the first chunk", b"@M1:7:FC:1:1:2:3 c:c:c:c:c\n", ok),
        ("the word ends behind the first chunk", b"@M01:7:FC:1:1:2:3 c:c:c:c:c\n", ok),
        ("an empty line", b"", few),
        ("one byte", b"@", few),
        ("two bytes", b"@\n", few),
        ("five fields (pre-1.8)", b"@HWUSI:6:73:941:1973#0/1\n", few),
        ("six fields", b"@M01:7:FC1:1:1101:15589 c\n", few),
        ("SRA: the place stands in the comment", b"@SRR1.1 M01:7:FC1:1:1101:15589:1332\n", few),
        ("an empty first field", b"@:7:FC1:1:1101:15589:1332\n", empty),
        ("an empty lane", b"@M01:7:FC1::1101:15589:1332\n", empty),
        ("an empty tile", b"@M01:7:FC1:1::15589:1332\n", empty),
        ("an empty x", b"@M01:7:FC1:1:1101::1332\n", empty),
        ("an empty y at the word's end", b"@M01:7:FC1:1:1101:15589: c\n", empty),
        ("an empty y in front of a UMI", b"@M01:7:FC1:1:1101:15589::ACGT\n", empty),
        ("an empty field and a bad tile", b"@M01::FC1:1:11x1:15589:1332\n", empty),
        ("an empty 8th field is not looked at", b"@M01:7:FC1:1:1101:15589:1332:\n", ok),
        ("a letter in the tile", b"@M01:7:FC1:1:11x1:15589:1332\n", digit),
        ("a sign in x", b"@M01:7:FC1:1:1101:-5:1332\n", digit),
        ("y begins with a letter", b"@M01:7:FC1:1:1101:15589:y1332\n", digit),
        ("y is '_' only", b"@M01:7:FC1:1:1101:15589:_ACGT\n", digit),
        ("ten digits in the tile", b"@M01:7:FC1:1:1234567890:15589:1332\n", long_),
        ("ten digits in x", b"@M01:7:FC1:1:1101:0000000001:1332\n", long_),
        ("ten digits in y", b"@M01:7:FC1:1:1101:15589:1234567890\n", long_),
        ("twelve digits in y", b"@M01:7:FC1:1:1101:15589:123456789012_ACGT\n", long_),
        ("ten bytes in the tile, a letter among them", b"@M01:7:FC1:1:123456789x:15589:1332\n", digit),
        ("a letter behind y", b"@M01:7:FC1:1:1101:15589:1332a\n", end),
        ("a '+' behind y", b"@M01:7:FC1:1:1101:15589:1332+ACGT\n", end),
        ("a '.' behind y", b"@M01:7:FC1:1:1101:15589:13.5\n", end),
        ("the tile's reason comes first", b"@M01:7:FC1:1:1234567890:1x:1332a\n", long_),
        ("x's reason comes before y's", b"@M01:7:FC1:1:1101:1x:12345678901\n", digit),
    ]
