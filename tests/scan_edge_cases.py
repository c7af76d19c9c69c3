"""Texts for fqd_count_lines / fqd_scan_records (csrc/fqd_inflate.hip) whose newlines sit on the edges of the kernels'
units: a lane takes 32 bytes (kScanPer), a workgroup an 8 KiB tile (kScanTile), and the tile counts are scanned in parts
of 1024 tiles (launch_tile_offsets).  Every text is made from a list of line lengths with a seeded numpy generator; the
bytes between the newlines are filler.  tests/test_edge_inputs.py holds the texts to their own claims on the host,
tests/test_gpu_scan_edges.py holds the kernels to tests/record_reference.py on them.

A case is (name, text bytes, K): K = 4 lines per record (FASTQ, '@' leads, sequence and quality of equal length) or
K = 2 (FASTA, '>' leads).  MARKS[(name, K)] lists what the case planted: offsets of chosen '\\n' bytes and of chosen
record starts."""
from functools import lru_cache

import numpy as np

from record_reference import numpy_records

LANE, TILE, PART_TILES = 32, 8192, 1024
MAX_LINE = 300
KS = (4, 2)


class Lines:
    """Line lengths of whole records, and where the next record would start."""

    def __init__(self, k: int, seed: int):
        self.k, self.rng = k, np.random.default_rng(seed)
        self.lens, self.pos = [], 0
        self.newlines, self.record_starts = [], []

    @property
    def biggest(self):
        return (MAX_LINE + 1) * self.k

    def record(self, id_len: int, seq_len: int, plus_len: int = 1):
        assert id_len >= 1                                   # the lead byte
        ls = [id_len, seq_len] if self.k == 2 else [id_len, seq_len, plus_len, seq_len]
        self.lens += ls
        self.pos += sum(ls) + self.k

    def ragged_record(self):
        r = self.rng.integers(0, MAX_LINE + 1, 3)
        self.record(max(1, int(r[0])), int(r[1]), int(r[2]))

    def ragged(self, until: int):
        """Ragged records (line lengths 0..300) while one more still leaves eight bytes before `until`."""
        while self.pos + self.biggest + 8 <= until:
            self.ragged_record()

    def id_newline_at(self, p: int):
        """The next record's ID line is padded so that its '\\n' is byte p of the text."""
        self.newlines.append(p)
        self.record(p - self.pos, int(self.rng.integers(0, 40)))

    def land(self, target: int, last: bool = False):
        """One record, its ID line padded so that the record's last '\\n' is byte target - 1: the next record starts at target."""
        room = target - self.pos
        if self.k == 4:
            assert room >= 6
            seq = min(int(self.rng.integers(0, 20)), (room - 6) // 2)
            self.record(room - 5 - 2 * seq, seq)
        else:
            assert room >= 3
            seq = min(int(self.rng.integers(0, 20)), room - 3)
            self.record(room - 2 - seq, seq)
        assert self.pos == target
        self.newlines.append(target - 1)
        if not last:
            self.record_starts.append(target)


def build_text(lens, k: int, seed: int) -> bytes:
    ll = np.asarray(lens, dtype=np.int64)
    ends = np.cumsum(ll + 1) - 1                             # the '\n' of every line
    starts = ends - ll
    n = int(ends[-1]) + 1
    rng = np.random.default_rng(seed)
    text = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, n)]
    text[ends] = 10
    text[starts[0::k]] = ord("@") if k == 4 else ord(">")
    if k == 4:
        plus = starts[2::4]
        text[plus[ll[2::4] > 0]] = ord("+")
    return text.tobytes()


# ---- the cases: name -> function(Lines) ------------------------------------------------------------------------------
def _lane_edges(b):
    """Newlines on a lane's last byte (offset = 31 mod 32) and on a lane's first byte (= 0 mod 32), in turn; ends anywhere."""
    b.id_newline_at(31)
    for _ in range(6):
        b.id_newline_at((b.pos + LANE) // LANE * LANE)           # the next offset = 0 (mod 32) at least one byte on
        b.id_newline_at((b.pos + 1 + LANE) // LANE * LANE - 1)   # the next offset = 31 (mod 32)
    b.record(3, 9)


def _tile_edges(b):
    """Newlines on a tile's last byte and first byte; a record that starts on a tile's first byte, one on its last byte."""
    b.ragged(TILE - 1)
    b.id_newline_at(TILE - 1)
    b.ragged(2 * TILE)
    b.id_newline_at(2 * TILE)
    b.ragged(3 * TILE)
    b.land(3 * TILE)                                         # '\n' at 8191 (mod 8192), the next record on a tile's first byte
    b.ragged_record()
    b.ragged(4 * TILE - 1)
    b.land(4 * TILE - 1)                                     # the next record starts on a tile's last byte
    b.record(1, 5)                                           # "@\n": its ID line's '\n' is the next tile's first byte
    b.newlines.append(4 * TILE)
    b.ragged(5 * TILE)
    b.land(5 * TILE, last=True)                              # and the text's last byte is a tile's last byte


def _length(n):
    def make(b):
        b.ragged(n)
        b.land(n, last=True)
    return make


def _one_record(b):
    b.record(2, 2) if b.k == 4 else b.record(2, 7)          # 11 bytes either way


def _empty_lines(b):
    """Records with an empty sequence (and quality) line among normal ones; two of them side by side, one at the end."""
    for j in range(400):
        if j % 3 == 0 or j in (100, 101):
            b.record(2, 0)                                   # "@x\n\n+\n\n"
        else:
            b.ragged_record()
    b.record(2, 0)


def _long_lines(b):
    """Reads of 20 000 and 70 000 bytes among short ones: tiles in a row without a newline, then a tile with many."""
    for _ in range(30):
        b.record(int(b.rng.integers(1, 12)), int(b.rng.integers(0, 12)))
    b.record(7, 20_000)
    for _ in range(300):
        b.record(int(b.rng.integers(1, 6)), int(b.rng.integers(0, 4)))     # many newlines in one tile
    b.record(9, 70_000)
    b.record(4, 0)
    b.record(3, 70_000)
    for _ in range(50):
        b.ragged_record()


def _tiles_1024(b):
    """Exactly one part: the last '\\n' is the last byte of the part's last tile."""
    b.ragged(PART_TILES * TILE)
    b.land(PART_TILES * TILE, last=True)


def _tiles_1025(b):
    """A second part of one tile.  A record starts on a tile's first byte inside the first part, and the second part's
    first record starts on its first byte; the last record has a sequence, so that the damage cases can shorten it."""
    b.ragged(17 * TILE)
    b.land(17 * TILE)
    b.ragged(PART_TILES * TILE)
    b.land(PART_TILES * TILE)
    for _ in range(4):
        b.ragged_record()
    b.record(5, 6)
    assert PART_TILES * TILE < b.pos <= (PART_TILES + 1) * TILE


def _tiles_2049(b):
    """Three parts; the part edges fall inside lines."""
    b.ragged(2 * PART_TILES * TILE + 5000)
    b.land(2 * PART_TILES * TILE + 5000, last=True)


SMALL = {"lane_edges": _lane_edges, "tile_edges": _tile_edges, "one_record": _one_record, "empty_lines": _empty_lines,
         "long_lines": _long_lines}
SMALL.update({"n_%d" % n: _length(n) for n in (64, 65, 95)})                                     # n mod 32 = 0, 1, 31
SMALL.update({"n_%dx8192+%d" % (t, r): _length(t * TILE + r) for t in (1, 2) for r in (0, 1, TILE - 1)})
PARTS = {"tiles_1024": _tiles_1024, "tiles_1025": _tiles_1025, "tiles_2049": _tiles_2049}
PART_TILE_COUNTS = {"tiles_1024": 1024, "tiles_1025": 1025, "tiles_2049": 2049}
ALL = {**SMALL, **PARTS}
MARKS = {}


@lru_cache(maxsize=None)
def text_of(name: str, k: int) -> bytes:
    seed = 1000 + 10 * sorted(ALL).index(name) + k
    b = Lines(k, seed)
    ALL[name](b)
    text = build_text(b.lens, k, seed + 1)
    assert len(text) == b.pos
    MARKS[(name, k)] = {"newlines": tuple(b.newlines), "record_starts": tuple(b.record_starts)}
    return text


def marks(name: str, k: int):
    text_of(name, k)
    return MARKS[(name, k)]


def small_cases():
    """(name, text, K) of every well-formed case of tile scale or smaller."""
    for k in KS:
        for name in SMALL:
            yield name, text_of(name, k), k


def part_cases():
    """(name, text, K) of the cases of 1024, 1025 and 2049 tiles."""
    for k in KS:
        for name in PARTS:
            yield name, text_of(name, k), k


def well_formed():
    yield from small_cases()
    yield from part_cases()


def ids(names, ks=KS):
    return [(name, k) for k in ks for name in names]


# ---- text that is not records: fqd_count_lines alone -----------------------------------------------------------------
def line_count_cases():
    """(name, bytes): every mask bit set, none set, and the one-byte texts."""
    rng = np.random.default_rng(77)
    yield "only_newlines", b"\n" * (3 * TILE + 5)
    yield "no_newline", np.frombuffer(b"ACGT@+>", np.uint8)[rng.integers(0, 7, 3 * TILE + 5)].tobytes()
    yield "one_byte_newline", b"\n"
    yield "one_byte_other", b"A"


# ---- damage: the 1025-tile FASTQ text, which must be reported as not well formed ----------------------------------------
DAMAGE = ("bad_lead_on_tile_start", "bad_lead_first_of_second_part", "length_mismatch_last_record", "no_final_newline", "extra_line")


def damaged(kind: str) -> bytes:
    text = text_of("tiles_1025", 4)
    start = numpy_records(text, 4)[0]
    if kind == "bad_lead_on_tile_start":
        s = int(start[(start % TILE == 0) & (start > 0) & (start < PART_TILES * TILE)][0])
        return text[:s] + b"A" + text[s + 1:]
    if kind == "bad_lead_first_of_second_part":
        s = int(start[start >= PART_TILES * TILE][0])
        return text[:s] + b"A" + text[s + 1:]
    if kind == "length_mismatch_last_record":
        return text[:-2] + b"\n"                             # one quality byte fewer
    if kind == "no_final_newline":
        return text[:-1]
    assert kind == "extra_line"
    return text + b"@x\n"
