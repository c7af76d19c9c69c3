"""A deflate WRITER for the tests, by hand (RFC 1951): every compressed byte the suite fed to the GPU readers used to come
from zlib's deflater or from this project's own; real files come from libdeflate, igzip, zopfli, 7-zip and sequencers'
converters, which write legal streams in shapes zlib's deflater never emits.  Here the caller decides everything: the
code lengths of both alphabets, how the lengths are written (HLIT, HDIST, HCLEN, the run-length coding, the code-length
code), which symbol and extra bits spell a length, where blocks begin and end.  Raw hooks write what is NOT legal, for
the error paths.  Nothing here looks at what the project's decoders do: tests/handmade_deflate_cases.py holds every
stream against zlib's inflater before it is used.

Tokens: an int is a literal; (length, distance) is a match, (length, distance, symbol) one whose length is spelt with
that length symbol (258 is symbol 285, or symbol 284 with extra bits 31); Raw(...) items write bits that `expand`
refuses to interpret."""
import heapq
import struct
import zlib

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    """Bits least significant first; Huffman codes most significant bit first."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, count):
        assert 0 <= value < (1 << count) or count == 0
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        rev = 0
        for _ in range(length):
            rev = (rev << 1) | (code & 1)
            code >>= 1
        self.bits(rev, length)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw_bytes(self, data):
        assert self.n == 0
        self.out += data

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical_codes(lengths):
    """code[s] for every symbol with a length, as RFC 1951 3.2.2 assigns them (an over-subscribed set still gets numbers:
    the raw hooks write those)."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def kraft(lengths):
    """Sum of 2^-l in units of 2^-15: 32768 is a complete set."""
    return sum(1 << (15 - l) for l in lengths if l)


def balanced_lengths(freqs, limit=15):
    """A complete set of lengths for the symbols with freqs[s] > 0 (two at least): Huffman's, or, where those run deeper
    than `limit`, all codes of two neighbouring lengths, the frequent symbols the shorter."""
    used = [s for s, f in enumerate(freqs) if f]
    assert len(used) >= 2
    lens = [0] * len(freqs)
    heap = [(freqs[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    depth = dict.fromkeys(used, 0)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    if max(depth.values()) <= limit:
        for s in used:
            lens[s] = depth[s]
    else:
        k = (len(used) - 1).bit_length()
        short = (1 << k) - len(used)
        for rank, s in enumerate(sorted(used, key=lambda s: -freqs[s])):
            lens[s] = k - 1 if rank < short else k
    assert kraft(lens) == 32768
    return lens


def length_symbol(length):
    """The usual spelling: the symbol with the largest base <= length (258: symbol 285)."""
    assert 3 <= length <= 258
    for k in range(28, -1, -1):
        if LENGTH_BASE[k] <= length:
            return 257 + k
    raise AssertionError


def dist_symbol(distance):
    assert 1 <= distance <= 32768
    for k in range(29, -1, -1):
        if DIST_BASE[k] <= distance:
            return k
    raise AssertionError


class Raw:
    """Bits written as they are, in a token list: ("bits", value, count), ("lit", symbol) — the literal/length code of any
    symbol that has one, 286 and 287 included —, ("dist", symbol, extra value, extra bits)."""

    def __init__(self, *item):
        self.item = item


def expand(tokens, history=b""):
    """The text the tokens stand for (behind `history`, which matches may reach into)."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        assert not isinstance(t, Raw), "raw bits have no meaning"
        length, distance = t[0], t[1]
        assert 3 <= length <= 258 and 1 <= distance <= len(out), (length, distance, len(out))
        if distance >= length:
            out += out[len(out) - distance:len(out) - distance + length]
        else:
            for _ in range(length):
                out.append(out[-distance])
    return bytes(out[len(history):])


def token_usage(tokens):
    """How often every literal/length and distance symbol occurs (the end-of-block code once)."""
    lit, dist = [0] * 286, [0] * 30
    lit[256] = 1
    for t in tokens:
        if isinstance(t, int):
            lit[t] += 1
        elif not isinstance(t, Raw):
            lit[t[2] if len(t) > 2 else length_symbol(t[0])] += 1
            dist[dist_symbol(t[1])] += 1
    return lit, dist


def code_length_runs(seq, mode="greedy"):
    """The code-length sequence as (symbol, extra value, first index, count) items.  "none": every length as itself; "greedy":
    the longest run code at every place, over the whole sequence — a run does not care where the literal/length lengths end."""
    items, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if mode == "none":
            items.append((v, 0, i, 1)); i += 1
        elif v == 0 and run >= 11:
            n = min(run, 138); items.append((18, n - 11, i, n)); i += n
        elif v == 0 and run >= 3:
            items.append((17, run - 3, i, run)); i += run
        elif v != 0 and i > 0 and seq[i - 1] == v and run >= 3:
            n = min(run, 6); items.append((16, n - 3, i, n)); i += n
        else:
            items.append((v, 0, i, 1)); i += 1
    return items


CL_EXTRA = {16: 2, 17: 3, 18: 7}


class Deflate:
    """One raw deflate stream, block after block."""

    def __init__(self):
        self.w = BitWriter()

    # ---- blocks
    def header(self, last, btype):
        self.w.bits(1 if last else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data, last=False, nlen=None):
        assert len(data) <= 65535
        self.header(last, 0)
        self.w.align()
        self.w.bits(len(data), 16)
        self.w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.w.raw_bytes(data)

    def fixed(self, tokens, last=False, end=True):
        self.header(last, 1)
        self.tokens(tokens, FIXED_LIT, FIXED_DIST, end)

    def dynamic(self, lit_lens, dist_lens, tokens, last=False, hlit=None, hdist=None, hclen=None, rle="greedy", cl_lens=None, cl_items=None, end=True):
        """lit_lens / dist_lens: lengths by symbol.  hlit, hdist: how many of them are written (default: without the zeros at
        their ends, 257 and 1 at least; larger values keep zeros, values the format does not allow go out as they are).
        rle: "none" | "greedy"; cl_items: the (symbol, extra) sequence itself.  cl_lens: the code-length code's 19 lengths
        (default: a complete code for the symbols that occur); hclen: how many of them are written.  Returns the items written."""
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        if hlit is None:
            hlit = max(257, max((s + 1 for s, l in enumerate(lit_lens) if l), default=0))
        if hdist is None:
            hdist = max(1, max((s + 1 for s, l in enumerate(dist_lens) if l), default=0))
        lit_lens += [0] * (hlit - len(lit_lens))
        dist_lens += [0] * (hdist - len(dist_lens))
        seq = lit_lens[:hlit] + dist_lens[:hdist]
        items = cl_items if cl_items is not None else code_length_runs(seq, rle)
        if cl_lens is None:
            freq = [0] * 19
            for it in items:
                freq[it[0]] += 1
            if sum(1 for f in freq if f) < 2:                       # zlib wants this code complete: a second symbol, never used
                freq[next(s for s in (0, 1) if not freq[s])] = 1
            cl_lens = balanced_lengths(freq, 7)
        if hclen is None:
            hclen = max(4, max(k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]))
        self.hclen = hclen
        self.header(last, 2)
        self.w.bits(hlit - 257, 5)
        self.w.bits(hdist - 1, 5)
        self.w.bits(hclen - 4, 4)
        for k in range(hclen):
            self.w.bits(cl_lens[CL_ORDER[k]], 3)
        cl_codes = canonical_codes(cl_lens)
        self.lengths_from = self.w.bitpos                     # (of the block written last: where its code lengths and its codes begin)
        for it in items:
            sym, extra = it[0], it[1]
            assert cl_lens[sym], ("no code for code-length symbol", sym)
            self.w.code(cl_codes[sym], cl_lens[sym])
            if sym >= 16:
                self.w.bits(extra, CL_EXTRA[sym])
        self.codes_from = self.w.bitpos
        self.tokens(tokens, lit_lens, dist_lens, end)
        return items

    def tokens(self, tokens, lit_lens, dist_lens, end=True):
        lc, dc = canonical_codes(lit_lens), canonical_codes(dist_lens)
        w = self.w

        def lit(s):
            assert s < len(lit_lens) and lit_lens[s], ("no code for literal/length symbol", s)
            w.code(lc[s], lit_lens[s])

        for t in tokens:
            if isinstance(t, int):
                lit(t)
            elif isinstance(t, Raw):
                it = t.item
                if it[0] == "bits":
                    w.bits(it[1], it[2])
                elif it[0] == "lit":
                    lit(it[1])
                else:
                    w.code(dc[it[1]], dist_lens[it[1]]); w.bits(it[2], it[3])
            else:
                length, distance = t[0], t[1]
                ls = t[2] if len(t) > 2 else length_symbol(length)
                extra = length - LENGTH_BASE[ls - 257]
                assert 0 <= extra < (1 << LENGTH_EXTRA[ls - 257]) or (extra == 0 and LENGTH_EXTRA[ls - 257] == 0), (length, ls)
                lit(ls)
                w.bits(extra, LENGTH_EXTRA[ls - 257])
                ds = dist_symbol(distance)
                assert ds < len(dist_lens) and dist_lens[ds], ("no code for distance symbol", ds)
                w.code(dc[ds], dist_lens[ds])
                w.bits(distance - DIST_BASE[ds], DIST_EXTRA[ds])
        if end:
            lit(256)

    def auto(self, tokens, last=False, **kw):
        """A dynamic block whose two codes are Huffman's for the tokens."""
        lit, dist = token_usage(tokens)
        if sum(1 for f in lit if f) < 2:
            lit[0 if lit[0] == 0 else 1] = 1
        n_dist = sum(1 for f in dist if f)
        dist_lens = [0] * 30 if n_dist == 0 else [1 if f else 0 for f in dist] if n_dist == 1 else balanced_lengths(dist)
        return self.dynamic(balanced_lengths(lit), dist_lens, tokens, last, **kw)

    @property
    def bitpos(self):
        return self.w.bitpos

    def getvalue(self):
        return self.w.getvalue()


def lz_tokens(data, start=0, end=None, max_dist=32768, min_len=3, max_len=258):
    """data[start:end) as literals and matches (which may reach back before `start`): the latest earlier place with the same
    three bytes, taken as far as it goes.  Nothing clever; a source of realistic token streams."""
    end = len(data) if end is None else end
    seen, toks, i = {}, [], start
    for k in range(max(0, start - max_dist), start):
        seen[data[k:k + 3]] = k
    while i < end:
        key = data[i:i + 3]
        j = seen.get(key)
        n = 0
        if j is not None and i - j <= max_dist and i + 3 <= end:
            limit = min(max_len, end - i)
            while n < limit and data[j + n] == data[i + n]:
                n += 1
        if n >= min_len:
            toks.append((n, i - j))
            for k in range(i, i + n):
                seen[data[k:k + 3]] = k
            i += n
        else:
            toks.append(data[i])
            seen[key] = i
            i += 1
    return toks


def bgzf_member(body: bytes, raw: bytes, isize=None) -> bytes:
    """The deflate stream `body` as one BGZF member whose trailer is that of `raw` (isize: what the trailer claims instead)."""
    total = 18 + len(body) + 8
    assert total <= 65536 and len(raw) <= 65536
    return (bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", total - 1) + body +
            struct.pack("<II", zlib.crc32(raw), len(raw) if isize is None else isize))


def gzip_member(body: bytes, raw: bytes, header=b"") -> bytes:
    head = header or b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03"
    return head + body + struct.pack("<II", zlib.crc32(raw) & 0xFFFFFFFF, len(raw) & 0xFFFFFFFF)
