"""Deflate streams written by hand (tests/deflate_writer.py): legal shapes zlib's deflater never emits, and illegal ones.

THE SPECIFICATION IS zlib's INFLATER.  Every valid case is inflated with `zlib.decompressobj(-15)` here, in the generator,
and must give exactly `expand(tokens)` and reach the end of the stream; every invalid case must make zlib refuse the stream
(`zlib.error`).  A case that fails that is a bug of the writer — it is never mended by looking at what the project's
decoders make of it, and no expected value anywhere comes from them.

Two things the list of shapes asked for cannot exist as VALID streams, and are here as what they can be:
  * four code-length-code lengths (HCLEN's smallest count) give codes to 16, 17, 18 and 0 only, so every length is zero and the
    end-of-block symbol has no code: zlib refuses it (`hclen_4_leaves_no_end_code`, invalid); the smallest valid count is five
    (`hclen_5_smallest_valid`), the largest nineteen (`hclen_19`);
  * a run of 138 zeros cannot END at HLIT + HDIST, because symbol 256 must have a length and lies at most 59 places from the
    end: the longest zero run that ends there is 59 (`zero_run_59_ends_at_hlit_plus_hdist`); the run of 138 is at the front
    (`zero_run_138`), and overruns the end in `run_overruns_hlit_plus_hdist` (invalid).
"""
import functools
import itertools
import random
import zlib

from bgzf_cases import fastq_text
from deflate_writer import (DIST_BASE, DIST_EXTRA, LENGTH_BASE, LENGTH_EXTRA, Deflate, Raw, balanced_lengths, bgzf_member, code_length_runs,
                            expand, gzip_member, kraft, lz_tokens)

EOF_MARK = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
TOKEN_ROOM = 12288                       # fqd::winf::kTokenRoom (tests/test_inflate_core.py holds the two together)
LITS = b"ACGTN@+\nIF#:r1,"              # fifteen literals

# Seeded random cases: RANDOM_TRIALS per seed.  The generator (both codes drawn, tokens drawn, written, inflated by zlib) takes
# 19 ms a trial on the CPU this was sized on (50 trials: 0.94 s), a decode a few milliseconds at most: 100 trials keep each
# seed's test at a few seconds.
RANDOM_SEEDS = (20240607, 7)
RANDOM_TRIALS = 100


def lens(n, *groups, complete=True):
    """lens(n, (symbols, length), ...): lengths by symbol."""
    out = [0] * n
    for symbols, length in groups:
        for s in ([symbols] if isinstance(symbols, int) else symbols):
            assert out[s] == 0
            out[s] = length
    assert not complete or kraft(out) == 32768, kraft(out)
    return out


def staircase(n, symbols):
    """1, 2, ..., 14, 15, 15 over sixteen symbols."""
    assert len(symbols) == 16
    return lens(n, *[(s, min(k + 1, 15)) for k, s in enumerate(symbols)])


def random_tokens(rnd, lit_lens, dist_lens, count, have=0, room=60000, p_match=0.4):
    """`count` tokens the two codes can spell, behind `have` bytes of text; every length symbol with extra bits drawn."""
    lits = [s for s in range(min(256, len(lit_lens))) if lit_lens[s]]
    lsyms = [s for s in range(257, min(286, len(lit_lens))) if lit_lens[s]]
    dsyms = [d for d in range(min(30, len(dist_lens))) if dist_lens[d]]
    toks = []
    for _ in range(count):
        ok = [d for d in dsyms if DIST_BASE[d] <= have] if lsyms else []
        if ok and (not lits or rnd.random() < p_match):
            ls = rnd.choice(lsyms)
            length = LENGTH_BASE[ls - 257] + rnd.randrange(1 << LENGTH_EXTRA[ls - 257])
            d = rnd.choice(ok)
            distance = min(have, DIST_BASE[d] + rnd.randrange(1 << DIST_EXTRA[d]))
            if have + length > room:
                break
            toks.append((length, distance, ls)); have += length
        elif lits:
            if have + 1 > room:
                break
            toks.append(rnd.choice(lits)); have += 1
        else:
            break
    return toks


def check_valid(name, body, text):
    d = zlib.decompressobj(-15)
    got = d.decompress(body)
    assert got == text and d.eof and d.unused_data == b"", f"the writer is wrong, not the decoders: {name}"


def check_invalid(name, body):
    try:
        zlib.decompress(body, -15)
    except zlib.error:
        return
    raise AssertionError(f"zlib takes what was meant to be illegal: {name}")


# sets of lengths several cases share
LIT_A = lens(286, (list(LITS) + [256], 5), (range(257, 265), 4))                       # 16 five-bit codes, lengths 3..10 at four bits
DIST_16 = lens(30, (range(16), 4))
LIT_STAIRS = staircase(286, [65, 67, 71, 84, 10, 70, 78, 73, 64, 43, 256, 257, 258, 35, 58, 44])
DIST_STAIRS = staircase(30, list(range(16)))


def _valid():
    """(name, text, deflate stream, fits a BGZF member)"""
    out = []

    def add(name, d, toks_or_text, bgzf=True):
        text = toks_or_text if isinstance(toks_or_text, bytes) else expand(toks_or_text)
        body = d.getvalue()
        check_valid(name, body, text)
        assert not bgzf or (len(text) <= 65536 and len(body) + 26 <= 65536), name
        assert all(n != name for n, *_ in out)
        out.append((name, text, body, bgzf))

    def one_block(name, lit_lens, dist_lens, seed=1, count=3000, **kw):
        """One final dynamic block of drawn tokens; returns the code-length items written."""
        rnd = random.Random(seed)
        toks = random_tokens(rnd, lit_lens, dist_lens, count)
        d = Deflate()
        items = d.dynamic(lit_lens, dist_lens, toks, last=True, **kw)
        add(name, d, toks)
        return items

    def crosses(items, sym, at):
        return any(it[0] == sym and it[2] < at < it[2] + it[3] for it in items)

    # ---- header shapes
    items = one_block("code16_run_crosses_hlit", LIT_A, DIST_16)
    assert crosses(items, 16, 265)
    items = one_block("code17_run_crosses_hlit", LIT_A, lens(30, (range(4, 20), 4)), hlit=269)
    assert crosses(items, 17, 269)
    items = one_block("code18_run_crosses_hlit", LIT_A, lens(30, (range(6, 22), 4)), hlit=275)
    assert crosses(items, 18, 275)
    items = one_block("no_run_length_codes", LIT_A, DIST_16, rle="none")
    assert all(it[0] < 16 for it in items)
    d = Deflate()
    toks = random_tokens(random.Random(2), lens(257, (list(range(255)) + [256], 8)), [0], 2000)
    d.dynamic(lens(257, (list(range(255)) + [256], 8)), [0], toks, last=True, rle="none")
    assert d.hclen == 5
    add("hclen_5_smallest_valid", d, toks)
    one_block("hclen_19", LIT_STAIRS, DIST_16, hclen=19)
    one_block("hlit_257", lens(257, (list(LITS) + [256], 4)), [0], hlit=257)
    one_block("hlit_286", lens(286, (list(LITS) + [256], 5), (list(range(257, 264)) + [285], 4)), DIST_16, hlit=286)
    one_block("hdist_1", LIT_A, [1], hdist=1)
    rnd = random.Random(3)
    hist = bytes(rnd.choice(LITS) for _ in range(24600))
    d = Deflate(); d.stored(hist)
    dl = lens(30, (list(range(15)) + [29], 4))
    toks = random_tokens(rnd, LIT_A, dl, 3000, have=len(hist)) + [(10, 24577), (9, 24600)]
    d.dynamic(LIT_A, dl, toks, last=True, hdist=30)
    add("hdist_30", d, hist + expand(toks, hist))
    lit_3456 = lens(286, (list(LITS[:4]), 3), (list(LITS[4:8]), 4), (list(LITS[8:12]), 5), (list(LITS[12:15]) + [50, 51, 256, 257, 258], 6))
    dist_3456 = lens(30, (range(4), 3), (range(4, 8), 4), (range(8, 12), 5), (range(12, 20), 6))
    one_block("code_length_code_of_7_bits", lit_3456, dist_3456, cl_lens=lens(19, (0, 1), (6, 2), (5, 3), (4, 4), (3, 5), (16, 6), ((17, 18), 7)))
    items = one_block("zero_run_138", lens(286, (list(range(138, 153)) + [256], 5), (range(257, 265), 4)), DIST_16)
    assert items[0] == (18, 127, 0, 138)
    items = one_block("zero_run_59_ends_at_hlit_plus_hdist", lens(257, (list(LITS) + [256], 4)), [0], hlit=286, hdist=30)
    assert items[-1][0] == 18 and items[-1][2] + items[-1][3] == 316 and items[-1][3] == 59

    # ---- code lengths
    one_block("staircase_1_to_15_15_literals", LIT_STAIRS, DIST_16, seed=4)
    one_block("staircase_1_to_15_15_distances", LIT_A, DIST_STAIRS, seed=5)
    one_block("staircase_1_to_15_15_both", LIT_STAIRS, DIST_STAIRS, seed=6)
    one_block("literal_codes_of_10_and_11_bits", lens(286, *[(s, k + 1) for k, s in enumerate(LITS[:8])], ((LITS[8], 257), 10), ((LITS[9], LITS[10], LITS[11], 256), 11)),
              DIST_16, seed=7)
    lit_34 = lens(286, (list(b"ACGT"), 3), (list(b"N\n@+IF") + [256, 257], 4))
    toks = []
    for tri in itertools.product(b"ACNI", repeat=3):                        # every sum of three code lengths from 9 to 12, at every bit offset
        toks += list(tri)
    toks += [(3, 1)] + toks[:97]
    d = Deflate(); d.dynamic(lit_34, [1], toks, last=True)
    add("three_literals_of_9_10_11_bits", d, toks)
    lit_l = lens(286, (list(b"ACGT"), 3), (list(b"N\n") + [256, 257, 258, 259, 260, 261], 4))
    toks = list(b"ACGTNACG")
    for k in range(400):                                                      # two three-bit literals and a four-bit length code: one 10-bit index
        toks += [b"ACGT"[k & 3], b"ACGT"[(k >> 2) & 3], (3 + k % 5, 1 + k % 8)] + ([78] if k % 3 == 0 else [])
    d = Deflate(); d.dynamic(lit_l, lens(30, (range(8), 3)), toks, last=True)
    add("two_literals_then_a_length_in_one_index", d, toks)
    one_block("distance_codes_of_9_and_10_bits", LIT_A, lens(30, *[(k, k + 1) for k in range(7)], ((7, 8), 9), ((9, 10, 11, 12), 10)), seed=8, count=6000)

    # ---- incomplete sets zlib lets pass
    one_block("no_distance_code", lens(257, (list(LITS) + [256], 4)), [0], hdist=1)
    one_block("one_distance_code_of_1_bit", LIT_A, [1], seed=9)
    one_block("one_distance_code_of_1_bit_symbol_3", LIT_A, [0, 0, 0, 1], seed=10)
    text = fastq_text(20, 1)
    only_end = lens(257, (256, 1), complete=False)
    d = Deflate(); d.dynamic(only_end, [0], [], last=False); d.stored(text, last=True)
    add("single_1_bit_end_code_then_stored", d, text)
    d = Deflate()
    for _ in range(200):
        d.dynamic(only_end, [0], [], last=False)
    toks = lz_tokens(text)
    d.auto(toks, last=True)
    add("single_1_bit_end_code_200_times", d, text)

    # ---- every length and distance symbol
    toks = list(b"ACGTACGTAC")
    for ls in range(257, 286):
        for extra in {0, (1 << LENGTH_EXTRA[ls - 257]) - 1}:
            toks += [(LENGTH_BASE[ls - 257] + extra, 1 + (ls * 7 + extra) % 10, ls), 65 + ls % 20]
    ms = [t for t in toks if not isinstance(t, int)]
    assert any(t[0] == 258 and t[2] == 284 for t in ms) and any(t[0] == 258 and t[2] == 285 for t in ms)      # 258 by both spellings
    d = Deflate(); d.fixed(toks, last=True); add("every_length_symbol_fixed", d, toks)
    d = Deflate(); d.auto(toks, last=True); add("every_length_symbol_dynamic", d, toks)
    rnd = random.Random(11)
    hist = bytes(rnd.randrange(256) for _ in range(32768))
    toks = []
    for ds in range(30):
        for extra in {0, (1 << DIST_EXTRA[ds]) - 1}:
            toks += [(3 + ds % 6, DIST_BASE[ds] + extra), 48 + ds]
    assert any(not isinstance(t, int) and t[1] == 32768 for t in toks)
    for kind in ("fixed", "dynamic"):
        d = Deflate(); d.stored(hist)
        d.fixed(toks, last=True) if kind == "fixed" else d.auto(toks, last=True)
        add(f"every_distance_symbol_{kind}", d, hist + expand(toks, hist))
    d = Deflate(); d.stored(hist); d.fixed([(258, 32768), 10, (3, 32768)], last=True)
    add("distance_32768_reaches_the_first_byte", d, hist + expand([(258, 32768), 10, (3, 32768)], hist))
    toks = list(b"@r1\nACGTTGCA\n+\nIIIIFFFF\n") + [(24, 24), 88, (258, 49), (100, 307), (3, 407)]
    d = Deflate(); d.auto(toks, last=True); add("match_source_starts_at_byte_0", d, toks)

    # ---- match shapes
    toks = list(b"ABCDEFGH")
    for dist in range(1, 9):
        toks += [(258, dist), 97 + dist, 48 + dist]
    d = Deflate(); d.auto(toks, last=True); add("distances_1_to_8_with_length_258", d, toks)
    toks = [rnd.choice(LITS) for _ in range(300)]
    for n in (3, 4, 7, 8, 9, 15, 16, 17, 23, 24, 25, 64, 129, 258):
        toks += [(n, n), 33, (n, n - 1) if n > 3 else (n, n), 34]
    d = Deflate(); d.auto(toks, last=True); add("distance_equal_to_length_and_one_less", d, toks)
    for depth in (65, 129, 1000):                                             # deeper than one group of 64 matches, than several
        toks = list(b"ACGTNIF#")
        for k in range(depth):
            toks.append((8, 8) if k % 3 else (5, 5))                          # match k copies what match k - 1 wrote
        d = Deflate(); d.auto(toks, last=True); add(f"chain_of_matches_depth_{depth}", d, toks)
        toks = list(b"ACGTNIF#")
        for k in range(depth):
            toks += [(6, 7), 65 + k % 26]                                     # ... and the literal before it
        d = Deflate(); d.auto(toks, last=True); add(f"chain_of_matches_and_literals_depth_{depth}", d, toks)
    toks = [rnd.choice(LITS) for _ in range(40)] + [(10, 20), 120, 121, (8, 6), (30, 37), 122, (40, 3), (20, 45), (258, 150)]
    d = Deflate(); d.auto(toks, last=True); add("match_source_straddles_the_previous_match", d, toks)
    for extra, name in ((0, "exactly_the_token_room"), (3, "three_more_than_the_token_room")):
        toks = [((3, 3), (3, 7), (3, 8), (3, 3))[k & 3] for k in range(TOKEN_ROOM + extra)]
        d = Deflate(); d.stored(b"ABCDEFGH")
        d.dynamic(lens(258, ((256, 257), 1)), lens(6, ((2, 5), 1)), toks, last=True)
        add(f"three_byte_matches_{name}", d, b"ABCDEFGH" + expand(toks, b"ABCDEFGH"))

    # ---- block sequences
    base = lz_tokens(fastq_text(6, 2))
    for k in range(8):
        for pad in range(16):
            d = Deflate(); toks = base + [200] * pad                         # (a nine-bit literal a time moves the end by one bit)
            d.fixed(toks)
            if d.bitpos % 8 == k:
                break
        assert d.bitpos % 8 == k
        d.stored(b""); more = [(30, 60), 10]; d.fixed(more, last=True)
        add(f"empty_stored_block_after_a_block_ending_at_bit_{k}", d, expand(toks + more))
    d = Deflate(); d.auto(base); d.stored(b"", last=True); add("final_stored_block_of_length_0", d, base)
    d = Deflate()
    for _ in range(1000):
        d.fixed([])
    d.auto(base, last=True); add("1000_empty_fixed_blocks", d, base)
    text = fastq_text(40, 3)
    q = len(text) // 4
    d = Deflate(); d.stored(text[:q])
    for k, how in enumerate(("auto", "fixed", "auto")):                      # every block opens with a match into the one before it
        lo, hi = q * (k + 1), (q * (k + 2) if k < 2 else len(text))
        toks = [(40, q - 3), (258, q + 40 - 7)] + lz_tokens(text, lo, hi)
        piece = expand(toks, text[:lo] if k == 0 else whole)
        whole = (text[:lo] if k == 0 else whole) + piece
        d.fixed(toks, last=k == 2) if how == "fixed" else d.auto(toks, last=k == 2)
    add("stored_dynamic_fixed_dynamic_reaching_back", d, whole)
    for k, name in ((0, "last_bit_of_the_last_byte"), (1, "first_bit_of_the_last_byte")):
        for pad in range(16):
            d = Deflate(); toks = base + [200] * pad; d.fixed(toks, last=True)
            if d.bitpos % 8 == k:
                break
        assert d.bitpos % 8 == k
        add(f"end_code_ends_on_the_{name}", d, toks)
    d = Deflate(); big = (fastq_text(200, 4) * 2)[:65535]; d.stored(big); d.auto(base, last=True)
    add("stored_block_of_65535_bytes", d, big + expand(base), bgzf=False)

    # ---- ordinary gzip: where units start is guessed
    fq = fastq_text(700, 5)                                                   # ~ 260 KB
    fake = Deflate(); fake.auto(lz_tokens(fq[:9000]), last=False); fake.auto(lz_tokens(fq[9000:12000]), last=False)
    payload = fake.getvalue()                                                 # complete dynamic blocks, byte-aligned in the stored block: a start where none is
    d = Deflate(); parts = []
    for _ in range(6):
        d.stored(payload); parts.append(payload)
    at = 0
    while at < len(fq):
        d.auto(lz_tokens(fq, at, min(at + 20000, len(fq))), last=at + 20000 >= len(fq)); at += 20000
    add("stored_payload_that_looks_like_block_starts", d, b"".join(parts) + fq, bgzf=False)
    d = Deflate(); at = 0
    fq2 = fastq_text(500, 6)
    while at < len(fq2):                                                      # a few records a block
        step = 700 + at % 900
        d.auto(lz_tokens(fq2, at, min(at + step, len(fq2))), last=at + step >= len(fq2)); at += step
    add("many_tiny_dynamic_blocks", d, fq2, bgzf=False)
    d = Deflate(); at = 0; whole = b""
    fq3 = fastq_text(600, 7)
    while at < len(fq3):                                                      # every block opens with a match exactly 32 KiB back
        toks = ([(258, 32768), (9, 32768)] if len(whole) >= 32768 else []) + lz_tokens(fq3, at, min(at + 6000, len(fq3)))
        whole += expand(toks, whole[-32768:])
        d.auto(toks, last=at + 6000 >= len(fq3)); at += 6000
    add("distance_32768_into_the_previous_unit", d, whole, bgzf=False)
    d = Deflate(); at = 0
    fq4 = fastq_text(300, 8)
    while at + 30000 < len(fq4):
        d.fixed(lz_tokens(fq4, at, at + 30000)) if (at // 30000) & 1 else d.stored(fq4[at:at + 30000]); at += 30000
    d.auto(lz_tokens(fq4, at), last=True)
    add("only_dynamic_block_is_the_final_one", d, fq4, bgzf=False)
    return out


def _invalid():
    """(name, deflate stream, the length its trailer claims)"""
    out = []
    toks = lz_tokens(fastq_text(4, 9))
    text = expand(toks)

    def add(name, d_or_body):
        body = d_or_body if isinstance(d_or_body, bytes) else d_or_body.getvalue()
        check_invalid(name, body)
        out.append((name, body, len(text)))

    lit_ok = [LITS[k % 15] for k in range(60)]
    over = lens(286, (list(LITS) + [256], 4), (257, 4), complete=False)      # seventeen four-bit codes
    d = Deflate(); d.dynamic(over, DIST_16, lit_ok[:50], last=True); add("oversubscribed_literal_lengths", d)
    d = Deflate(); d.dynamic(LIT_A, lens(30, (range(17), 4), complete=False), lit_ok[:50], last=True); add("oversubscribed_distance_lengths", d)
    d = Deflate(); d.dynamic(LIT_A, DIST_16, lit_ok[:50], last=True, rle="none", cl_lens=lens(19, ((0, 4, 5), 1), complete=False)); add("oversubscribed_code_length_lengths", d)
    d = Deflate(); d.dynamic(lens(286, (list(LITS[:6]) + [256], 3), complete=False), DIST_16, [65, 67, 71], last=True); add("incomplete_literal_set_of_seven_codes", d)
    d = Deflate(); d.dynamic(lens(286, ((65, 256), 2), complete=False), [0], [65, 65], last=True); add("incomplete_literal_set_of_two_codes", d)
    d = Deflate(); d.dynamic(LIT_A, DIST_16, lit_ok[:50], last=True, rle="none", cl_lens=lens(19, ((0, 4, 5), 2), complete=False)); add("incomplete_code_length_code", d)
    d = Deflate(); d.dynamic(lens(286, (list(LITS) + [257], 4)), [0], lit_ok[:50], last=True, end=False); add("no_code_for_symbol_256", d)
    d = Deflate(); d.dynamic(LIT_A, DIST_16, [], last=True, cl_items=[(16, 0, 0, 3)], cl_lens=lens(19, ((0, 16), 1)), end=False); add("repeat_code_16_as_the_first_length", d)
    seq = LIT_A[:265] + DIST_16[:16]
    items = code_length_runs(seq)
    assert items[-1][0] == 16 and items[-1][3] < 6
    items[-1] = (16, 3, items[-1][2], 6)                                       # the last run: six lengths where fewer are left
    d = Deflate(); d.dynamic(LIT_A, DIST_16, lit_ok[:50], last=True, cl_items=items); add("run_overruns_hlit_plus_hdist", d)
    d = Deflate(); d.dynamic(LIT_A, [0], lit_ok[:50], last=True, hlit=265, hdist=1, cl_items=code_length_runs(LIT_A[:265]) + [(18, 127, 265, 138)]); add("zero_run_of_138_overruns_hlit_plus_hdist", d)
    for hlit in (287, 288):
        d = Deflate(); d.dynamic(LIT_A + [0] * (hlit - 286), DIST_16, lit_ok[:50], last=True, hlit=hlit); add(f"hlit_{hlit}", d)
    for hdist in (31, 32):
        d = Deflate(); d.dynamic(LIT_A, DIST_16 + [0] * (hdist - 30), lit_ok[:50], last=True, hdist=hdist); add(f"hdist_{hdist}", d)
    d = Deflate(); d.dynamic(lens(257, (256, 1), complete=False), [0], [], last=True, cl_lens=lens(19, ((16, 17, 18, 0), 2)), hclen=4,
                             cl_items=[(18, 127, 0, 138), (18, 109, 138, 120)], end=False); add("hclen_4_leaves_no_end_code", d)
    d = Deflate(); d.stored(text[:100], last=True, nlen=(100 ^ 0xFFFF) ^ 0x0100); add("stored_len_and_nlen_disagree", d)
    d = Deflate(); d.header(True, 3); d.w.bits(0, 29); add("block_type_3", d)
    d = Deflate(); d.fixed(lit_ok[:40] + [Raw("lit", 257), Raw("dist", DIST_BASE.index(33), 8, 4)], last=True); add("distance_one_beyond_the_start", d)   # 41 back of 40
    for sym in (286, 287):
        d = Deflate(); d.fixed(lit_ok[:40] + [Raw("lit", sym)] + lit_ok[40:60], last=True); add(f"symbol_{sym}_in_a_fixed_block", d)
    for ds in (30, 31):
        d = Deflate(); d.fixed(lit_ok[:40] + [Raw("lit", 257), Raw("dist", ds, 0, 0)] + lit_ok[40:60], last=True); add(f"distance_code_{ds}_in_a_fixed_block", d)
    d = Deflate(); d.dynamic(LIT_A, [1], lit_ok[:40] + [Raw("lit", 257), Raw("bits", 1, 1)] + lit_ok[40:60], last=True); add("unused_bit_of_a_one_code_distance_alphabet", d)
    d = Deflate(); d.dynamic(lens(257, (256, 1), complete=False), [0], [Raw("bits", 1, 1)] + [Raw("bits", 0, 8)] * 4, last=True, end=False)
    add("unused_bit_of_a_one_code_literal_alphabet", d)
    d = Deflate(); d.auto(toks, last=True)
    whole = d.getvalue()
    add("truncated_inside_the_header", whole[:1])
    add("truncated_inside_the_code_length_list", whole[:(d.lengths_from + d.codes_from) // 16])
    d = Deflate(); d.fixed(lit_ok + [(200, 100)], last=True)                   # 3 + 8 * 60 bits, then 8 + 5 + 5 + 5 for the match: its last
    add("truncated_inside_a_match_s_extra_bits", d.getvalue()[:63])           # extra bits lie on both sides of bit 504
    return out


@functools.lru_cache(maxsize=None)
def valid_cases():
    return _valid()


@functools.lru_cache(maxsize=None)
def invalid_cases():
    return _invalid()


def bgzf_valid():
    """(name, text, BGZF file): the member between two of zlib's, so that what lies around it is somebody else's."""
    return [(name, text, bgzf_member(body, text) + EOF_MARK) for name, text, body, fits in valid_cases() if fits]


def good_member(k: int):
    text = fastq_text(30, 100 + k)
    d = Deflate(); d.auto(lz_tokens(text), last=True)
    return text, bgzf_member(d.getvalue(), text)


def bgzf_invalid():
    """(name, the good members' text, BGZF file, planted bad members): each bad member between two good ones."""
    (t0, m0), (t1, m1) = good_member(0), good_member(1)
    return [(name, t0 + t1, m0 + bgzf_member(body, b"", isize=claimed) + m1 + EOF_MARK, 1) for name, body, claimed in invalid_cases()]


def bgzf_all_valid_in_one_file():
    members = [(text, bgzf_member(body, text)) for _, text, body, fits in valid_cases() if fits and text]
    return b"".join(t for t, _ in members), b"".join(m for _, m in members) + EOF_MARK


def bgzf_all_invalid_in_one_file():
    good = [good_member(k) for k in range(len(invalid_cases()) + 1)]
    raw = good[0][1]
    for k, (_, body, claimed) in enumerate(invalid_cases()):
        raw += bgzf_member(body, b"", isize=claimed) + good[k + 1][1]
    return b"".join(t for t, _ in good), raw + EOF_MARK, len(invalid_cases())


def gzip_valid():
    """(name, text, gzip file): every valid stream as an ordinary gzip member."""
    return [(name, text, gzip_member(body, text)) for name, text, body, _ in valid_cases()]


GUESSING = ("stored_payload_that_looks_like_block_starts", "many_tiny_dynamic_blocks", "distance_32768_into_the_previous_unit", "only_dynamic_block_is_the_final_one")


def gzip_guessing():
    """The cases that are about guessed unit starts (a few hundred KB each)."""
    return [c for c in gzip_valid() if c[0] in GUESSING]


def gzip_invalid():
    """(name, gzip file): a truncated stream is a file that ends there, without a trailer."""
    return [(name, gzip_member(body, b"\0" * claimed)[: None if not name.startswith("truncated") else 10 + len(body)]) for name, body, claimed in invalid_cases()]


def random_lengths(rnd, n_symbols, max_len, must_have=()):
    """A Kraft-complete set: leaves split at random until n_symbols are there or none can be split; symbols drawn at random
    (must_have among them)."""
    leaves = [1, 1]
    want = rnd.randrange(max(2, len(must_have)), n_symbols + 1)
    while len(leaves) < want:
        can = [k for k, l in enumerate(leaves) if l < max_len]
        if not can:
            break
        k = rnd.choice(can)
        leaves[k] += 1
        leaves.append(leaves[k])
    symbols = list(must_have) + rnd.sample([s for s in range(n_symbols) if s not in must_have], len(leaves) - len(must_have))
    rnd.shuffle(leaves)
    out = [0] * n_symbols
    for s, l in zip(symbols, leaves):
        out[s] = l
    assert kraft(out) == 32768
    return out


def random_cases(seed: int, trials: int):
    """(text, BGZF file) pairs: both codes drawn with a longest code of 7 to 15 bits, tokens drawn for them, the header written
    in one of the ways above — one, two or three blocks a member."""
    rnd = random.Random(seed)
    for _ in range(trials):
        d = Deflate(); text = b""
        blocks = rnd.randrange(1, 4)
        for b in range(blocks):
            lit_lens = random_lengths(rnd, 286, rnd.randrange(7, 16), must_have=(256, rnd.randrange(256)))
            dist_lens = random_lengths(rnd, 30, rnd.randrange(7, 16))
            kw = {}
            how = rnd.randrange(5)
            if how == 0: kw["rle"] = "none"
            if how == 1: kw["hlit"], kw["hdist"] = 286, 30
            if how == 2: kw["hclen"] = 19
            if how == 3 and len(text) < 30000:                               # a stored block first: the codes start at a byte boundary
                piece = bytes(rnd.choice(LITS) for _ in range(rnd.randrange(0, 300)))
                d.stored(piece); text += piece
            toks = random_tokens(rnd, lit_lens, dist_lens, rnd.randrange(1, 1500), have=len(text), room=60000)
            d.dynamic(lit_lens, dist_lens, toks, last=b == blocks - 1, **kw)
            text += expand(toks, text)
        body = d.getvalue()
        check_valid(f"random {seed}", body, text)
        if text:
            yield text, bgzf_member(body, text) + EOF_MARK


def fastq_in_handmade_members(text: bytes, size=40000) -> bytes:
    """A BGZF file of `text` whose members take turns through the shapes above (for a whole run of the program)."""
    only_end = lens(257, (256, 1), complete=False)
    raw = b""
    for k, at in enumerate(range(0, len(text), size)):
        piece = text[at:at + size]
        toks = lz_tokens(piece)
        d = Deflate()
        how = k % 6
        if how == 0:                                                            # the one-code alphabet, then stored bytes
            d.dynamic(only_end, [0], []); d.stored(piece, last=True)
        elif how == 1:
            for _ in range(3):
                d.dynamic(only_end, [0], [])
            d.auto(toks, last=True)
        elif how == 2:
            d.fixed(toks); d.stored(b""); d.stored(b"", last=True)
        elif how == 3:
            d.auto(toks, last=True, rle="none", hlit=286, hdist=30, hclen=19)
        elif how == 4:                                                          # stored, dynamic, fixed: matches reach back across the boundaries
            a, b = len(piece) // 3, 2 * len(piece) // 3
            d.stored(piece[:a]); d.auto(lz_tokens(piece, a, b)); d.fixed(lz_tokens(piece, b), last=True)
        else:
            for _ in range(200):
                d.fixed([])
            d.auto(toks, last=True)
        check_valid(f"member {k}", d.getvalue(), piece)
        raw += bgzf_member(d.getvalue(), piece)
    return raw + EOF_MARK
