"""The edge list of FQD_FAST_UMI, shared by tests/test_umi_core.py (the core header on the CPU) and tests/test_gpu_umi.py
(fqd_umi_find, fqd_umi_reads).  ID lines are bytes; every case is named.  A case is judged on its own (as record 0 of a
run); what it means to differ from record 0's shape is the files of shape_files()."""
import random

import umi_reference as ref

COLON, UNDERSCORE = b":", b"_"
WORD_END_AT = [15, 16, 17, 255, 256, 257, 600]                 # 600: more than one round of sixteen chunks
UMI_BASES = [1, 15, 16, 17, 64]


def random_umi(rng, L, alphabet="ACGTN"):
    return "".join(rng.choice(alphabet) for _ in range(L)).encode()


def id_line(rng, end_at, umi, sep, ending=b" 1:N:0:ATCACG+TT_A\n", lead=b"@"):
    """An ID line whose first word ends at byte end_at (there stands the first byte of `ending`) and carries `umi` behind
    its last `sep`.  The filler in front holds earlier separators of both kinds; so does the comment."""
    room = end_at - 1 - len(sep) - len(umi)
    assert room >= 0, (end_at, umi)
    filler = "".join(rng.choice("A0:1_FCx:") for _ in range(room)).encode()
    line = lead + filler + sep + umi + ending
    assert len(lead) == 1 and line[end_at:end_at + 1] == ending[:1]
    return line


def taken_cases():
    """[(name, line, sep)] of lines the rule takes."""
    rng = random.Random(41)
    out = []
    for sep in (COLON, UNDERSCORE):
        tag = "colon" if sep == COLON else "underscore"
        for end_at in list(range(3, 40)) + WORD_END_AT + [511, 512, 513]:
            for ending in (b" x:y_z\n", b"\n", b"\t1:N:0:ACGT\n", b"\r\n"):
                L = min(end_at - 2, rng.choice([1, 4, 8, 12]))
                out.append((f"{tag}, word end at {end_at}, ending {ending[:1]!r}", id_line(rng, end_at, random_umi(rng, L), sep, ending), sep))
        for lb in UMI_BASES:
            for end_at in (lb + 2, lb + 30, 300):
                out.append((f"{tag}, {lb} bases, word end at {end_at}", id_line(rng, end_at, random_umi(rng, lb), sep), sep))
        # U across a 16-byte and a 256-byte boundary of the line
        for end_at, L in ((20, 8), (33, 20), (260, 8), (270, 30), (520, 64), (300, 64)):
            out.append((f"{tag}, U of {L} ends at {end_at}", id_line(rng, end_at, random_umi(rng, L), sep), sep))
        for umi in (b"ACGT+TGCA", b"ACGT-TGCA", b"A+C", b"AC+GT+TG", b"AC+GT-TG", b"+A", b"A+", b"N", b"NNNN+NNNN", b"A" * 63 + b"+",
                    b"+" + b"C" * 63, b"ACGTACGTACGTACG+ACGTACGTACGTACGT", b"ACGTACGTACGTACGT+ACGTACGTACGTACGT"):
            out.append((f"{tag}, {umi.decode()}", id_line(rng, len(umi) + 12, umi, sep), sep))
        out.append((f"{tag}, no word end in the line", b"@A00:7" + sep + b"ACGT", sep))
        out.append((f"{tag}, no word end in a long line", b"@" + b"x" * 290 + sep + b"ACGTAC", sep))
        out.append((f"{tag}, fasta", id_line(rng, 24, b"ACGTNN", sep, lead=b">"), sep))
        out.append((f"{tag}, a blank at the line's first byte", b" A" + sep + b"ACGT\n", sep))
        out.append((f"{tag}, the shortest", b"@" + sep + b"A\n", sep))
        out.append((f"{tag}, the shortest without an end", b"@" + sep + b"A", sep))
    out.append(("colon, underscore joins", id_line(rng, 30, b"ACGT_TGCA", COLON), COLON))
    out.append(("colon, bcl-convert", b"@A00:1:FC:1:1101:1000:2000:ACGTACGT 1:N:0:ATCACG\n", COLON))
    out.append(("underscore, umi_tools", b"@READ_ACGTACGT\n", UNDERSCORE))
    out.append(("underscore, colons in the word", b"@A00:1:FC_ACGTACGT 1:N:0:ATCACG\n", UNDERSCORE))
    return out


def refused_cases():
    """[(name, line, sep, reason)] of lines the rule refuses on their own."""
    rng = random.Random(42)
    out = []
    for sep in (COLON, UNDERSCORE):
        o = b"_" if sep == COLON else b":"
        tag = "colon" if sep == COLON else "underscore"
        out += [(f"{tag}, two bytes", b"@\n", sep, ref.NO_SEPARATOR),
                (f"{tag}, one byte", b"@", sep, ref.NO_SEPARATOR),
                (f"{tag}, no byte", b"", sep, ref.NO_SEPARATOR),
                (f"{tag}, the separator is the line's first byte", sep + b"ACGT\n", sep, ref.NO_SEPARATOR),
                (f"{tag}, the word is empty", b"@ x" + sep + b"ACGT\n", sep, ref.NO_SEPARATOR),
                (f"{tag}, a separator in the comment only", b"@READ1 1" + sep + b"N" + sep + b"ACGT\n", sep, ref.NO_SEPARATOR),
                (f"{tag}, a separator behind a tab only", b"@READ1\tx" + sep + b"ACGT\n", sep, ref.NO_SEPARATOR),
                (f"{tag}, a separator behind the word end of a long line", b"@" + b"R" * 300 + b" " + sep + b"ACGT\n", sep, ref.NO_SEPARATOR),
                (f"{tag}, the other separator only", b"@A00" + o + b"ACGT\n", sep, ref.NO_SEPARATOR),
                (f"{tag}, the separator is the word's last byte", b"@A00" + sep + b"1" + sep + b" ACGT\n", sep, ref.EMPTY),
                (f"{tag}, the separator is the line's last byte but one", b"@A00" + sep + b"\n", sep, ref.EMPTY),
                (f"{tag}, the separator is the line's last byte", b"@A00" + sep, sep, ref.EMPTY),
                (f"{tag}, the separator before a carriage return", b"@A00" + sep + b"\r\n", sep, ref.EMPTY),
                (f"{tag}, 65 bases", id_line(rng, 80, random_umi(rng, 65), sep), sep, ref.TOO_LONG),
                (f"{tag}, 64 bases and a joiner", id_line(rng, 80, random_umi(rng, 32) + b"+" + random_umi(rng, 32), sep), sep, ref.TOO_LONG),
                (f"{tag}, 300 bytes", id_line(rng, 400, random_umi(rng, 300), sep), sep, ref.TOO_LONG),
                (f"{tag}, 65 bytes with a lower-case one", id_line(rng, 80, b"a" * 65, sep), sep, ref.TOO_LONG),
                (f"{tag}, a lower-case byte", id_line(rng, 30, b"ACgT", sep), sep, ref.BAD_BYTE),
                (f"{tag}, a lower-case byte at place 63", id_line(rng, 90, b"A" * 63 + b"t", sep), sep, ref.BAD_BYTE),
                (f"{tag}, a digit", id_line(rng, 30, b"1101", sep), sep, ref.BAD_BYTE),
                (f"{tag}, an R", id_line(rng, 30, b"ACRT", sep), sep, ref.BAD_BYTE),
                (f"{tag}, a byte above 127", id_line(rng, 30, b"AC\xc3T", sep), sep, ref.BAD_BYTE),
                (f"{tag}, joiners and a lower-case byte", id_line(rng, 30, b"+-x", sep), sep, ref.BAD_BYTE),
                (f"{tag}, a joiner alone", id_line(rng, 30, b"+", sep), sep, ref.NO_BASE),
                (f"{tag}, joiners alone", id_line(rng, 30, b"+-+", sep), sep, ref.NO_BASE),
                (f"{tag}, 64 joiners", id_line(rng, 90, b"+" * 64, sep), sep, ref.NO_BASE)]
    out.append(("colon, an underscore alone", id_line(rng, 30, b"_", COLON), COLON, ref.NO_BASE))
    return out


def random_lines(seed, count):
    """[(line, sep)]: bytes drawn from what matters to the rule, most lines short, some across rounds."""
    rng = random.Random(seed)
    alphabet = b"@>ACGTN+-_:: \t\r\nacx1"
    out = []
    for k in range(count):
        L = rng.choice([0, 1, 2, 3, 5, 8, 13, 15, 16, 17, 20, 31, 32, 33, 48, 70, 100, 255, 256, 257, 300, 520])
        body = bytes(rng.choice(alphabet[2:8] if rng.random() < 0.7 else alphabet) for _ in range(L))
        if L and rng.random() < 0.8:
            body = b"@" + body[1:]
        if L > 3 and rng.random() < 0.5:                       # a likely well-formed tail
            at = rng.randrange(1, L)
            body = body[:at] + rng.choice([b":", b"_"]) + body[at + 1:]
        out.append((body, rng.choice([COLON, UNDERSCORE])))
    return out


def shape_files():
    """[(name, id lines, sep)]: files whose records are fine one by one; what is refused is a shape that is not record
    0's — at record 1, at the last record, in two places (the lowest counts) — or record 0 itself."""
    rng = random.Random(43)

    def lines(umis, sep=COLON):
        return [id_line(rng, rng.choice([len(u) + 2, 25, 40, 270]) if len(u) < 20 else len(u) + 9, u, sep) for u in umis]

    same = [random_umi(rng, 8) for _ in range(70)]
    dual = [random_umi(rng, 4) + b"+" + random_umi(rng, 4) for _ in range(70)]
    out = [("all of one shape", lines(same), COLON), ("all dual", lines(dual), COLON), ("all dual, underscore", lines(dual, UNDERSCORE), UNDERSCORE)]
    for name, at, umi in (("a longer UMI at record 1", [1], b"ACGTACGTA"), ("a shorter UMI at the last record", [69], b"ACGTACG"),
                          ("a joiner at the last record", [69], b"ACG+ACGT"), ("two places", [40, 13], b"ACGT+CGT"),
                          ("a joiner moved at record 65", [65], None)):
        for base in (same, dual):
            umis = list(base)
            for a in at:
                umis[a] = umi if umi is not None else (b"ACG+TACG" if base is same else b"ACG+TACGT")
            out.append((f"{name}, {'dual' if base is dual else 'plain'}", lines(umis), COLON))
    bad0 = lines(same)
    bad0[0] = b"@READ 1:N:0\n"
    bad0[5] = b"@READ:acgt\n"
    out.append(("a bad record 0", bad0, COLON))
    bad_and_shape = lines(same)
    bad_and_shape[30] = id_line(rng, 30, b"ACGTACGTAC", COLON)       # shape
    bad_and_shape[20] = id_line(rng, 30, b"ACGTACGx", COLON)         # its own fault, lower
    out.append(("a bad byte below a differing shape", bad_and_shape, COLON))
    other = lines(same)
    other[7] = id_line(rng, 30, b"AC+TACGT", COLON)
    out.append(("a differing joiner place only", other, COLON))
    joiner_char = lines(dual)
    joiner_char[9] = id_line(rng, 30, b"ACGT-ACGT", COLON)               # another joiner at the same place: the same shape
    out.append(("another joiner character at the same place", joiner_char, COLON))
    return out
