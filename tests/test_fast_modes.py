"""The FQD_FAST_* switches as one value (fastq-dupaway_amd/host/fast_modes.hpp: FastModes) on the CPU, in a harness built
with the sanitizers (tests/native/fast_modes_check.cpp): what each spelling sets, what a bad value says, which of two bad
settings is reported, the derived predicates, how the messages name the switches, every refusal decided before a GPU call,
and the out-of-memory note.  Every expected string is written out here.  The runs that these values steer:
tests/test_fast_*_cli.py."""
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
SRC = [HERE / "native" / "fast_modes_check.cpp", ROOT / "fastq-dupaway_amd" / "host" / "fast_modes.cpp"]
EXE = HERE / "native" / "fast_modes_check"


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "include"), "-o", str(EXE)] + [str(s) for s in SRC], check=True, capture_output=True)
    return str(EXE)


def ask(harness, cases):
    """cases: (env, unordered, devices, format) each; unordered None: from_env() alone, no check().  One answer a case."""
    text = "".join("\t".join(["-" if u is None else str(int(u)), str(d), f] + [f"{k}={v}" for k, v in env.items()]) + "\n" for env, u, d, f in cases)
    r = subprocess.run([harness], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = [line.split("\t") for line in r.stdout.split("\n")[:-1]]
    assert len(got) == len(cases)
    return got


def one(harness, env, unordered=False, devices=0, fmt="fastq"):
    return ask(harness, [(env, unordered, devices, fmt)])[0]


def fields(answer):
    assert answer[0] == "ok", answer
    names = "keep_best clusters both_strands umi umi_mismatch size_out levels sort_by_size min_size max_size size_in".split()
    return dict(zip(names, map(int, answer[1].split())))


def predicates(answer):
    assert answer[0] == "ok", answer
    return dict(zip("size_filter sized linked any".split(), map(int, answer[2].split())))


UNSET = dict(keep_best=0, clusters=0, both_strands=0, umi=0, umi_mismatch=0, size_out=0, levels=0, sort_by_size=0, min_size=1, max_size=0, size_in=0)
LINKS = "up to 37 bytes a record for the links, the owners and their grouping do not fit in GPU memory"
NOTE_PLAIN = "the text, the record arrays and " + LINKS
NOTE_STRAND = ("the text, the record arrays, the canonical reads (the sequence bytes once more, 12 bytes a record and mate, 1 byte a record) and, with FQD_FAST_KEEP / "
               "FQD_FAST_CLUSTERS, " + LINKS)
NOTE_UMI = ("the text, the record arrays, the keyed bytes of FQD_FAST_UMI (mate 1's sequence bytes once more and the UMI bases of every record, 16 bytes a record) and, with "
            "FQD_FAST_KEEP / FQD_FAST_CLUSTERS, " + LINKS)
NOTE_UMI_STRAND = ("the text, the record arrays, the keyed bytes of FQD_FAST_UMI (mate 1's sequence bytes once more and the UMI bases of every record, 16 bytes a record), the "
                   "canonical reads (the sequence bytes once more, 12 bytes a record and mate, 1 byte a record) and, with FQD_FAST_KEEP / FQD_FAST_CLUSTERS, " + LINKS)
NOTE_SIZEOUT = "; the cluster sizes of FQD_FAST_SIZEOUT take 4 bytes a record more and the labels' places and grown sizes 8 bytes a record and file"


def test_nothing_set_is_nothing(harness):
    a = one(harness, {})
    assert fields(a) == UNSET and predicates(a) == dict(size_filter=0, sized=0, linked=0, any=0)
    assert a[3] == "" and a[4] == NOTE_PLAIN
    # the same whatever the command line says: no switch, no refusal
    assert one(harness, {}, unordered=True, devices=4, fmt="fasta")[1:] == a[1:]


SPELLINGS = [("FQD_FAST_KEEP", "first", {}), ("FQD_FAST_KEEP", "best", dict(keep_best=1)),
             ("FQD_FAST_STRAND", "given", {}), ("FQD_FAST_STRAND", "both", dict(both_strands=1)),
             ("FQD_FAST_UMI", "off", {}), ("FQD_FAST_UMI", "colon", dict(umi=ord(":"))), ("FQD_FAST_UMI", "underscore", dict(umi=ord("_"))),
             ("FQD_FAST_UMI_MISMATCH", "0", {}), ("FQD_FAST_UMI_MISMATCH", "1", dict(umi_mismatch=1)), ("FQD_FAST_UMI_MISMATCH", "2", dict(umi_mismatch=2)),
             ("FQD_FAST_SORT", "input", {}), ("FQD_FAST_SORT", "size", dict(sort_by_size=1)),
             ("FQD_FAST_CLUSTERS", "1", dict(clusters=1)), ("FQD_FAST_CLUSTERS", "0", {}), ("FQD_FAST_CLUSTERS", "", {}), ("FQD_FAST_CLUSTERS", "yes", {}), ("FQD_FAST_CLUSTERS", "2", dict(clusters=1)),
             ("FQD_FAST_SIZEOUT", "1", dict(size_out=1)), ("FQD_FAST_SIZEOUT", "0", {}),
             ("FQD_FAST_LEVELS", "1", dict(levels=1)), ("FQD_FAST_LEVELS", "0", {}),
             ("FQD_FAST_SIZEIN", "1", dict(size_in=1)), ("FQD_FAST_SIZEIN", "0", {})]


def test_every_accepted_spelling(harness):
    got = ask(harness, [({name: value}, None, 0, "fastq") for name, value, _ in SPELLINGS])
    for (name, value, sets), a in zip(SPELLINGS, got):
        assert fields(a) == {**UNSET, **sets}, (name, value)


# the values that the runs refuse before any GPU call: tests/test_fast_keep_cli.py, test_fast_strand_cli.py, test_fast_umi_cli.py,
# test_fast_umi_merge_cli.py (value lists) and test_fast_sort_cli.py (BAD_VALUES)
BAD_VALUES = ([("FQD_FAST_KEEP", v, "FQD_FAST_KEEP must be 'first' or 'best', not '%s'") for v in ["bogus", "", "BEST", "best ", "1"]] +
              [("FQD_FAST_STRAND", v, "FQD_FAST_STRAND must be 'given' or 'both', not '%s'") for v in ["sideways", "", "BOTH", "both ", "1"]] +
              [("FQD_FAST_UMI", v, "FQD_FAST_UMI must be 'off', 'colon' or 'underscore', not '%s'") for v in ["comma", "", "COLON", "colon ", "1", ":"]] +
              [("FQD_FAST_UMI_MISMATCH", v, "FQD_FAST_UMI_MISMATCH must be 0, 1 or 2, not '%s'") for v in ["3", "-1", "", "one", "1 ", "01", "2.0"]] +
              [("FQD_FAST_SORT", v, "FQD_FAST_SORT must be 'input' or 'size', not '%s'") for v in ["abundance", ""]] +
              [("FQD_FAST_MINSIZE", v, "FQD_FAST_MINSIZE must be a decimal integer in 1 .. 2147483647, not '%s'") for v in ["0", "-1", "2x", "2147483648", ""]] +
              [("FQD_FAST_MAXSIZE", v, "FQD_FAST_MAXSIZE must be a decimal integer in 1 .. 2147483647, not '%s'") for v in ["0", "+3", "99999999999"]])


def test_every_bad_value_names_its_variable(harness):
    got = ask(harness, [({name: value}, False, 0, "fastq") for name, value, _ in BAD_VALUES])
    for (name, value, message), a in zip(BAD_VALUES, got):
        assert a == ["value", message % value], (name, value)
        assert a[1].count(name) == 1
    assert one(harness, {"FQD_FAST_MAXSIZE": "1", "FQD_FAST_MINSIZE": "2"}) == ["refusal", "FQD_FAST_MAXSIZE=1 is below FQD_FAST_MINSIZE=2: no cluster could be written"]


@pytest.mark.parametrize("name,unset", [("FQD_FAST_MINSIZE", 1), ("FQD_FAST_MAXSIZE", 0)])
def test_the_bounds_of_a_size_bound(harness, name, unset):
    field = "min_size" if name == "FQD_FAST_MINSIZE" else "max_size"
    good = ["1", "2", "0000000002", "2147483647"]
    for value, a in zip(good, ask(harness, [({name: value}, False, 0, "fastq") for value in good])):
        assert fields(a) == {**UNSET, field: int(value)}, value
    bad = ["0", "2147483648", "9999999999", "99999999999", "00000000002", "+3", "-1", "2x", " 2", ""]
    for value, a in zip(bad, ask(harness, [({name: value}, False, 0, "fastq") for value in bad])):
        assert a == ["value", f"{name} must be a decimal integer in 1 .. 2147483647, not '{value}'"], value
    assert unset == UNSET[field]


ALL_ON = {"FQD_FAST_KEEP": "best", "FQD_FAST_CLUSTERS": "1", "FQD_FAST_STRAND": "both", "FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "2", "FQD_FAST_SIZEOUT": "1",
          "FQD_FAST_LEVELS": "1", "FQD_FAST_SORT": "size", "FQD_FAST_MINSIZE": "2", "FQD_FAST_MAXSIZE": "9", "FQD_FAST_SIZEIN": "1"}
ALL_NAMES = ("FQD_FAST_KEEP=best and FQD_FAST_CLUSTERS=1 and FQD_FAST_STRAND=both and FQD_FAST_UMI=colon and FQD_FAST_UMI_MISMATCH=2 and FQD_FAST_SIZEOUT=1 and "
             "FQD_FAST_LEVELS=1 and FQD_FAST_SORT=size and FQD_FAST_SIZEIN=1 and FQD_FAST_MINSIZE=2 and FQD_FAST_MAXSIZE=9")


def test_the_names(harness):
    a = one(harness, ALL_ON)
    assert fields(a) == dict(keep_best=1, clusters=1, both_strands=1, umi=ord(":"), umi_mismatch=2, size_out=1, levels=1, sort_by_size=1, min_size=2, max_size=9, size_in=1)
    assert a[3] == ALL_NAMES
    # the order is the names' own, not the environment's
    assert one(harness, dict(reversed(list(ALL_ON.items()))))[3] == ALL_NAMES
    a = one(harness, {"FQD_FAST_MINSIZE": "1"})
    assert fields(a) == UNSET and predicates(a) == dict(size_filter=0, sized=0, linked=0, any=0) and a[3] == ""
    assert one(harness, {"FQD_FAST_MAXSIZE": "1"})[3] == "FQD_FAST_MAXSIZE=1"
    assert one(harness, {"FQD_FAST_UMI": "underscore", "FQD_FAST_UMI_MISMATCH": "1"})[3] == "FQD_FAST_UMI=underscore and FQD_FAST_UMI_MISMATCH=1"
    assert one(harness, {"FQD_FAST_STRAND": "both", "FQD_FAST_MINSIZE": "2147483647"})[3] == "FQD_FAST_STRAND=both and FQD_FAST_MINSIZE=2147483647"


#                  switch alone                        size_filter sized linked any
TRUTH = [({"FQD_FAST_KEEP": "best"}, (0, 0, 1, 1)), ({"FQD_FAST_CLUSTERS": "1"}, (0, 0, 1, 1)), ({"FQD_FAST_STRAND": "both"}, (0, 0, 0, 1)),
         ({"FQD_FAST_UMI": "colon"}, (0, 0, 0, 1)), ({"FQD_FAST_UMI": "underscore"}, (0, 0, 0, 1)), ({"FQD_FAST_UMI_MISMATCH": "1"}, (0, 0, 1, 1)),
         ({"FQD_FAST_UMI_MISMATCH": "2"}, (0, 0, 1, 1)), ({"FQD_FAST_SIZEOUT": "1"}, (0, 1, 1, 1)), ({"FQD_FAST_LEVELS": "1"}, (0, 1, 1, 1)),
         ({"FQD_FAST_SORT": "size"}, (0, 1, 1, 1)), ({"FQD_FAST_MINSIZE": "2"}, (1, 1, 1, 1)), ({"FQD_FAST_MAXSIZE": "5"}, (1, 1, 1, 1)),
         ({"FQD_FAST_MAXSIZE": "1"}, (1, 1, 1, 1)), ({"FQD_FAST_SIZEIN": "1"}, (0, 0, 0, 0))]


def test_the_predicates_of_each_switch_alone(harness):
    got = ask(harness, [(env, None, 0, "fastq") for env, _ in TRUTH])
    for (env, (size_filter, sized, linked, any_)), a in zip(TRUTH, got):
        assert predicates(a) == dict(size_filter=size_filter, sized=sized, linked=linked, any=any_), env


SIZEIN_ALONE = ("FQD_FAST_SIZEIN=1 changes what a cluster's size is and nothing else: set one of FQD_FAST_SIZEOUT=1, FQD_FAST_LEVELS=1, FQD_FAST_SORT=size, FQD_FAST_MINSIZE "
                "(above 1) or FQD_FAST_MAXSIZE as well, which read the sizes")
FASTA = "FQD_FAST_KEEP=best needs the quality lines of FASTQ records: --format fasta has none"


def mismatch_alone(d):
    return f"FQD_FAST_UMI_MISMATCH={d} merges the UMIs that FQD_FAST_UMI finds: set FQD_FAST_UMI=colon or FQD_FAST_UMI=underscore as well"


def test_every_refusal_of_the_check(harness):
    assert one(harness, {"FQD_FAST_SIZEIN": "1"}) == ["refusal", SIZEIN_ALONE]
    assert one(harness, {"FQD_FAST_SIZEIN": "1", "FQD_FAST_KEEP": "best", "FQD_FAST_UMI": "colon", "FQD_FAST_MINSIZE": "1"}) == ["refusal", SIZEIN_ALONE]
    for reader in ({"FQD_FAST_SIZEOUT": "1"}, {"FQD_FAST_LEVELS": "1"}, {"FQD_FAST_SORT": "size"}, {"FQD_FAST_MINSIZE": "2"}, {"FQD_FAST_MAXSIZE": "1"}):
        assert one(harness, {"FQD_FAST_SIZEIN": "1", **reader})[0] == "ok"
    for d in (1, 2):
        assert one(harness, {"FQD_FAST_UMI_MISMATCH": str(d)}) == ["refusal", mismatch_alone(d)]
        assert one(harness, {"FQD_FAST_UMI_MISMATCH": str(d), "FQD_FAST_UMI": "off"}) == ["refusal", mismatch_alone(d)]
    env = {"FQD_FAST_CLUSTERS": "1", "FQD_FAST_UMI": "colon"}
    assert one(harness, env, unordered=True) == ["refusal", "FQD_FAST_CLUSTERS=1 and FQD_FAST_UMI=colon with --unordered: these modes run on ordered inputs only"]
    assert one(harness, env, devices=2) == ["refusal", "FQD_FAST_CLUSTERS=1 and FQD_FAST_UMI=colon runs on one GPU: FQD_DEVICES may name one device only"]
    assert one(harness, env, devices=1)[0] == "ok" and one(harness, env, devices=0)[0] == "ok"
    assert one(harness, {"FQD_FAST_KEEP": "best"}, fmt="fasta") == ["refusal", FASTA]
    assert one(harness, {"FQD_FAST_KEEP": "first", "FQD_FAST_CLUSTERS": "1"}, fmt="fasta")[0] == "ok"     # FASTA is allowed to every other switch
    assert one(harness, ALL_ON, fmt="fasta") == ["refusal", FASTA]


def bad_value(name, must_be, value="?"):
    return ["value", f"{name} must be {must_be}, not '{value}'"]


A_NUMBER = "a decimal integer in 1 .. 2147483647"
BELOW = ["refusal", "FQD_FAST_MAXSIZE=1 is below FQD_FAST_MINSIZE=2: no cluster could be written"]
# Two bad settings at a time, adjacent in the order in which they are reported: the earlier one is.  (A MAXSIZE below MINSIZE
# needs both bounds well-formed, so it stands beside a bad FQD_FAST_SORT in place of a bad bound.)
PRECEDENCE = [
    ({"FQD_FAST_KEEP": "?", "FQD_FAST_SORT": "?"}, {}, bad_value("FQD_FAST_KEEP", "'first' or 'best'")),
    ({"FQD_FAST_SORT": "?", "FQD_FAST_MINSIZE": "?"}, {}, bad_value("FQD_FAST_SORT", "'input' or 'size'")),
    ({"FQD_FAST_MINSIZE": "?", "FQD_FAST_MAXSIZE": "?"}, {}, bad_value("FQD_FAST_MINSIZE", A_NUMBER)),
    ({"FQD_FAST_MAXSIZE": "?", "FQD_FAST_STRAND": "?"}, {}, bad_value("FQD_FAST_MAXSIZE", A_NUMBER)),
    ({"FQD_FAST_SORT": "?", "FQD_FAST_MINSIZE": "2", "FQD_FAST_MAXSIZE": "1"}, {}, bad_value("FQD_FAST_SORT", "'input' or 'size'")),
    ({"FQD_FAST_MINSIZE": "2", "FQD_FAST_MAXSIZE": "1", "FQD_FAST_STRAND": "?"}, {}, BELOW),
    ({"FQD_FAST_STRAND": "?", "FQD_FAST_UMI": "?"}, {}, bad_value("FQD_FAST_STRAND", "'given' or 'both'")),
    ({"FQD_FAST_UMI": "?", "FQD_FAST_UMI_MISMATCH": "?"}, {}, bad_value("FQD_FAST_UMI", "'off', 'colon' or 'underscore'")),
    ({"FQD_FAST_UMI_MISMATCH": "?", "FQD_FAST_SIZEIN": "1"}, {}, bad_value("FQD_FAST_UMI_MISMATCH", "0, 1 or 2")),
    ({"FQD_FAST_SIZEIN": "1", "FQD_FAST_UMI_MISMATCH": "1"}, {}, ["refusal", SIZEIN_ALONE]),
    ({"FQD_FAST_UMI_MISMATCH": "1", "FQD_FAST_KEEP": "best"}, dict(unordered=True), ["refusal", mismatch_alone(1)]),
    ({"FQD_FAST_KEEP": "best"}, dict(unordered=True, devices=2), ["refusal", "FQD_FAST_KEEP=best with --unordered: these modes run on ordered inputs only"]),
    ({"FQD_FAST_KEEP": "best"}, dict(devices=2, fmt="fasta"), ["refusal", "FQD_FAST_KEEP=best runs on one GPU: FQD_DEVICES may name one device only"]),
    # and the two ends of the order against each other
    ({"FQD_FAST_KEEP": "?"}, dict(unordered=True, devices=2, fmt="fasta"), bad_value("FQD_FAST_KEEP", "'first' or 'best'")),
    ({"FQD_FAST_KEEP": "best", "FQD_FAST_CLUSTERS": "?", "FQD_FAST_SIZEOUT": "?", "FQD_FAST_LEVELS": "?"}, dict(fmt="fasta"), ["refusal", FASTA]),
]


def test_which_of_two_bad_settings_is_reported(harness):
    got = ask(harness, [(env, line.get("unordered", False), line.get("devices", 0), line.get("fmt", "fastq")) for env, line, _ in PRECEDENCE])
    for (env, line, expect), a in zip(PRECEDENCE, got):
        assert a == expect, (env, line)


NOTES = [({}, NOTE_PLAIN),
         ({"FQD_FAST_STRAND": "both"}, NOTE_STRAND),
         ({"FQD_FAST_UMI": "colon"}, NOTE_UMI),
         ({"FQD_FAST_UMI": "underscore", "FQD_FAST_STRAND": "both"}, NOTE_UMI_STRAND),
         ({"FQD_FAST_SIZEOUT": "1", "FQD_FAST_SIZEIN": "1"},
          NOTE_PLAIN + NOTE_SIZEOUT + "; FQD_FAST_SIZEIN takes 4 bytes a record for the weights while the sizes are made and 4 bytes a record and file for the annotations' "
          "lengths in the writer"),
         ({"FQD_FAST_SORT": "size", "FQD_FAST_SIZEOUT": "1"},
          NOTE_PLAIN + NOTE_SIZEOUT + "; FQD_FAST_SORT=size takes 4 bytes a cluster for the written order, 1 byte a cluster for its flags and, while it sorts, 24 bytes a cluster "
          "of scratch (the scratch of the grouping serves where it is as large), and the labels' places and the sizes in written order 4 bytes a cluster and file and 4 bytes a "
          "cluster"),
         ({"FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1"},
          NOTE_UMI + "; FQD_FAST_UMI_MISMATCH takes 12 bytes a record more (the owners by sequence, the exact counts, the merged owners) and, while it merges, 4 bytes a record "
          "and up to 66 bytes an exact cluster"),
         # the sizes are named after the first switch that reads them; SIZEIN without SIZEOUT adds the weights alone
         ({"FQD_FAST_LEVELS": "1", "FQD_FAST_SORT": "size"},
          NOTE_PLAIN + "; the cluster sizes of FQD_FAST_LEVELS take 4 bytes a record more; FQD_FAST_SORT=size takes 4 bytes a cluster for the written order, 1 byte a cluster for "
          "its flags and, while it sorts, 24 bytes a cluster of scratch (the scratch of the grouping serves where it is as large)"),
         ({"FQD_FAST_MAXSIZE": "3", "FQD_FAST_SIZEIN": "1"},
          NOTE_PLAIN + "; the cluster sizes of FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE take 4 bytes a record more; FQD_FAST_SIZEIN takes 4 bytes a record for the weights while the "
          "sizes are made")]


def test_the_out_of_memory_note(harness):
    got = ask(harness, [(env, False, 0, "fastq") for env, _ in NOTES])
    for (env, note), a in zip(NOTES, got):
        assert a[0] == "ok" and a[4] == note, env
