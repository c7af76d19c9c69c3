"""FastModes::prefix and FastModes::longest (fastq-dupaway_amd/host/fast_modes.cpp), the host's view of FQD_FAST_PREFIX=L and of
FQD_FAST_CENTROID=longest, in a small native harness (tests/native/fast_prefix_check.cpp, built with the sanitizers): the values,
the words of a bad value, the order in which the variables are read, the predicates, names(), the refusals' words and their
order, and the clauses of the out-of-memory note.  Every expected string is written out.  The run itself:
tests/test_fast_prefix_cli.py."""
import os
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
LONGEST = {"FQD_FAST_CENTROID": "longest"}
WITHOUT = ("FQD_FAST_CENTROID=longest chooses the sequence that all others of a merged cluster are prefixes of, and nothing else: set FQD_FAST_PREFIX as well, "
           "which merges them (FQD_FAST_CENTROID=abundant goes with the other merging switches)")


@pytest.fixture(scope="module")
def harness():
    target = HERE / "native" / "fast_prefix_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "include"), "-o", str(target), str(HERE / "native" / "fast_prefix_check.cpp"),
                    str(ROOT / "fastq-dupaway_amd" / "host" / "fast_modes.cpp")], check=True, capture_output=True)
    return str(target)


def modes(harness, env, *args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("FQD_")}
    e.update(env)
    r = subprocess.run([harness, *map(str, args)], capture_output=True, text=True, env=e, timeout=60)
    assert r.returncode == 0, r.stderr
    return dict(line.split(" ", 1) if " " in line else (line, "") for line in r.stdout.splitlines())


def prefix(value):
    return {"FQD_FAST_PREFIX": str(value)}


def test_unset_and_zero_are_off(harness):
    off = modes(harness, {})
    assert off == {"prefix": "0", "longest": "0", "centroid": "0", "merges": "0", "picks": "0", "linked": "0", "any": "0", "names": "", "name": "", "note": off["note"],
                   "check": "passed"}
    assert "PREFIX" not in off["note"] and "longest" not in off["note"]
    assert modes(harness, prefix(0)) == off
    env = {"FQD_FAST_KEEP": "best", "FQD_FAST_SIZEOUT": "1", "FQD_FAST_OPTICAL": "9"}
    assert modes(harness, {**env, **prefix(0)}) == modes(harness, env)


@pytest.mark.parametrize("value", [1, 2, 20, 32, 150, 65535])
def test_the_values_that_are_on(harness, value):
    on = modes(harness, prefix(value))
    assert (on["prefix"], on["merges"], on["picks"], on["linked"], on["any"], on["names"], on["name"], on["check"]) == \
           (str(value), "1", "0", "1", "1", f"FQD_FAST_PREFIX={value}", f"FQD_FAST_PREFIX={value}", "passed")
    assert modes(harness, prefix(value), 0, 1, 1)["check"] == "passed"      # FASTA is allowed


@pytest.mark.parametrize("value", ["", "x", "-1", "01", "1 ", "+1", "65536", "00", "1.0", "4294967297", "123456"])
def test_a_bad_value(harness, value):
    assert modes(harness, prefix(value)) == {"error": f"FQD_FAST_PREFIX must be a decimal integer in 1 .. 65535 (or 0 for off), not '{value}'"}


def test_it_is_read_last(harness):
    for name, bad, words in [("FQD_FAST_KEEP", "x", "FQD_FAST_KEEP must be 'first' or 'best', not 'x'"),
                             ("FQD_FAST_OPTICAL", "x", "FQD_FAST_OPTICAL must be a decimal integer in 1 .. 2147483647, not 'x'"),
                             ("FQD_FAST_HAMMING", "9", "FQD_FAST_HAMMING must be 0, 1, 2 or 3, not '9'"),
                             ("FQD_FAST_UMI_HAMMING", "9", "FQD_FAST_UMI_HAMMING must be 0, 1, 2 or 3, not '9'"),
                             ("FQD_FAST_CENTROID", "x", "FQD_FAST_CENTROID must be 'first' or 'abundant', not 'x'")]:
        assert modes(harness, {"FQD_FAST_PREFIX": "x", name: bad}) == {"error": words}, name
    got = modes(harness, {"FQD_FAST_PREFIX": "x", "FQD_FAST_CENTROID": "longest", "FQD_FAST_CONSENSUS": "1", "FQD_FAST_KEEP": "best"})
    assert got == {"error": "FQD_FAST_PREFIX must be a decimal integer in 1 .. 65535 (or 0 for off), not 'x'"}


def test_its_place_among_the_names(harness):
    env = {"FQD_FAST_KEEP": "best", "FQD_FAST_CLUSTERS": "1", "FQD_FAST_OPTICAL": "100", "FQD_FAST_SIZEOUT": "1", "FQD_FAST_MINSIZE": "2", "FQD_FAST_MAXSIZE": "9",
           **prefix(24)}
    got = modes(harness, env)
    assert got["names"] == ("FQD_FAST_KEEP=best and FQD_FAST_CLUSTERS=1 and FQD_FAST_OPTICAL=100 and FQD_FAST_SIZEOUT=1 and FQD_FAST_MINSIZE=2 and FQD_FAST_MAXSIZE=9 "
                            "and FQD_FAST_PREFIX=24")
    assert got["check"] == "passed"
    got = modes(harness, {**env, **LONGEST})
    assert got["names"] == ("FQD_FAST_KEEP=best and FQD_FAST_CLUSTERS=1 and FQD_FAST_OPTICAL=100 and FQD_FAST_CENTROID=longest and FQD_FAST_SIZEOUT=1 and FQD_FAST_MINSIZE=2 "
                            "and FQD_FAST_MAXSIZE=9 and FQD_FAST_PREFIX=24")
    assert got["check"] == "passed"


def test_each_refusal_in_its_words(harness):
    got = modes(harness, {**prefix(20), "FQD_FAST_HAMMING": "2"})
    assert got["refusal"] == ("FQD_FAST_PREFIX=20 with FQD_FAST_HAMMING=2: a truncated copy with substituted bases inside the overlap is a rule of its own, and each of the "
                              "two switches merges by its own rule alone")
    assert "check" not in got
    got = modes(harness, {**prefix(20), "FQD_FAST_UMI": "colon"})
    assert got["refusal"] == ("FQD_FAST_PREFIX=20 with FQD_FAST_UMI=colon: which sequences under one UMI are copies of one molecule is a rule of its own, and this switch "
                              "merges by sequence alone")
    got = modes(harness, {**prefix(20), "FQD_FAST_UMI": "underscore", "FQD_FAST_UMI_MISMATCH": "1", "FQD_FAST_UMI_HAMMING": "2"})
    assert got["refusal"] == ("FQD_FAST_PREFIX=20 with FQD_FAST_UMI=underscore and FQD_FAST_UMI_MISMATCH=1 and FQD_FAST_UMI_HAMMING=2: which sequences under one UMI are "
                              "copies of one molecule is a rule of its own, and this switch merges by sequence alone")
    got = modes(harness, {**prefix(20), "FQD_FAST_STRAND": "both"})
    assert got["refusal"] == ("FQD_FAST_PREFIX=20 with FQD_FAST_STRAND=both: a truncated read's reverse complement is a suffix of its untrimmed copy's, not a prefix, so the "
                              "two would be keyed in orientations that are never compared")
    got = modes(harness, {**prefix(20), "FQD_FAST_CONSENSUS": "1"})
    assert got["refusal"] == ("FQD_FAST_PREFIX=20 with FQD_FAST_CONSENSUS=1: the members of a merged cluster differ in length, and a column-wise vote needs members of one "
                              "length")
    assert modes(harness, {**prefix(20), "FQD_FAST_STRAND": "given", "FQD_FAST_HAMMING": "0", "FQD_FAST_UMI": "off", "FQD_FAST_CONSENSUS": "0"})["check"] == "passed"


def test_the_order_of_the_refusals(harness):
    everything = {**prefix(20), "FQD_FAST_HAMMING": "1", "FQD_FAST_UMI": "colon", "FQD_FAST_STRAND": "both", "FQD_FAST_CONSENSUS": "1"}
    # every clause that was there before is said first, in the words it always had ...
    assert modes(harness, everything)["refusal"].startswith("FQD_FAST_HAMMING=1 with FQD_FAST_STRAND=both: ")
    assert modes(harness, {**prefix(20), "FQD_FAST_CONSENSUS": "1", "FQD_FAST_STRAND": "both"})["refusal"].startswith("FQD_FAST_CONSENSUS=1 with FQD_FAST_STRAND=both: ")
    assert modes(harness, {**prefix(20), "FQD_FAST_HAMMING": "1"}, 1)["refusal"] == "FQD_FAST_HAMMING=1 and FQD_FAST_PREFIX=20 with --unordered: these modes run on ordered inputs only"
    assert modes(harness, prefix(20), 0, 2)["refusal"] == "FQD_FAST_PREFIX=20 runs on one GPU: FQD_DEVICES may name one device only"
    assert modes(harness, {**prefix(20), "FQD_FAST_KEEP": "best"}, 0, 1, 1)["refusal"] == "FQD_FAST_KEEP=best needs the quality lines of FASTQ records: --format fasta has none"
    # ... then the new ones among themselves: HAMMING, UMI, STRAND, CONSENSUS, CENTROID=longest
    del everything["FQD_FAST_STRAND"]
    assert modes(harness, {**everything, "FQD_FAST_UMI": "off"})["refusal"].startswith("FQD_FAST_PREFIX=20 with FQD_FAST_HAMMING=1: ")
    assert modes(harness, {**prefix(20), "FQD_FAST_UMI": "colon", "FQD_FAST_CONSENSUS": "1"})["refusal"].startswith("FQD_FAST_PREFIX=20 with FQD_FAST_UMI=colon: ")
    assert modes(harness, {**prefix(20), "FQD_FAST_UMI": "colon", "FQD_FAST_STRAND": "both"})["refusal"].startswith("FQD_FAST_PREFIX=20 with FQD_FAST_UMI=colon: ")
    assert modes(harness, {**LONGEST, "FQD_FAST_CONSENSUS": "1"})["refusal"] == WITHOUT


def test_centroid_longest_with_and_without_it(harness):
    on = modes(harness, {**LONGEST, **prefix(32)})
    assert (on["prefix"], on["longest"], on["centroid"], on["merges"], on["picks"], on["linked"], on["any"], on["check"]) == ("32", "1", "0", "1", "1", "1", "1", "passed")
    assert on["names"] == "FQD_FAST_CENTROID=longest and FQD_FAST_PREFIX=32"
    assert modes(harness, {**LONGEST, **prefix(32), "FQD_FAST_KEEP": "best"})["check"] == "passed"
    assert modes(harness, {**LONGEST, **prefix(32)}, 0, 1, 1)["check"] == "passed"                     # FASTA is allowed
    got = modes(harness, LONGEST)
    assert got["refusal"] == WITHOUT and "check" not in got and (got["longest"], got["any"]) == ("1", "1")
    for env in ({"FQD_FAST_HAMMING": "1"}, {"FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1"}, {"FQD_FAST_KEEP": "best"}, prefix(0)):
        assert modes(harness, {**LONGEST, **env})["refusal"] == WITHOUT, env
    # abundant goes with FQD_FAST_PREFIX as with the other merges
    got = modes(harness, {"FQD_FAST_CENTROID": "abundant", **prefix(32)})
    assert (got["centroid"], got["longest"], got["picks"], got["check"]) == ("1", "0", "1", "passed")
    assert got["names"] == "FQD_FAST_CENTROID=abundant and FQD_FAST_PREFIX=32"


@pytest.mark.parametrize("value", [1, 32, 65535])
def test_the_clauses_of_the_memory_note(harness, value):
    off = modes(harness, {})["note"]
    clause = (f"; FQD_FAST_PREFIX takes 4 bytes a record for the merged owners and, while it merges, 24 bytes an exact cluster for the seeds and their sort (12 bytes a "
              f"seed, one seed a cluster of at least {value} bases a mate, twice over), 8 bytes a record for the parents and 4 bytes a record for the roots")
    assert modes(harness, prefix(value))["note"] == off + clause
    longest = ("; FQD_FAST_CENTROID=longest takes 4 bytes a record for the exact owners kept beside the merged ones and 4 bytes a record for the lengths, and, while it "
               "chooses, about 5 bytes a record of scratch")
    assert modes(harness, {**prefix(value), **LONGEST})["note"] == off + clause + longest
    both = modes(harness, {**prefix(value), "FQD_FAST_OPTICAL": "9"})["note"]
    assert both.startswith(off + "; FQD_FAST_OPTICAL takes 16 bytes a record") and both.endswith(clause)
