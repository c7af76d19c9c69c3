"""FastModes::centroid (fastq-dupaway_amd/host/fast_modes.cpp), the host's view of FQD_FAST_CENTROID=first|abundant, in a small
native harness (tests/native/fast_centroid_check.cpp, built with the sanitizers): the spellings, the words of a bad value, the
order in which the variables are read, the predicates, names(), the refusals' words and which of two is said, and the clause of
the out-of-memory note.  Every expected string is written out.  The run itself: tests/test_fast_centroid_cli.py."""
import os
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
ABUNDANT = {"FQD_FAST_CENTROID": "abundant"}
HAMMING = {"FQD_FAST_HAMMING": "1"}
ALONE = ("FQD_FAST_CENTROID=abundant chooses among the different sequences of a merged cluster and nothing else: set one of FQD_FAST_UMI_MISMATCH, "
         "FQD_FAST_HAMMING or FQD_FAST_UMI_HAMMING as well, which merge them (without one every cluster holds one sequence)")


@pytest.fixture(scope="module")
def harness():
    target = HERE / "native" / "fast_centroid_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "include"), "-o", str(target), str(HERE / "native" / "fast_centroid_check.cpp"),
                    str(ROOT / "fastq-dupaway_amd" / "host" / "fast_modes.cpp")], check=True, capture_output=True)
    return str(target)


def modes(harness, env, *args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("FQD_")}
    e.update(env)
    r = subprocess.run([harness, *map(str, args)], capture_output=True, text=True, env=e, timeout=60)
    assert r.returncode == 0, r.stderr
    return dict(line.split(" ", 1) if " " in line else (line, "") for line in r.stdout.splitlines())


def test_unset_and_first_are_off(harness):
    off = modes(harness, {})
    assert off == {"centroid": "0", "merges": "0", "linked": "0", "any": "0", "names": "", "note": off["note"], "check": "passed"}
    assert "CENTROID" not in off["note"]
    assert modes(harness, {"FQD_FAST_CENTROID": "first"}) == off
    # beside other switches as well: `first` changes nothing that is said
    env = {"FQD_FAST_HAMMING": "2", "FQD_FAST_KEEP": "best", "FQD_FAST_SIZEOUT": "1"}
    assert modes(harness, {**env, "FQD_FAST_CENTROID": "first"}) == modes(harness, env)


def test_abundant_beside_a_merging_switch(harness):
    on = modes(harness, {**ABUNDANT, **HAMMING})
    assert (on["centroid"], on["merges"], on["linked"], on["any"], on["check"]) == ("1", "1", "1", "1", "passed")
    assert on["names"] == "FQD_FAST_HAMMING=1 and FQD_FAST_CENTROID=abundant"
    assert modes(harness, {**ABUNDANT, **HAMMING}, 0, 1, 1)["check"] == "passed"                       # FASTA is allowed
    for env in ({"FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1"}, {"FQD_FAST_UMI": "underscore", "FQD_FAST_UMI_HAMMING": "2"},
                {"FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "2", "FQD_FAST_UMI_HAMMING": "1", "FQD_FAST_OPTICAL": "40"}):
        got = modes(harness, {**ABUNDANT, **env})
        assert (got["centroid"], got["merges"], got["check"]) == ("1", "1", "passed"), env
    # both strands: allowed where the merging switch allows them (abundance by orientation is not told apart)
    assert modes(harness, {**ABUNDANT, "FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1", "FQD_FAST_STRAND": "both"})["check"] == "passed"


@pytest.mark.parametrize("value", ["", "Abundant", "abundant ", "best", "1", "0", "most", "first,abundant"])
def test_a_bad_value(harness, value):
    assert modes(harness, {"FQD_FAST_CENTROID": value}) == {"error": f"FQD_FAST_CENTROID must be 'first' or 'abundant', not '{value}'"}


def test_it_is_read_after_umi_hamming(harness):
    got = modes(harness, {"FQD_FAST_CENTROID": "x", "FQD_FAST_UMI_HAMMING": "9"})
    assert got == {"error": "FQD_FAST_UMI_HAMMING must be 0, 1, 2 or 3, not '9'"}
    got = modes(harness, {"FQD_FAST_CENTROID": "x", "FQD_FAST_HAMMING": "7"})
    assert got == {"error": "FQD_FAST_HAMMING must be 0, 1, 2 or 3, not '7'"}
    got = modes(harness, {"FQD_FAST_CENTROID": "x", "FQD_FAST_UMI_HAMMING": "1", "FQD_FAST_KEEP": "best"})
    assert got == {"error": "FQD_FAST_CENTROID must be 'first' or 'abundant', not 'x'"}


def test_its_place_among_the_names(harness):
    env = {"FQD_FAST_KEEP": "best", "FQD_FAST_CLUSTERS": "1", "FQD_FAST_HAMMING": "2", "FQD_FAST_OPTICAL": "100", "FQD_FAST_CONSENSUS": "1", "FQD_FAST_SIZEOUT": "1",
           "FQD_FAST_MINSIZE": "2", **ABUNDANT}
    got = modes(harness, env)
    assert got["names"] == ("FQD_FAST_KEEP=best and FQD_FAST_CLUSTERS=1 and FQD_FAST_HAMMING=2 and FQD_FAST_OPTICAL=100 and FQD_FAST_CONSENSUS=1 and "
                            "FQD_FAST_CENTROID=abundant and FQD_FAST_SIZEOUT=1 and FQD_FAST_MINSIZE=2")
    assert got["check"] == "passed"


def test_alone_it_is_refused(harness):
    got = modes(harness, ABUNDANT)
    assert got["refusal"] == ALONE and "check" not in got
    # with switches that do not merge: still alone
    for env in ({"FQD_FAST_KEEP": "best"}, {"FQD_FAST_CLUSTERS": "1", "FQD_FAST_SIZEOUT": "1"}, {"FQD_FAST_OPTICAL": "50"}, {"FQD_FAST_UMI": "colon"},
                {"FQD_FAST_STRAND": "both"}):
        assert modes(harness, {**ABUNDANT, **env})["refusal"] == ALONE, env
    assert modes(harness, ABUNDANT, 0, 1, 1)["refusal"] == ALONE                                       # FASTA: the same words


def test_which_of_two_refusals_is_said(harness):
    # everything in front of it in check()'s order is said first ...
    assert modes(harness, {**ABUNDANT, "FQD_FAST_SIZEIN": "1"})["refusal"].startswith("FQD_FAST_SIZEIN=1 changes what a cluster's size is and nothing else")
    assert modes(harness, {**ABUNDANT, "FQD_FAST_UMI_MISMATCH": "1"})["refusal"].startswith("FQD_FAST_UMI_MISMATCH=1 merges the UMIs that FQD_FAST_UMI finds")
    assert modes(harness, {**ABUNDANT, "FQD_FAST_UMI_HAMMING": "1"})["refusal"].startswith("FQD_FAST_UMI_HAMMING=1 merges the sequences under one of the UMIs")
    assert modes(harness, {**ABUNDANT, **HAMMING, "FQD_FAST_STRAND": "both"})["refusal"].startswith("FQD_FAST_HAMMING=1 with FQD_FAST_STRAND=both: ")
    assert modes(harness, {**ABUNDANT, "FQD_FAST_CONSENSUS": "1", "FQD_FAST_STRAND": "both"})["refusal"].startswith("FQD_FAST_CONSENSUS=1 with FQD_FAST_STRAND=both: ")
    got = modes(harness, {**ABUNDANT, "FQD_FAST_CONSENSUS": "1", "FQD_FAST_SIZEIN": "1", "FQD_FAST_SIZEOUT": "1"})
    assert got["refusal"].startswith("FQD_FAST_CONSENSUS=1 with FQD_FAST_SIZEIN=1: ")
    # ... and it is said in front of everything behind it
    assert modes(harness, ABUNDANT, 1)["refusal"] == ALONE
    assert modes(harness, ABUNDANT, 0, 2)["refusal"] == ALONE
    assert modes(harness, {**ABUNDANT, "FQD_FAST_KEEP": "best"}, 0, 1, 1)["refusal"] == ALONE
    assert modes(harness, {**ABUNDANT, "FQD_FAST_CONSENSUS": "1"}, 0, 1, 1)["refusal"] == ALONE


def test_unordered_and_several_devices_are_refused_as_for_every_linked_switch(harness):
    env = {**ABUNDANT, **HAMMING}
    assert modes(harness, env, 1)["refusal"] == "FQD_FAST_HAMMING=1 and FQD_FAST_CENTROID=abundant with --unordered: these modes run on ordered inputs only"
    assert modes(harness, env, 0, 2)["refusal"] == "FQD_FAST_HAMMING=1 and FQD_FAST_CENTROID=abundant runs on one GPU: FQD_DEVICES may name one device only"
    assert modes(harness, {**env, "FQD_FAST_KEEP": "best"}, 0, 1, 1)["refusal"] == "FQD_FAST_KEEP=best needs the quality lines of FASTQ records: --format fasta has none"


def test_the_clause_of_the_memory_note(harness):
    clause = ("; FQD_FAST_CENTROID takes 4 bytes a record for the exact owners kept beside the merged ones and, while it chooses, 4 bytes a record for the "
              "abundances, about 5 bytes a record of scratch and 32 bytes for every member of a cluster above 2048")
    for env in (HAMMING, {"FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1", "FQD_FAST_CONSENSUS": "1", "FQD_FAST_SORT": "size"}):
        without = modes(harness, env)["note"]
        assert modes(harness, {**env, **ABUNDANT})["note"] == without + clause
        assert modes(harness, {**env, "FQD_FAST_CENTROID": "first"})["note"] == without
