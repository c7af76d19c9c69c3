"""FastModes::consensus (fastq-dupaway_amd/host/fast_modes.cpp), the host's view of FQD_FAST_CONSENSUS=1, in a small native
harness (tests/native/fast_consensus_check.cpp, built with the sanitizers): the spellings, the predicates, names(), the three
refusals' words and their order among the others, and the clause of the out-of-memory note.  Every expected string is written
out.  The run itself: tests/test_fast_consensus_cli.py."""
import os
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent

ON = {"FQD_FAST_CONSENSUS": "1"}
STRANDS = ("FQD_FAST_CONSENSUS=1 with FQD_FAST_STRAND=both: the members of a cluster may be keyed in opposite orientations, and a column-wise vote needs them in one; "
           "turning reads for the vote is not done")
SIZEIN = ("FQD_FAST_CONSENSUS=1 with FQD_FAST_SIZEIN=1: a record that stands for several reads has lost the quality lines of the reads it stands for, and the vote "
          "weighs every base by its quality")
FASTA = "FQD_FAST_CONSENSUS=1 with --format fasta: the vote weighs every base by its quality, and FASTA records have no quality lines"


@pytest.fixture(scope="module")
def harness():
    target = HERE / "native" / "fast_consensus_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "include"), "-o", str(target), str(HERE / "native" / "fast_consensus_check.cpp"),
                    str(ROOT / "fastq-dupaway_amd" / "host" / "fast_modes.cpp")], check=True, capture_output=True)
    return str(target)


def modes(harness, env, *args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("FQD_")}
    e.update(env)
    r = subprocess.run([harness, *map(str, args)], capture_output=True, text=True, env=e, timeout=60)
    assert r.returncode == 0, r.stderr
    return dict(line.split(" ", 1) if " " in line else (line, "") for line in r.stdout.splitlines())


def test_unset_and_zero_are_off(harness):
    off = modes(harness, {})
    assert off == {"consensus": "0", "linked": "0", "sized": "0", "any": "0", "names": "", "note": off["note"], "check": "passed"}
    assert "CONSENSUS" not in off["note"]
    for value in ("0", "", "x", "00", "off"):                    # FQD_FAST_CLUSTERS' reading: an integer other than 0 turns it on
        assert modes(harness, {"FQD_FAST_CONSENSUS": value}) == off


@pytest.mark.parametrize("value", ["1", "2", "-1", "01", "1x"])
def test_the_spellings_that_are_on(harness, value):
    on = modes(harness, {"FQD_FAST_CONSENSUS": value})
    assert (on["consensus"], on["linked"], on["sized"], on["any"], on["names"], on["check"]) == ("1", "1", "0", "1", "FQD_FAST_CONSENSUS=1", "passed")


def test_it_reads_like_the_cluster_files_switch(harness):
    for value in ("1", "0", "", "7", "yes"):
        a = modes(harness, {"FQD_FAST_CONSENSUS": value})
        b = modes(harness, {"FQD_FAST_CLUSTERS": value})
        assert (a["linked"], a["any"]) == (b["linked"], b["any"]) and (a["names"] != "") == (b["names"] != "")


def test_its_place_among_the_names(harness):
    env = {"FQD_FAST_KEEP": "best", "FQD_FAST_CLUSTERS": "1", "FQD_FAST_HAMMING": "2", "FQD_FAST_OPTICAL": "100", "FQD_FAST_CONSENSUS": "1", "FQD_FAST_SIZEOUT": "1",
           "FQD_FAST_MINSIZE": "2"}
    got = modes(harness, env)
    assert got["names"] == ("FQD_FAST_KEEP=best and FQD_FAST_CLUSTERS=1 and FQD_FAST_HAMMING=2 and FQD_FAST_OPTICAL=100 and FQD_FAST_CONSENSUS=1 and FQD_FAST_SIZEOUT=1 "
                            "and FQD_FAST_MINSIZE=2")
    assert got["check"] == "passed"
    got = modes(harness, {"FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1", **ON})
    assert (got["names"], got["check"]) == ("FQD_FAST_UMI=colon and FQD_FAST_UMI_MISMATCH=1 and FQD_FAST_CONSENSUS=1", "passed")


def test_both_strands_are_refused(harness):
    got = modes(harness, {**ON, "FQD_FAST_STRAND": "both"})
    assert got["refusal"] == STRANDS and "check" not in got
    assert modes(harness, {**ON, "FQD_FAST_STRAND": "given"})["check"] == "passed"


def test_size_annotations_are_refused(harness):
    got = modes(harness, {**ON, "FQD_FAST_SIZEIN": "1", "FQD_FAST_SIZEOUT": "1"})
    assert got["refusal"] == SIZEIN and "check" not in got
    assert modes(harness, {**ON, "FQD_FAST_SIZEIN": "0", "FQD_FAST_SIZEOUT": "1"})["check"] == "passed"


def test_fasta_is_refused(harness):
    assert modes(harness, ON, 0, 1, 1)["refusal"] == FASTA
    assert modes(harness, ON, 0, 1, 0)["check"] == "passed"


def test_the_order_of_the_refusals(harness):
    everything = {**ON, "FQD_FAST_STRAND": "both", "FQD_FAST_SIZEIN": "1", "FQD_FAST_SIZEOUT": "1"}
    # the existing ones that stand in front
    assert modes(harness, {**ON, "FQD_FAST_SIZEIN": "1"}, 1, 2, 1)["refusal"].startswith("FQD_FAST_SIZEIN=1 changes what a cluster's size is and nothing else")
    assert modes(harness, {**everything, "FQD_FAST_UMI_MISMATCH": "1"}, 1, 2, 1)["refusal"].startswith("FQD_FAST_UMI_MISMATCH=1 merges the UMIs that FQD_FAST_UMI finds")
    assert modes(harness, {**everything, "FQD_FAST_HAMMING": "1"}, 1, 2, 1)["refusal"].startswith("FQD_FAST_HAMMING=1 with FQD_FAST_STRAND=both: ")
    assert modes(harness, {**ON, "FQD_FAST_SIZEIN": "1", "FQD_FAST_SIZEOUT": "1", "FQD_FAST_HAMMING": "1", "FQD_FAST_UMI": "colon"}, 1, 2, 1)["refusal"].startswith(
        "FQD_FAST_HAMMING=1 with FQD_FAST_UMI=colon: ")
    # the strands, then the annotations, in front of the command line's
    assert modes(harness, everything, 1, 2, 1)["refusal"] == STRANDS
    del everything["FQD_FAST_STRAND"]
    assert modes(harness, everything, 1, 2, 1)["refusal"] == SIZEIN
    # `--unordered`, several devices and FQD_FAST_KEEP=best with FASTA in front of this switch's FASTA refusal
    assert modes(harness, ON, 1, 2, 1)["refusal"] == "FQD_FAST_CONSENSUS=1 with --unordered: these modes run on ordered inputs only"
    assert modes(harness, ON, 0, 2, 1)["refusal"] == "FQD_FAST_CONSENSUS=1 runs on one GPU: FQD_DEVICES may name one device only"
    assert modes(harness, {**ON, "FQD_FAST_KEEP": "best"}, 0, 1, 1)["refusal"] == "FQD_FAST_KEEP=best needs the quality lines of FASTQ records: --format fasta has none"
    assert modes(harness, ON, 0, 1, 1)["refusal"] == FASTA


def test_the_clause_of_the_memory_note(harness):
    off = modes(harness, {})["note"]
    on = modes(harness, ON)["note"]
    assert on == (off + "; FQD_FAST_CONSENSUS takes, for paired files, 1 byte a record for the pairs it changed and, while it votes, 4 bytes a cluster and up to 5 bytes "
                  "a record of scratch (the scratch of the grouping serves where it is as large)")
    with_optical = modes(harness, {"FQD_FAST_OPTICAL": "9"})["note"]
    assert modes(harness, {**ON, "FQD_FAST_OPTICAL": "9"})["note"] == with_optical + on[len(off):]
