"""FastModes::umi_hamming (fastq-dupaway_amd/host/fast_modes.cpp), the host's view of FQD_FAST_UMI_HAMMING=D, in a small native
harness (tests/native/fast_umi_hamming_check.cpp, built with the sanitizers): the values, the words of a bad value, the order in
which the variables are read, the predicates, names(), the two refusals, their words and their place among the old ones, and the
clause of the out-of-memory note.  Every expected string is written out.  The run itself: tests/test_fast_umi_hamming_cli.py."""
import os
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


@pytest.fixture(scope="module")
def harness():
    target = HERE / "native" / "fast_umi_hamming_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "include"), "-o", str(target), str(HERE / "native" / "fast_umi_hamming_check.cpp"),
                    str(ROOT / "fastq-dupaway_amd" / "host" / "fast_modes.cpp")], check=True, capture_output=True)
    return str(target)


def modes(harness, env, *args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("FQD_")}
    e.update(env)
    r = subprocess.run([harness, *map(str, args)], capture_output=True, text=True, env=e, timeout=60)
    assert r.returncode == 0, r.stderr
    return dict(line.split(" ", 1) if " " in line else (line, "") for line in r.stdout.splitlines())


def switch(d, umi="colon"):
    return {"FQD_FAST_UMI_HAMMING": str(d), **({"FQD_FAST_UMI": umi} if umi else {})}


def test_unset_and_zero_are_off(harness):
    off = modes(harness, {})
    assert off == {"umi_hamming": "0", "hamming": "0", "umi": "0", "linked": "0", "any": "0", "names": "", "name": "", "note": off["note"], "check": "passed"}
    assert "HAMMING" not in off["note"]
    assert modes(harness, switch(0, None)) == off
    # with FQD_FAST_UMI: 0 is the FQD_FAST_UMI run, which links nothing
    umi = modes(harness, {"FQD_FAST_UMI": "colon"})
    assert (umi["linked"], umi["any"], umi["names"]) == ("0", "1", "FQD_FAST_UMI=colon")
    assert modes(harness, switch(0)) == umi


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("umi", ["colon", "underscore"])
def test_the_values_that_are_on(harness, d, umi):
    on = modes(harness, switch(d, umi))
    assert (on["umi_hamming"], on["hamming"], on["umi"], on["linked"], on["any"], on["name"], on["check"]) == \
           (str(d), "0", str(ord(":" if umi == "colon" else "_")), "1", "1", f"FQD_FAST_UMI_HAMMING={d}", "passed")
    assert on["names"] == f"FQD_FAST_UMI={umi} and FQD_FAST_UMI_HAMMING={d}"
    assert modes(harness, switch(d, umi), 0, 1, 1)["check"] == "passed"      # FASTA is allowed


@pytest.mark.parametrize("value", ["4", "-1", "", "x", "01", "1 ", "+1", "1.0", "00", "2147483648"])
def test_a_bad_value(harness, value):
    assert modes(harness, switch(value)) == {"error": f"FQD_FAST_UMI_HAMMING must be 0, 1, 2 or 3, not '{value}'"}
    assert modes(harness, switch(value, None)) == {"error": f"FQD_FAST_UMI_HAMMING must be 0, 1, 2 or 3, not '{value}'"}


def test_it_is_read_directly_behind_hamming(harness):
    got = modes(harness, {"FQD_FAST_UMI_HAMMING": "9", "FQD_FAST_HAMMING": "x"})
    assert got == {"error": "FQD_FAST_HAMMING must be 0, 1, 2 or 3, not 'x'"}
    got = modes(harness, {"FQD_FAST_UMI_HAMMING": "9", "FQD_FAST_OPTICAL": "x"})
    assert got == {"error": "FQD_FAST_OPTICAL must be a decimal integer in 1 .. 2147483647, not 'x'"}
    got = modes(harness, {"FQD_FAST_UMI_HAMMING": "9", "FQD_FAST_HAMMING": "3", "FQD_FAST_OPTICAL": "5", "FQD_FAST_UMI_MISMATCH": "2", "FQD_FAST_CONSENSUS": "1"})
    assert got == {"error": "FQD_FAST_UMI_HAMMING must be 0, 1, 2 or 3, not '9'"}


def test_its_place_among_the_names(harness):
    env = {"FQD_FAST_KEEP": "best", "FQD_FAST_CLUSTERS": "1", "FQD_FAST_UMI": "underscore", "FQD_FAST_UMI_MISMATCH": "1", "FQD_FAST_UMI_HAMMING": "2",
           "FQD_FAST_OPTICAL": "100", "FQD_FAST_CONSENSUS": "1", "FQD_FAST_SIZEOUT": "1", "FQD_FAST_MINSIZE": "2"}
    got = modes(harness, env)
    assert got["names"] == ("FQD_FAST_KEEP=best and FQD_FAST_CLUSTERS=1 and FQD_FAST_UMI=underscore and FQD_FAST_UMI_MISMATCH=1 and FQD_FAST_UMI_HAMMING=2 and "
                            "FQD_FAST_OPTICAL=100 and FQD_FAST_CONSENSUS=1 and FQD_FAST_SIZEOUT=1 and FQD_FAST_MINSIZE=2")
    assert got["check"] == "passed"
    # directly behind the mismatch switch, in front of FQD_FAST_HAMMING (the two are refused together, and the refusal names them)
    got = modes(harness, {"FQD_FAST_UMI": "colon", "FQD_FAST_UMI_HAMMING": "1", "FQD_FAST_HAMMING": "3", "FQD_FAST_OPTICAL": "7"})
    assert got["names"] == "FQD_FAST_UMI=colon and FQD_FAST_UMI_HAMMING=1 and FQD_FAST_HAMMING=3 and FQD_FAST_OPTICAL=7"


def test_the_switch_without_the_umi_switch_is_refused(harness):
    for d in (1, 2, 3):
        got = modes(harness, switch(d, None))
        assert got["refusal"] == (f"FQD_FAST_UMI_HAMMING={d} merges the sequences under one of the UMIs that FQD_FAST_UMI finds: set FQD_FAST_UMI=colon or "
                                  "FQD_FAST_UMI=underscore as well")
        assert "check" not in got
    assert modes(harness, {"FQD_FAST_UMI_HAMMING": "1", "FQD_FAST_UMI": "off"})["refusal"].startswith("FQD_FAST_UMI_HAMMING=1 merges the sequences under one of the UMIs")


def test_both_strands_are_refused(harness):
    got = modes(harness, {**switch(2), "FQD_FAST_STRAND": "both"})
    assert got["refusal"] == ("FQD_FAST_UMI_HAMMING=2 with FQD_FAST_STRAND=both: a substituted base can change which orientation of a read is the canonical one, "
                              "so copies with errors may be keyed in opposite orientations and never be compared")
    assert "check" not in got
    assert modes(harness, {**switch(2), "FQD_FAST_STRAND": "given"})["check"] == "passed"
    # without the UMI switch that refusal comes first
    assert modes(harness, {**switch(2, None), "FQD_FAST_STRAND": "both"})["refusal"].startswith("FQD_FAST_UMI_HAMMING=2 merges the sequences under one of the UMIs")


def test_the_place_of_the_refusals_among_the_old_ones(harness):
    # in front of them, unmoved: SIZEIN with nothing that reads sizes, UMI_MISMATCH without UMI, HAMMING with STRAND=both, HAMMING with UMI
    assert modes(harness, {**switch(1, None), "FQD_FAST_SIZEIN": "1"})["refusal"].startswith("FQD_FAST_SIZEIN=1 changes what a cluster's size is and nothing else")
    assert modes(harness, {**switch(1, None), "FQD_FAST_UMI_MISMATCH": "1"})["refusal"] == \
        "FQD_FAST_UMI_MISMATCH=1 merges the UMIs that FQD_FAST_UMI finds: set FQD_FAST_UMI=colon or FQD_FAST_UMI=underscore as well"
    assert modes(harness, {**switch(1, None), "FQD_FAST_HAMMING": "2", "FQD_FAST_STRAND": "both"})["refusal"].startswith("FQD_FAST_HAMMING=2 with FQD_FAST_STRAND=both: ")
    assert modes(harness, {**switch(1), "FQD_FAST_HAMMING": "2"})["refusal"] == \
        ("FQD_FAST_HAMMING=2 with FQD_FAST_UMI=colon: which sequences under one UMI are copies of one molecule is a rule of its own, and this switch merges by "
         "sequence alone")
    assert modes(harness, {**switch(1), "FQD_FAST_HAMMING": "2", "FQD_FAST_UMI_MISMATCH": "1"})["refusal"].startswith(
        "FQD_FAST_HAMMING=2 with FQD_FAST_UMI=colon and FQD_FAST_UMI_MISMATCH=1: which sequences")
    # behind them: CONSENSUS with STRAND=both, CONSENSUS with SIZEIN, --unordered, several devices, the FASTA ones
    assert modes(harness, {**switch(1), "FQD_FAST_STRAND": "both", "FQD_FAST_CONSENSUS": "1"})["refusal"].startswith("FQD_FAST_UMI_HAMMING=1 with FQD_FAST_STRAND=both: ")
    assert modes(harness, {**switch(1, None), "FQD_FAST_CONSENSUS": "1", "FQD_FAST_SIZEIN": "1", "FQD_FAST_LEVELS": "1"})["refusal"].startswith(
        "FQD_FAST_UMI_HAMMING=1 merges the sequences")
    assert modes(harness, {**switch(1), "FQD_FAST_CONSENSUS": "1", "FQD_FAST_SIZEIN": "1", "FQD_FAST_LEVELS": "1"})["refusal"].startswith(
        "FQD_FAST_CONSENSUS=1 with FQD_FAST_SIZEIN=1: ")
    assert modes(harness, switch(2, None), 1)["refusal"].startswith("FQD_FAST_UMI_HAMMING=2 merges the sequences")
    assert modes(harness, switch(2), 1)["refusal"] == "FQD_FAST_UMI=colon and FQD_FAST_UMI_HAMMING=2 with --unordered: these modes run on ordered inputs only"
    assert modes(harness, switch(2), 0, 2)["refusal"] == "FQD_FAST_UMI=colon and FQD_FAST_UMI_HAMMING=2 runs on one GPU: FQD_DEVICES may name one device only"
    assert modes(harness, {**switch(2), "FQD_FAST_KEEP": "best"}, 0, 1, 1)["refusal"] == "FQD_FAST_KEEP=best needs the quality lines of FASTQ records: --format fasta has none"
    # the partners that are allowed
    for env in ({"FQD_FAST_UMI_MISMATCH": "2"}, {"FQD_FAST_CONSENSUS": "1"}, {"FQD_FAST_OPTICAL": "50"}, {"FQD_FAST_KEEP": "best", "FQD_FAST_SORT": "size"},
                {"FQD_FAST_SIZEIN": "1", "FQD_FAST_SIZEOUT": "1"}):
        assert modes(harness, {**switch(3, "underscore"), **env})["check"] == "passed", env


@pytest.mark.parametrize("d", [1, 2, 3])
def test_the_clause_of_the_memory_note(harness, d):
    off = modes(harness, {"FQD_FAST_UMI": "colon"})["note"]
    on = modes(harness, switch(d))["note"]
    assert on == (off + f"; FQD_FAST_UMI_HAMMING takes 4 bytes a record for the molecules' owners and, while it merges, {24 * (d + 1)} bytes an exact cluster for the "
                  f"seeds and their sort, 4 bytes a record for the labels and 8 bytes for every pair of clusters found near, with room for {d + 1} of them a "
                  "cluster from the start")
    both = modes(harness, {**switch(d), "FQD_FAST_UMI_MISMATCH": "1", "FQD_FAST_OPTICAL": "9"})["note"]
    mismatch = modes(harness, {"FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1"})["note"]
    assert both.startswith(mismatch + "; FQD_FAST_UMI_HAMMING takes 4 bytes a record for the molecules' owners, 4 bytes a record more for the exact owners kept beside the "
                           f"merged ones and, while it merges, {24 * (d + 1)} bytes an exact cluster for the seeds and their sort, 4 bytes a record for the labels and 8 "
                           f"bytes for every pair of clusters found near and every link, with room for {d + 1} of them a cluster from the start"
                           "; FQD_FAST_OPTICAL takes 16 bytes a record")
