"""FastModes::hamming (fastq-dupaway_amd/host/fast_modes.cpp), the host's view of FQD_FAST_HAMMING=D, in a small native harness
(tests/native/fast_hamming_check.cpp, built with the sanitizers): the values, the words of a bad value, the order in which
the variables are read, the predicates, names(), the refusals' words and the clause of the out-of-memory note.  Every
expected string is written out.  The run itself: tests/test_fast_hamming_cli.py."""
import os
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


@pytest.fixture(scope="module")
def harness():
    target = HERE / "native" / "fast_hamming_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "include"), "-o", str(target), str(HERE / "native" / "fast_hamming_check.cpp"),
                    str(ROOT / "fastq-dupaway_amd" / "host" / "fast_modes.cpp")], check=True, capture_output=True)
    return str(target)


def modes(harness, env, *args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("FQD_")}
    e.update(env)
    r = subprocess.run([harness, *map(str, args)], capture_output=True, text=True, env=e, timeout=60)
    assert r.returncode == 0, r.stderr
    return dict(line.split(" ", 1) if " " in line else (line, "") for line in r.stdout.splitlines())


def hamming(d):
    return {"FQD_FAST_HAMMING": str(d)}


def test_unset_and_zero_are_off(harness):
    off = modes(harness, {})
    assert off == {"hamming": "0", "optical": "0", "linked": "0", "any": "0", "names": "", "name": "", "note": off["note"], "check": "passed"}
    assert "HAMMING" not in off["note"]
    assert modes(harness, hamming(0)) == off


@pytest.mark.parametrize("d", [1, 2, 3])
def test_the_values_that_are_on(harness, d):
    on = modes(harness, hamming(d))
    assert (on["hamming"], on["linked"], on["any"], on["names"], on["name"], on["check"]) == (str(d), "1", "1", f"FQD_FAST_HAMMING={d}", f"FQD_FAST_HAMMING={d}", "passed")
    assert modes(harness, hamming(d), 0, 1, 1)["check"] == "passed"      # FASTA is allowed


@pytest.mark.parametrize("value", ["4", "-1", "", "x", "01", "1 ", "+1", "1.0", "00", "2147483648"])
def test_a_bad_value(harness, value):
    got = modes(harness, hamming(value))
    assert got == {"error": f"FQD_FAST_HAMMING must be 0, 1, 2 or 3, not '{value}'"}


def test_it_is_read_after_optical(harness):
    got = modes(harness, {"FQD_FAST_HAMMING": "9", "FQD_FAST_OPTICAL": "x"})
    assert got == {"error": "FQD_FAST_OPTICAL must be a decimal integer in 1 .. 2147483647, not 'x'"}
    got = modes(harness, {"FQD_FAST_HAMMING": "9", "FQD_FAST_OPTICAL": "5", "FQD_FAST_UMI_MISMATCH": "2"})
    assert got == {"error": "FQD_FAST_HAMMING must be 0, 1, 2 or 3, not '9'"}


def test_its_place_among_the_names(harness):
    env = {"FQD_FAST_KEEP": "best", "FQD_FAST_CLUSTERS": "1", "FQD_FAST_HAMMING": "2", "FQD_FAST_OPTICAL": "100", "FQD_FAST_SIZEOUT": "1", "FQD_FAST_MINSIZE": "2"}
    got = modes(harness, env)
    assert got["names"] == "FQD_FAST_KEEP=best and FQD_FAST_CLUSTERS=1 and FQD_FAST_HAMMING=2 and FQD_FAST_OPTICAL=100 and FQD_FAST_SIZEOUT=1 and FQD_FAST_MINSIZE=2"
    assert got["check"] == "passed"
    got = modes(harness, {"FQD_FAST_UMI": "colon", "FQD_FAST_UMI_MISMATCH": "1", "FQD_FAST_HAMMING": "1", "FQD_FAST_OPTICAL": "7"})
    assert got["names"] == "FQD_FAST_UMI=colon and FQD_FAST_UMI_MISMATCH=1 and FQD_FAST_HAMMING=1 and FQD_FAST_OPTICAL=7"


def test_both_strands_are_refused(harness):
    got = modes(harness, {**hamming(2), "FQD_FAST_STRAND": "both"})
    assert got["refusal"] == ("FQD_FAST_HAMMING=2 with FQD_FAST_STRAND=both: a substituted base can change which orientation of a read is the canonical one, "
                              "so copies with errors may be keyed in opposite orientations and never be compared")
    assert "check" not in got
    assert modes(harness, {**hamming(2), "FQD_FAST_STRAND": "given"})["check"] == "passed"


def test_umis_are_refused(harness):
    got = modes(harness, {**hamming(1), "FQD_FAST_UMI": "colon"})
    assert got["refusal"] == ("FQD_FAST_HAMMING=1 with FQD_FAST_UMI=colon: which sequences under one UMI are copies of one molecule is a rule of its own, "
                              "and this switch merges by sequence alone")
    got = modes(harness, {**hamming(3), "FQD_FAST_UMI": "underscore", "FQD_FAST_UMI_MISMATCH": "2"})
    assert got["refusal"] == ("FQD_FAST_HAMMING=3 with FQD_FAST_UMI=underscore and FQD_FAST_UMI_MISMATCH=2: which sequences under one UMI are copies of one molecule is a "
                              "rule of its own, and this switch merges by sequence alone")
    # the strands come first; a mismatch switch without its UMI switch is still that switch's own refusal
    assert modes(harness, {**hamming(1), "FQD_FAST_UMI": "colon", "FQD_FAST_STRAND": "both"})["refusal"].startswith("FQD_FAST_HAMMING=1 with FQD_FAST_STRAND=both: ")
    assert modes(harness, {**hamming(1), "FQD_FAST_UMI_MISMATCH": "1"})["refusal"].startswith("FQD_FAST_UMI_MISMATCH=1 merges the UMIs that FQD_FAST_UMI finds")


def test_unordered_and_several_devices_are_refused_as_for_every_linked_switch(harness):
    assert modes(harness, hamming(2), 1)["refusal"] == "FQD_FAST_HAMMING=2 with --unordered: these modes run on ordered inputs only"
    assert modes(harness, hamming(2), 0, 2)["refusal"] == "FQD_FAST_HAMMING=2 runs on one GPU: FQD_DEVICES may name one device only"
    assert modes(harness, {**hamming(2), "FQD_FAST_KEEP": "best"}, 0, 1, 1)["refusal"] == "FQD_FAST_KEEP=best needs the quality lines of FASTQ records: --format fasta has none"


@pytest.mark.parametrize("d", [1, 2, 3])
def test_the_clause_of_the_memory_note(harness, d):
    off = modes(harness, {})["note"]
    on = modes(harness, hamming(d))["note"]
    assert on == (off + f"; FQD_FAST_HAMMING takes 4 bytes a record for the merged owners and, while it merges, {24 * (d + 1)} bytes an exact cluster for the seeds "
                  f"and their sort (12 bytes a seed, {d + 1} seeds a cluster, twice over), 4 bytes a record for the labels and 8 bytes for every pair of clusters "
                  f"found near, with room for {d + 1} such pairs a cluster from the start")
    both = modes(harness, {**hamming(d), "FQD_FAST_OPTICAL": "9"})["note"]
    assert both.startswith(on + "; FQD_FAST_OPTICAL takes 16 bytes a record")
