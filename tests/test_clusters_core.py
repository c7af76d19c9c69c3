"""The words of the `--fast` units' cluster walk (fastq-dupaway_amd/csrc/fqd_clusters_core.hpp) on the CPU, in a harness built
with the sanitizers (tests/native/clusters_check.cpp): a list entry and the refusal word come apart into what went in, at the
ends of their fields; a list has room for every cluster that can be on it.  The device code that runs the same functions:
tests/test_gpu_optical.py, test_gpu_centroid.py, test_gpu_consensus.py, test_gpu_umi_merge.py, test_gpu_umi.py,
test_gpu_sizein.py."""
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "clusters_check.cpp"
EXE = HERE / "native" / "clusters_check"
ENDS = [0, 1, 2 ** 31 - 1, 2 ** 32 - 1]


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(EXE), str(SRC)], check=True, capture_output=True)
    return str(EXE)


def ask(harness, what, text=""):
    r = subprocess.run([harness, what], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def test_an_entry_comes_apart_into_its_place_and_members(harness):
    asked = [(k0, s) for k0 in ENDS for s in ENDS]
    got = ask(harness, "entry", "".join(f"{k0} {s}\n" for k0, s in asked))
    assert got == [((k0 << 32) | s, k0, s) for k0, s in asked]


def test_the_refusal_word_comes_apart_into_record_and_reason(harness):
    asked = [(record, reason) for record in (0, 2 ** 61 - 1) for reason in range(8)]
    got = ask(harness, "bad", "".join(f"{record} {reason}\n" for record, reason in asked))
    assert got == [((record << 3) | reason, record, reason) for record, reason in asked]
    # the lowest record wins an atomicMin whatever the reasons, and among one record's words the lowest reason
    words = [g[0] for g in got]
    assert words == sorted(words) and len(set(words)) == len(words)
    # "no record" is above every word a record below 2^61 - 1 can send: the one asked word that equals it is the last
    ((none,),) = ask(harness, "none")
    assert none == 2 ** 64 - 1 and [w for w in words if w >= none] == [words[-1]] and asked[-1] == (2 ** 61 - 1, 7)


def test_a_list_has_room_for_every_cluster_that_can_be_on_it(harness):
    """By exhaustion: among n places lie at most floor(n / (bound + 1)) disjoint clusters of more than `bound` members."""
    asked = [(n, bound) for bound in (1, 8, 64, 255) for n in range(301)]
    got = ask(harness, "room", "".join(f"{n} {bound}\n" for n, bound in asked))
    assert len(got) == len(asked)
    for (n, bound), (room,) in zip(asked, got):
        most, left = 0, n                                          # pack clusters of the smallest size that is listed
        while left >= bound + 1:
            most, left = most + 1, left - (bound + 1)
        assert most == n // (bound + 1)
        assert most <= room <= most + 1, (n, bound, room)
