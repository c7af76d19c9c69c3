"""`--compare-seq` in ranges of the sort order (FQD_SEQ_RANGE_KB; host/run_sequence.cpp, rules in csrc/fqd_seq_range_core.hpp).
Every case is run in core and ranged by the same binary: outputs, `.clusters` files and `-v` lines must be the same bytes
(a `.gz` output is compared after it is inflated: its text is the same bytes, but the ranged run ends a BGZF member where a
range ends, so the member boundaries — not the text — differ from the in-core file's), and equal to the restatement (tests/seq_reference.py) under the comparison of tests/test_seq_cli.py.  The number of ranges
is read off the run's timing line and must be what a brute-force plan over the keys says — and at least 3: a run that did
not split proves nothing.  Then hand-built clusters that straddle cuts, one key value beyond the target, and the refusals."""
import os
import random
import re
import threading
from pathlib import Path

import pytest

import seq_reference as ref
from test_seq_cli import check_same, exe, make_reads, read_out, run, write      # noqa: F401 (exe is a fixture)
from test_seq_ranged_core import brute_plan

pytestmark = pytest.mark.gpu
LINE = re.compile(r"^sequence: ranged run, (\d+) ranges, largest (\d+) bytes$", re.M)


def planned_ranges(data, fasta, target):
    """The plan the run must come to, from the records themselves: mate 1's key, both mates' sizes, the shorter file's count."""
    recs = [ref.parse(d, fasta) for d in data]
    n = min(len(r) for r in recs)
    pairs = []
    for i in range(n):
        seq = recs[0][i][2].rstrip(b"\n")
        pairs.append((int.from_bytes((seq + b"\n" * 8)[:8], "big"), sum(len(r[i][0]) for r in recs)))
    return brute_plan(pairs, target)[0]


def both_ways(exe, tmp_path, data, fasta, mode, d, in_kind="plain", out_gz=False, clusters=False, kb=32, extra_env=None, min_ranges=3):
    """Runs in core and ranged; checks the two against each other and against the restatement; returns the ranged run."""
    ext = ".fa" if fasta else ".fq"
    ins = [tmp_path / (f"in{k}{ext}" + (".gz" if in_kind != "plain" else "")) for k in range(len(data))]
    for p, x in zip(ins, data):
        write(p, x, in_kind)
    results = {}
    for how in ("core", "ranged"):
        outs = [tmp_path / (f"{how}{k}{ext}" + (".gz" if out_gz else "")) for k in range(len(data))]
        args = ["-i", ins[0], "-o", outs[0]]
        if len(data) == 2:
            args += ["-u", ins[1], "-p", outs[1]]
        args += ["--compare-seq", mode, "--distance", d, "-v"]
        if fasta:
            args += ["--format", "fasta"]
        if clusters:
            args += ["--write-clusters"]
        env = {"FQD_HOST_TIMING": "1", **(extra_env or {})}
        if how == "ranged":
            env["FQD_SEQ_RANGE_KB"] = str(kb)
        r = run(exe, *args, env=env)
        assert r.returncode == 0, r.stderr
        results[how] = (r, outs)
    (rc, oc), (rr, orr) = results["core"], results["ranged"]
    assert LINE.search(rc.stderr) is None
    m = LINE.search(rr.stderr)
    assert m, rr.stderr
    R, largest = int(m.group(1)), int(m.group(2))
    rows = planned_ranges(data, fasta, kb << 10)
    print(f"[ranged] {R} ranges, largest {largest} bytes")
    assert R == len(rows) and largest == max(b for _, _, _, b in rows)
    assert R >= min_ranges
    exp_out, exp_cl, total, dups = ref.dedup(data, fasta=fasta, mode=ref.MODES[mode], distance=d)
    assert rr.stdout == rc.stdout == ref.verbose_line(total, dups, len(data) == 2)
    for k in range(len(data)):
        assert read_out(orr[k]) == read_out(oc[k])                  # ties are stable in both: the same bytes
        if not out_gz:
            assert orr[k].read_bytes() == oc[k].read_bytes()
        check_same(read_out(orr[k]), exp_out[k], fasta)
        cr, cc = Path(str(orr[k]) + ".clusters"), Path(str(oc[k]) + ".clusters")
        assert cr.exists() == cc.exists() == clusters
        if clusters:
            assert cr.read_bytes() == cc.read_bytes()
            got = cr.read_bytes()
            if got != exp_cl[k]:
                assert sorted(got.split(b"\n")) == sorted(exp_cl[k].split(b"\n"))
                assert [x.startswith(b"--") for x in got.split(b"\n")] == [x.startswith(b"--") for x in exp_cl[k].split(b"\n")]
    return rr


CASES = [
    # (fasta, paired, mode, distance, crlf, in_kind, out_gz, clusters, unequal)
    (False, False, "tight", 2, False, "plain", False, True, False),
    (False, False, "loose", 2, False, "bgzf", False, True, False),
    (False, False, "tail-hamming", 1, True, "plain", True, True, False),
    (False, False, "tail-hamming", 3, False, "gz", False, False, False),
    (True, False, "loose", 2, True, "gz", True, False, False),
    (False, True, "tight", 2, False, "plain", False, True, True),
    (False, True, "loose", 2, False, "bgzf", True, True, True),
    (False, True, "tail-hamming", 2, False, "plain", False, True, True),
    (True, True, "loose", 2, True, "plain", False, False, False),
    (True, True, "tail-hamming", 1, False, "gz", False, True, False),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{'fa' if c[0] else 'fq'}-{'pe' if c[1] else 'se'}-{c[2]}-d{c[3]}-{c[5]}{'-gzout' if c[6] else ''}"
                                             f"{'-crlf' if c[4] else ''}" for c in CASES])
def test_ranged_equals_in_core_and_restatement(exe, tmp_path, case):
    fasta, paired, mode, d, crlf, in_kind, out_gz, clusters, unequal = case
    rng = random.Random(100 + CASES.index(case))
    n = 3000
    files = [make_reads(rng, n, fasta, crlf, pool_size=150)]          # many distinct 8-byte prefixes: the split happens
    if paired:
        files.append(make_reads(rng, n - 137 if unequal else n, fasta, crlf, pool_size=10))
    data = [b"".join(f) for f in files]
    both_ways(exe, tmp_path, data, fasta, mode, d, in_kind, out_gz, clusters, kb=16 if fasta else 32)


def test_several_blocks_per_pass(exe, tmp_path):
    """Inputs of several reader blocks (FQD_BLOCK_MB=1): a range's records come out of many blocks, in input order."""
    rng = random.Random(77)
    data = [b"".join(make_reads(rng, 16000, False, False, pool_size=400)), b"".join(make_reads(rng, 16000, False, False, pool_size=30))]
    assert len(data[0]) > 2_000_000
    both_ways(exe, tmp_path, data, False, "loose", 2, clusters=True, kb=512, extra_env={"FQD_BLOCK_MB": "1"})


def fat(name, seq, fasta=True):
    """A record of more than 512 bytes whatever its sequence: with FQD_SEQ_RANGE_KB=1 no two key values share a range."""
    pad = "x" * 600
    if fasta:
        return f">{name} {pad}\n{seq}\n".encode()
    return f"@{name} {pad}\n{seq}\n+\n{'I' * len(seq)}\n".encode()


BOUNDARY = {
    # a loose chain over cuts: every record a prefix of the next; the keys of the first three differ
    "loose-chain": ("loose", 0, [["ACGT", "ACGTAAAAA", "ACGTAAAAAC", "ACGTAA", "ACG", "ACGTAAAAACGG", "ACGTT", "", "A"]]),
    # tail-hamming: within d, differing in byte 3 (another key, another range); a member, then a non-member after it
    "hamming-byte3": ("tail-hamming", 1, [["ACGAACGTACGT", "ACGTACGTACGT", "ACGTACGTACGA", "ACGTACGTACTA", "ACGCACGTACGT", "ACGGACGTACGG"]]),
    "hamming-head-member-stranger": ("tail-hamming", 2, [["AAAAAAAAAAAA", "AAAAAAACAAAA", "AAAAAAAGAAAA", "AAAAAACCAAAT", "AAAAAAATAAAAA", "AAAAAAAT"]]),
    "hamming-d0": ("tail-hamming", 0, [["ACGTACGTA", "ACGTACGTA", "ACGAACGTA", "ACGTACGTC", "ACGCACGTA", "TCGTACGTA"]]),
    "empties": ("loose", 0, [["", "", "A", "", "AC", "T"]]),
    "empties-hamming": ("tail-hamming", 3, [["", "A", "", "C", "AC", "GT", "G"]]),
    "tight-neighbours": ("tight", 0, [["ACGTACGT", "ACGTACGTA", "ACGTACGT", "ACGTACG", "ACGTACGTA", ""]]),
    # pairs: mate 1 decides the range, mate 2 the cluster
    "pe-loose": ("loose", 0, [["ACGT", "ACGTAAAAA", "ACGTAAAAAC", "ACGTAA", "ACGTAAAAACT"], ["GG", "GGT", "GGTA", "GC", "GGTAC"]]),
    "pe-loose-sides": ("loose", 0, [["ACGT", "ACGTAAAAA", "ACGTAAAAAC", "ACGTAAAAACC", "ACG", "ACGTAA"], ["GGTT", "GGT", "GGTA", "GGTAC", "GGTTA", "GG"]]),
    "pe-hamming": ("tail-hamming", 1, [["ACGAACGTACGT", "ACGTACGTACGT", "ACGCACGTACGT", "ACGGACGTACGT", "ACGTACGTACGA"],
                                       ["TTTTTTTT", "TTTTTTTT", "TTTTTTAA", "TTTTTTTA", "TTTTTTTT"]]),
    "pe-tight": ("tight", 0, [["ACGTACGTA", "ACGTACGTA", "ACGTACGTA", "ACGTACGT", "ACGTACG", "ACGAACGTA", "ACGAACGTA", "ACGTACG"],
                              ["CC", "CC", "CA", "CC", "CC", "CC", "CA", "CC"]]),
}


@pytest.mark.parametrize("name", list(BOUNDARY))
@pytest.mark.parametrize("fasta", [True, False], ids=["fa", "fq"])
def test_clusters_that_straddle_cuts(exe, tmp_path, name, fasta):
    mode, d, mates = BOUNDARY[name]
    rng = random.Random(len(name))
    order = list(range(len(mates[0]))) * 2                           # every record twice: ties, in input order
    rng.shuffle(order)
    data = [b"".join(fat(f"r{j}_{k}", m[k], fasta) for j, k in enumerate(order)) for m in mates]
    distinct = len({(s + "\n" * 8)[:8] for s in mates[0]})
    assert distinct >= 3                                             # every case does straddle cuts
    r = both_ways(exe, tmp_path, data, fasta, mode, d, clusters=True, kb=1)
    assert int(LINE.search(r.stderr).group(1)) == distinct           # every key value is a range of its own


def test_one_key_value_beyond_the_target(exe, tmp_path):
    """2000 records that share their first 8 bytes are one range however small the target; the others split around it."""
    rng = random.Random(9)
    recs = []
    for k in range(2600):
        if k % 13 < 10:
            seq = "ACGTACGT" + "".join(rng.choice("ACGT") for _ in range(rng.choice([0, 3, 3, 40])))
        else:
            seq = "".join(rng.choice("ACGT") for _ in range(30))
        recs.append(f"@r{k}\n{seq}\n+\n{'I' * len(seq)}\n".encode())
    r = both_ways(exe, tmp_path, [b"".join(recs)], False, "loose", 0, clusters=True, kb=1)
    assert int(LINE.search(r.stderr).group(2)) > (1 << 10)


# ---------------------------------------------------------------- refusals: the in-core run's message, no output

GOOD = b"".join(f"@r{k}\n{'ACGT'[k % 4] * 9}{'ACGT'[k % 3]}\n+\n{'I' * 10}\n".encode() for k in range(400))


@pytest.mark.parametrize("name,data,needle", [
    ("nul-in-the-last-record", GOOD + b"@z\nAC\x00T\n+\nIIII\n", "below '\\n'"),
    ("truncated-last-record", GOOD + b"@z\nACGT\n+\nII\n", "should have the same length"),
    ("empty", b"", "Not enough memory to read a single object!"),
], ids=["nul-in-the-last-record", "truncated-last-record", "empty"])
def test_refusals_leave_no_output(exe, tmp_path, name, data, needle):
    src = tmp_path / "in.fq"; src.write_bytes(data)
    seen = []
    for env in ({}, {"FQD_SEQ_RANGE_KB": "1"}):
        out = tmp_path / ("o%d.fq" % len(seen))
        r = run(exe, "-i", src, "-o", out, "--compare-seq", "loose", "--write-clusters", env=env)
        assert r.returncode == 1, r.stderr
        assert not out.exists() and not Path(str(out) + ".clusters").exists()
        seen.append(r.stderr)
    assert seen[0] == seen[1]                                        # the in-core run's words
    if needle:
        assert needle in seen[1]


def test_low_byte_behind_the_last_pair_is_not_looked_at(exe, tmp_path):
    """Pairs end with the shorter file: a NUL in a record of the longer file that has no partner refuses neither run."""
    a = GOOD + b"@z\nAC\x00T\n+\nIIII\n"
    both_ways(exe, tmp_path, [a, GOOD], False, "tight", 0, kb=1)


def test_a_pipe_is_refused_by_the_ranged_run_only(exe, tmp_path):
    fifo = tmp_path / "in.fq"
    os.mkfifo(fifo)
    out = tmp_path / "o.fq"

    def feed():
        with open(fifo, "wb") as f:
            try:
                f.write(GOOD)
            except BrokenPipeError:
                pass
    keep_open = os.open(fifo, os.O_RDWR)                            # the run's opens never wait for a writer
    try:
        t = threading.Thread(target=feed)
        t.start()
        r = run(exe, "-i", fifo, "-o", out, "--compare-seq", "tight", env={"FQD_SEQ_RANGE_KB": "64"})
        assert r.returncode == 1
        assert "not a regular file" in r.stderr and "pipe" in r.stderr
        assert not out.exists()
    finally:
        os.close(keep_open)
        t.join(timeout=10)
