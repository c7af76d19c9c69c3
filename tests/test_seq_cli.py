"""The `--compare-seq` modes of the CLI.  CPU part: option handling and the failures that come before any GPU work.
GPU part: the reference's own test_seq.py cases against its fixtures, and a fuzz of the CLI against the restatement
(tests/seq_reference.py): FASTQ / FASTA, SE / PE, every mode, several distances, ragged and empty reads, lowercase and
IUPAC bytes, CRLF, `.gz` (BGZF and ordinary) in and out, files of unequal record counts, cluster files and `-v`."""
import gzip
import os
import random
import subprocess
from pathlib import Path

import pytest

import fastq_dupaway_amd as fqd
from fastq_dupaway_amd import _lib
import seq_reference as ref

FIX = Path(__file__).resolve().parent / "golden" / "reference_seq_fixtures"


@pytest.fixture(scope="module")
def exe():
    if not _lib.CLI_PATH.exists():
        fqd.build_native("all")
    return str(_lib.CLI_PATH)


def run(exe, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([exe, *map(str, args)], capture_output=True, env=e)
    r.stdout = r.stdout.decode("latin-1")
    r.stderr = r.stderr.decode("latin-1")
    return r


# ---------------------------------------------------------------- CPU

def test_compare_seq_with_distance_parses(exe, tmp_path):
    # --distance with tight is accepted and ignored (main.cpp:123-134); the run then fails on the missing input
    r = run(exe, "-i", "/nonexistent/in.fq", "-o", tmp_path / "o.fq", "--compare-seq", "tight", "--distance", "3")
    assert "arguments parsing" not in r.stderr
    assert r.stderr.startswith("Cannot open file /nonexistent/in.fq\n")


def test_bare_invocation_names_compare_seq(exe, tmp_path):
    r = run(exe, "-i", "a", "-o", tmp_path / "b")
    assert r.returncode == 1
    assert "--fast mode only" in r.stderr and "--compare-seq" in r.stderr


@pytest.mark.parametrize("mode", ["tight", "loose", "tail-hamming"])
def test_missing_input_no_output(exe, tmp_path, mode):
    # the reference sorts before it opens an output (seq_dup_remover.hpp:44-50): the missing file's text, no output file
    out = tmp_path / "o.fq"
    r = run(exe, "-i", "/nonexistent/in.fq", "-o", out, "--compare-seq", mode)
    assert r.returncode == 1
    assert r.stderr == ("Cannot open file /nonexistent/in.fq\nAn error occured during fastq-dupaway execution:\n"
                        "File does not exist or cannot be opened!\n")
    assert not out.exists()


def test_missing_second_input_no_output(exe, tmp_path):
    src = tmp_path / "a.fq"; src.write_bytes(b"@r\nACGT\n+\nIIII\n")
    o1, o2 = tmp_path / "o1.fq", tmp_path / "o2.fq"
    r = run(exe, "-i", src, "-u", "/nonexistent/b.fq", "-o", o1, "-p", o2, "--compare-seq", "loose")
    assert r.returncode == 1 and "Cannot open file /nonexistent/b.fq\n" in r.stderr
    assert not o1.exists() and not o2.exists()


def test_help_names_the_modes(exe):
    r = run(exe, "-h")
    assert "tight, loose or tail-hamming" in r.stderr and "does not bound it" in r.stderr


# ---------------------------------------------------------------- GPU: the reference's test_seq.py

@pytest.mark.gpu
@pytest.mark.parametrize("name,args", [
    ("single_tight.fa", ["--format", "fasta", "--compare-seq", "tight"]),
    ("single_loose.fa", ["--format", "fasta", "--compare-seq", "loose"]),
    ("single_hamming.fa", ["--format", "fasta", "--compare-seq", "tail-hamming", "--distance", "1"]),
])
def test_reference_single_fixtures(exe, tmp_path, name, args):
    out = tmp_path / name
    r = run(exe, "-i", FIX / "inputs" / name, "-o", out, *args)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == (FIX / "expected" / name).read_bytes()


@pytest.mark.gpu
def test_reference_paired_fixture(exe, tmp_path):
    ins = [FIX / "inputs" / f"paired_tight_r{k}.fa" for k in (1, 2)]
    outs = [tmp_path / f"paired_tight_r{k}.fa" for k in (1, 2)]
    r = run(exe, "-i", ins[0], "-u", ins[1], "-o", outs[0], "-p", outs[1], "--format", "fasta", "--compare-seq", "tight")
    assert r.returncode == 0, r.stderr
    for k, o in zip((1, 2), outs):
        assert o.read_bytes() == (FIX / "expected" / f"paired_tight_r{k}.fa").read_bytes()


@pytest.mark.gpu
def test_reference_nonmatching_outputs(exe, tmp_path):
    out = tmp_path / "single_tight.fa"
    r = run(exe, "-i", FIX / "inputs" / "single_tight.fa", "-o", out, "--format", "fasta", "--compare-seq", "tight")
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() != (FIX / "expected" / "single_hamming.fa").read_bytes()


# ---------------------------------------------------------------- GPU: fuzz against the restatement

def make_reads(rng, n, fasta, crlf, pool_size=40):
    """Records with many exact and near duplicates, ragged lengths 0-200, lowercase / IUPAC bytes; every record's ID
    and quality are unique, so identical sequences differ elsewhere (compare sequences + multiset there)."""
    alpha = "ACGTNacgtRYKMSWBDHV"
    pool = []
    for _ in range(pool_size):
        L = rng.choice([0, 1, 5, 20, 75, 150, 200, rng.randrange(0, 201)])
        pool.append("".join(rng.choice("ACGT" if rng.random() < 0.8 else alpha) for _ in range(L)))
    recs = []
    for k in range(n):
        s = rng.choice(pool)
        t = rng.random()
        if t < 0.25 and s:                                  # a prefix (loose)
            s = s[:rng.randrange(0, len(s) + 1)]
        elif t < 0.5 and s:                                 # a few substitutions (hamming)
            s = list(s)
            for _ in range(rng.randrange(1, 4)):
                s[rng.randrange(len(s))] = rng.choice("ACGTN")
            s = "".join(s)
        seq = s + ("\r" if crlf else "")
        if fasta:
            recs.append(f">r{k} x\n{seq}\n".encode())
        else:
            recs.append(f"@r{k} x\n{seq}\n+\n{chr(33 + k % 90) * len(seq)}\n".encode())
    return recs


def write(path, data, kind):
    if kind == "plain":
        path.write_bytes(data)
    elif kind == "gz":
        path.write_bytes(gzip.compress(data))
    else:                                                   # BGZF: members of at most 64 KiB with the 'BC' extra field
        import struct, zlib
        out = bytearray()
        for i in range(0, max(len(data), 1), 60000):
            chunk = data[i:i + 60000]
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            comp = c.compress(chunk) + c.flush()
            out += b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25)
            out += comp + struct.pack("<II", zlib.crc32(chunk), len(chunk))
        out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
        path.write_bytes(bytes(out))


def read_out(path):
    data = path.read_bytes()
    return gzip.decompress(data) if str(path).endswith(".gz") else data


def check_same(got, exp, fasta):
    """Byte for byte when identical sequences share their other lines; otherwise the sequence lines in order and the
    multiset of records."""
    if got == exp:
        return
    g, e = ref.parse(got, fasta), ref.parse(exp, fasta)
    assert [x[2] for x in g] == [x[2] for x in e]
    assert sorted(x[0] for x in g) == sorted(x[0] for x in e)


CASES = [
    # (fasta, paired, mode, distance, crlf, in_kind, out_gz, clusters, unequal)
    (False, False, "tight", 2, False, "plain", False, True, False),
    (False, False, "loose", 2, False, "plain", False, True, False),
    (False, False, "tail-hamming", 0, False, "bgzf", False, False, False),
    (False, False, "tail-hamming", 1, True, "plain", True, True, False),
    (False, False, "tail-hamming", 3, False, "gz", False, False, False),
    (True, False, "loose", 2, True, "gz", True, False, False),
    (True, False, "tight", 3, False, "plain", False, False, False),
    (False, True, "tight", 2, False, "plain", False, True, True),
    (False, True, "loose", 2, False, "bgzf", True, True, False),
    (False, True, "tail-hamming", 2, False, "plain", False, True, True),
    (True, True, "loose", 2, True, "plain", False, False, True),
    (True, True, "tail-hamming", 1, False, "gz", True, False, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{'fa' if c[0] else 'fq'}-{'pe' if c[1] else 'se'}-{c[2]}-d{c[3]}-{c[5]}{'-gzout' if c[6] else ''}"
                                             f"{'-crlf' if c[4] else ''}" for c in CASES])
def test_cli_fuzz_against_restatement(exe, tmp_path, case):
    fasta, paired, mode, d, crlf, in_kind, out_gz, clusters, unequal = case
    rng = random.Random(CASES.index(case))
    n = 3000
    files = [make_reads(rng, n, fasta, crlf)]
    if paired:
        files.append(make_reads(rng, n - 137 if unequal else n, fasta, crlf, pool_size=10))
    data = [b"".join(f) for f in files]
    ext = ".fa" if fasta else ".fq"
    ins = [tmp_path / (f"in{k}{ext}" + (".gz" if in_kind != "plain" else "")) for k in range(len(data))]
    outs = [tmp_path / (f"out{k}{ext}" + (".gz" if out_gz else "")) for k in range(len(data))]
    for p, x in zip(ins, data):
        write(p, x, in_kind)
    args = ["-i", ins[0], "-o", outs[0]]
    if paired:
        args += ["-u", ins[1], "-p", outs[1]]
    args += ["--compare-seq", mode, "--distance", d, "-v"]
    if fasta:
        args += ["--format", "fasta"]
    if clusters:
        args += ["--write-clusters"]
    r = run(exe, *args)
    assert r.returncode == 0, r.stderr
    exp_out, exp_cl, total, dups = ref.dedup(data, fasta=fasta, mode=ref.MODES[mode], distance=d)
    assert r.stdout == ref.verbose_line(total, dups, paired)
    for k, o in enumerate(outs):
        check_same(read_out(o), exp_out[k], fasta)
        cl = Path(str(o) + ".clusters")
        assert cl.exists() == clusters
        if clusters:
            got = cl.read_bytes()
            if got != exp_cl[k]:                            # identical sequences may carry their IDs in another order
                assert sorted(got.split(b"\n")) == sorted(exp_cl[k].split(b"\n"))
                assert [x.startswith(b"--") for x in got.split(b"\n")] == [x.startswith(b"--") for x in exp_cl[k].split(b"\n")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["flipped_bit", "bad_record", "good"])
def test_bgzf_input_falls_back_to_the_host_reader(exe, tmp_path, case):
    """A BGZF input of the sequence run goes to HBM as it lies on disk and is inflated and cut there; a damaged member
    or a malformed record sends the file to the host reader, which says what is wrong before any output exists.
    Either way: exactly what the run with FQD_GUNZIP_DEVICE=0 says and leaves behind."""
    from inflate_cases import bgzf
    rng = random.Random(5)
    pool = ["".join(rng.choice("ACGT") for _ in range(rng.randrange(40, 91))) for _ in range(150)]
    recs = []
    for k in range(600):
        s = list(rng.choice(pool))
        if rng.random() < 0.3:                              # a substitution or two near the end (tail-hamming)
            for _ in range(rng.randrange(1, 3)):
                s[rng.randrange(len(s) // 2, len(s))] = rng.choice("ACGT")
        recs.append(f"@r{k} x\n{''.join(s)}\n+\n{chr(33 + k % 90) * len(s)}\n".encode())
    text = b"".join(recs)
    if case == "bad_record":
        cut = text.index(b"\n@", len(text) // 2) + 1
        text = text[:cut] + b"x" + text[cut + 1:]           # a record that does not start with '@'
    z = bgzf(text, level=1)
    if case == "flipped_bit":
        z = bytearray(z); z[len(z) // 2] ^= 0x10; z = bytes(z)
    src = tmp_path / "in.fq.gz"
    src.write_bytes(z)
    runs = {}
    for gunzip in ("1", "0"):
        out = tmp_path / f"out_{gunzip}.fq"
        r = run(exe, "-i", src, "-o", out, "--compare-seq", "tail-hamming", "--distance", 2, "-v",
                env={"FQD_HOST_TIMING": "1", "FQD_GUNZIP_DEVICE": gunzip, "FQD_PGZIP_MIN_MB": "0" if gunzip == "1" else "8"})
        said = "\n".join(l for l in r.stderr.splitlines() if "[host timing]" not in l)
        runs[gunzip] = (r.returncode, r.stdout, said, out.read_bytes() if out.exists() else None)
    assert runs["1"] == runs["0"]
    rc, stdout, said, got = runs["1"]
    if case == "good":
        assert rc == 0, said
        exp_out, _, total, dups = ref.dedup([text], fasta=False, mode=ref.MODES["tail-hamming"], distance=2)
        assert dups > 0
        assert stdout == ref.verbose_line(total, dups, False)
        check_same(got, exp_out[0], False)
    else:
        assert rc != 0
        assert ("corrupt or truncated" if case == "flipped_bit" else "Invalid record start character: x") in said
        assert got is None                                  # the reference sorts before it opens an output


@pytest.mark.gpu
def test_empty_input_is_refused(exe, tmp_path):
    src = tmp_path / "in.fq"; src.write_bytes(b"")
    out = tmp_path / "o.fq"
    r = run(exe, "-i", src, "-o", out, "--compare-seq", "tight")
    assert r.returncode == 1 and r.stderr.endswith("Not enough memory to read a single object!\n")
    assert not out.exists()


@pytest.mark.gpu
def test_nul_byte_is_refused(exe, tmp_path):
    src = tmp_path / "in.fq"; src.write_bytes(b"@a\nAC\x00T\n+\nIIII\n@b\nACGT\n+\nIIII\n")
    out = tmp_path / "o.fq"
    r = run(exe, "-i", src, "-o", out, "--compare-seq", "loose")
    assert r.returncode == 1 and "below '\\n'" in r.stderr
    assert not out.exists()


def test_several_devices_are_refused(exe, tmp_path):
    # refused before any GPU work (the sequence-based run is single-GPU)
    src = tmp_path / "in.fq"; src.write_bytes(b"@a\nACGT\n+\nIIII\n")
    r = run(exe, "-i", src, "-o", tmp_path / "o.fq", "--compare-seq", "tight", env={"FQD_DEVICES": "0,1"})
    assert r.returncode == 1 and "one GPU" in r.stderr
    assert not (tmp_path / "o.fq").exists()
