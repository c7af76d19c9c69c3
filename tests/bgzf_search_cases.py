"""Inputs and the CPU harness shared by the CPU and GPU tests of the device BGZF coder's search mode."""
import subprocess
import zlib
from pathlib import Path

import numpy as np

from bgzf_cases import cases

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "bgzf_search_check.cpp"
EXE = HERE / "native" / "bgzf_search_check"
CORES = [HERE.parent / "fastq-dupaway_amd" / "csrc" / n for n in ("fqd_bgzf_core.hpp", "fqd_bgzf_search_core.hpp")]
MEMBER = 65280
FAST, HIGH = 0, 1


def build_harness():
    if not EXE.exists() or EXE.stat().st_mtime < max(p.stat().st_mtime for p in [SRC, *CORES]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-o", str(EXE), str(SRC)], check=True, capture_output=True)
    return EXE


def harness_bgzf(data: bytes, lines_per_record: int, effort: int, tmp_path, timeout=None) -> bytes:
    src, out = tmp_path / "in.bin", tmp_path / "out.gz"
    src.write_bytes(data)
    r = subprocess.run([str(build_harness()), str(src), str(out), str(lines_per_record), str(effort)], check=True, capture_output=True, text=True,
                       timeout=timeout)
    members, stored, size = map(int, r.stdout.split())
    raw = out.read_bytes()
    assert len(raw) == size and members == -(-len(data) // MEMBER)
    return raw


def binned_text(n, seed=3):
    """Illumina IDs, bases ACGT, qualities as current sequencers bin them: nine in ten 'F'."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=150).tobytes()
        qual = rng.choice(np.frombuffer(b"F:,#", dtype=np.uint8), size=150, p=[.90, .06, .03, .01]).tobytes()
        head = b"@A00123:45:HXXXXXXX:%d:%d:%d:%d 1:N:0:ACGTACGT" % (1 + i % 4, 1101 + i // 5000, int(rng.integers(1000, 33000)), int(rng.integers(1000, 40000)))
        out.append(head + b"\n" + seq + b"\n+\n" + qual + b"\n")
    return b"".join(out)


def zlib_per_member(data: bytes, level: int) -> int:
    """What bgzip would write at this level: every 65280-byte piece as a raw deflate stream of its own plus 26 bytes of framing."""
    total = 0
    for at in range(0, len(data), MEMBER):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(data[at:at + MEMBER]) + c.flush()) + 26
    return total


def search_cases():
    rng = np.random.default_rng(17)
    rnd = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    far = rnd(40_000)
    yield "repeat_beyond_32768", far * 3, 4                       # the only match lies 40 000 back: it must not be emitted
    yield "repeat_20000", rnd(20_000) * 4, 4                      # long matches, cut and cut again
    yield "period_3", b"abc" * 50_000, 4
    yield "period_5", b"abcde" * 30_000, 4
    tail = rnd(3_000)
    yield "match_ends_on_last_byte", rnd(10_000) + tail + rnd(5_000) + tail, 4
    block = rnd(600)
    yield "repeat_straddles_member_boundary", rnd(MEMBER - 900) + block + block + block + rnd(2_000), 4
    yield "one_bucket", b"ABCD" * 40_000, 4
    yield "text_lines", b"".join(b"line %d of some ordinary text, with words that come back\n" % (i % 97) for i in range(6000)), 4


def all_cases():
    yield from cases()
    yield from search_cases()
