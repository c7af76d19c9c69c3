#!/usr/bin/env python3
"""The ranged `--compare-seq` run against the in-core run on the same input: 20 M x 150 bp single-end FASTQ (about 6.6 GB
of text), once in core and once with an FQD_SEQ_RANGE_KB that gives about 4 ranges.  The outputs must be byte-identical;
the stage times of both runs (FQD_HOST_TIMING) are appended to profiles/seq_ranged_probe.jsonl.  No threshold is set:
nobody has measured this path.  The figure to write beside the result is the in-core time of the commit before the ranged
run existed, on the same input (--label names what was measured).

  python tools/seq_ranged_probe.py [--reads 20000000] [--ranges 4] [--mode tight] [--dir /dev/shm] [--label TEXT]"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from fastq_dupaway_amd import _lib                            # noqa: E402

STAGE = re.compile(r"^\[host timing\] (.+?)\s+([0-9.]+) s\s+\((\d+)\)$", re.M)
LINE = re.compile(r"^sequence: ranged run, (\d+) ranges, largest (\d+) bytes$", re.M)


def write_input(path, reads, length, dup, seed):
    rng = np.random.default_rng(seed)
    chunk = 1_000_000
    acgt = np.frombuffer(b"ACGT", np.uint8)
    qual = b"I" * length
    with open(path, "wb") as f:
        done = 0
        pool = rng.choice(acgt, size=(chunk, length))
        while done < reads:
            n = min(chunk, reads - done)
            seqs = rng.choice(acgt, size=(n, length))
            copies = rng.random(n) < dup                       # duplicates of an earlier chunk's reads
            seqs[copies] = pool[rng.integers(0, len(pool), int(copies.sum()))]
            pool = seqs if n == chunk else pool
            f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (done + k, seqs[k].tobytes(), qual) for k in range(n)))
            done += n


def digest(path):
    h = hashlib.blake2b()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--dup", type=float, default=0.2)
    ap.add_argument("--ranges", type=int, default=4)
    ap.add_argument("--mode", default="tight")
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    work = Path(a.dir) / f"seq_ranged_probe_{os.getpid()}"
    work.mkdir(parents=True)
    src = work / "in.fq"
    try:
        write_input(src, a.reads, a.length, a.dup, 1)
        size = src.stat().st_size
        target_kb = max(1, -(-size // a.ranges) >> 10)
        result = {"reads": a.reads, "length": a.length, "mode": a.mode, "input_bytes": size, "label": a.label}
        sums = {}
        for how, env in (("in_core", {}), ("ranged", {"FQD_SEQ_RANGE_KB": str(target_kb)})):
            out = work / f"{how}.fq"
            t0 = time.perf_counter()
            r = subprocess.run([str(_lib.CLI_PATH), "-i", str(src), "-o", str(out), "--compare-seq", a.mode, "-v"], capture_output=True, text=True,
                               env=dict(os.environ, FQD_HOST_TIMING="1", **env))
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                sys.exit(f"{how}: exit {r.returncode}\n{r.stderr}")
            sums[how] = digest(out)
            result[how] = {"wall_s": round(wall, 3), "verbose": r.stdout.strip(),
                           "stages": {m.group(1).strip(): float(m.group(2)) for m in STAGE.finditer(r.stderr)}}
            m = LINE.search(r.stderr)
            if m:
                result[how].update(ranges=int(m.group(1)), largest_bytes=int(m.group(2)), target_kb=target_kb)
            out.unlink()
        result["identical"] = sums["in_core"] == sums["ranged"] and result["in_core"]["verbose"] == result["ranged"]["verbose"]
        prof = ROOT / "profiles" / "seq_ranged_probe.jsonl"
        with open(prof, "a") as f:
            f.write(json.dumps(result) + "\n")
        print(json.dumps(result))
        if not result["identical"]:
            sys.exit("the ranged run's output differs from the in-core run's")
    finally:
        for p in work.glob("*"):
            p.unlink()
        work.rmdir()


if __name__ == "__main__":
    main()
