#!/usr/bin/env python3
"""Stage time of FQD_FAST_CENTROID=abundant next to the run without the switch, and next to FQD_FAST_KEEP=best's pick — the
nearest existing yardstick: the same segmented pass over the n places.
The input is tools/e2e_bench.py's: N single-end reads of 150 bases drawn from a pool of 0.8 N random reads, every quality
byte 'I'.  Random reads of 150 bases are never near each other, so FQD_FAST_HAMMING=1 merges nothing: the stage runs over
clusters of one sequence each, which is what it costs a run whose merges find little.
  python tools/centroid_probe.py [--reads N] [--repeat K] [--dir /tmp]
Through the CLI with FQD_HOST_TIMING=1, K times each: FQD_FAST_HAMMING=1 alone, with FQD_FAST_CENTROID=abundant, and with
FQD_FAST_KEEP=best: the `fast:` lines, the stage clock's lines of the two picks and main()'s wall time.
"""
import argparse
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import e2e_bench                                               # noqa: E402  (the input's FASTQ file)

KEEP = ("fast: most abundant", "fast: best-quality", "fast: substitutions", "fast: owners and clusters", "reads processed", "were written by", "dedup on the GPU")
L = 150


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--dir", default="/tmp")
    a = ap.parse_args()
    from fastq_dupaway_amd import _lib
    rng = np.random.default_rng(1)
    n = a.reads
    pool = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=(int(n * 0.8) + 1, L))
    idx = rng.integers(0, len(pool), size=n)
    d = Path(a.dir)
    src, out = d / f"centroid_probe_{os.getpid()}.fq", d / f"centroid_probe_{os.getpid()}.out.fq"
    e2e_bench.write_fastq(src, n, L, rng, idx, pool, "")
    del pool, idx
    print(f"input: {n} reads of {L} bases, {src.stat().st_size} bytes", flush=True)
    hamming = {"FQD_FAST_HAMMING": "1"}
    runs = [("HAMMING=1", hamming), ("HAMMING=1 CENTROID=abundant", {**hamming, "FQD_FAST_CENTROID": "abundant"}), ("HAMMING=1 KEEP=best", {**hamming, "FQD_FAST_KEEP": "best"})]
    try:
        for rep in range(a.repeat):
            for name, env in runs:
                out.unlink(missing_ok=True)
                t0 = time.perf_counter()
                r = subprocess.run([str(_lib.CLI_PATH), "-i", str(src), "-o", str(out), "-v", "--fast"], capture_output=True, text=True, timeout=900,
                                   env=dict(os.environ, FQD_HOST_TIMING="1", **env))
                print(f"== {name} ({rep}): rc={r.returncode}, wall {time.perf_counter() - t0:.2f} s, output {out.stat().st_size if out.exists() else None} bytes")
                for line in (r.stdout + r.stderr).splitlines():
                    if any(k in line for k in KEEP):
                        print("   " + line.strip())
                sys.stdout.flush()
                if r.returncode != 0:
                    print(r.stderr[-2000:])
                    return 1
    finally:
        src.unlink(missing_ok=True); out.unlink(missing_ok=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
