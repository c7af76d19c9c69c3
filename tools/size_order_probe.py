#!/usr/bin/env python3
"""Stage times of FQD_FAST_SORT=size / FQD_FAST_MINSIZE next to the run with FQD_FAST_SIZEOUT=1 alone.
The input is tools/e2e_bench.py's (its generator, its seed: N single-end reads of 150 bases drawn from a pool of 0.8 N), or
with --skewed one with large clusters, which the other has none of: N reads of 100 bases, read i a copy of sequence
i * U // N of U = 0.75 N random sequences, a quarter of the reads (rng.random(N) < 0.25) redirected to sequence
floor(50 * pareto(1.0)) mod U, then 100 000 reads chosen without replacement redirected to sequence 0, which is poly-G;
numpy's default_rng(1), the draws in that order.
  python tools/size_order_probe.py [--reads N] [--skewed] [--repeat K] [--dir /tmp] [--other-cli PATH]
--other-cli: another build's CLI (the parent commit's), timed with FQD_FAST_SIZEOUT=1 alone in the same alternation.
Prints, per run, the `fast:` lines and the stage clock's lines of FQD_HOST_TIMING=1 that §15 quotes.
"""
import argparse
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

KEEP = ("fast: ", "fast: size filter on the GPU", "fast: abundance order on the GPU", "ordered/resident: dedup on the GPU",
        "ordered/resident: survivors out of HBM", "process: main() took", "processed, out of which", "were not written")


def skewed(path, n):
    rng = np.random.default_rng(1)
    U = int(n * 0.75)
    ids = np.arange(n, dtype=np.int64) * U // n
    copy = rng.random(n) < 0.25
    ids[copy] = (rng.pareto(1.0, int(copy.sum())) * 50).astype(np.int64) % U
    ids[rng.choice(n, min(n, 100_000), replace=False)] = 0
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (U, 100), dtype=np.uint8)]
    bases[0] = ord("G")
    rec = np.empty((n, 216), np.uint8)
    rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
    k = np.arange(n, dtype=np.int64)
    for d in range(9):
        rec[:, 10 - d] = ord("0") + (k % 10); k //= 10
    rec[:, 11] = 10
    rec[:, 12:112] = bases[ids]
    rec[:, 112] = 10; rec[:, 113] = ord("+"); rec[:, 114] = 10
    rec[:, 115:215] = ord("I"); rec[:, 215] = 10
    rec.tofile(path)
    return np.bincount(ids)


def like_e2e_bench(path, n):
    import e2e_bench
    rng = np.random.default_rng(1)
    L = 150
    pool = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=(int(n * 0.8) + 1, L))
    idx = rng.integers(0, len(pool), size=n)
    e2e_bench.write_fastq(path, n, L, rng, idx, pool, "")
    return np.bincount(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--skewed", action="store_true")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--other-cli", default="")
    a = ap.parse_args()
    from fastq_dupaway_amd import _lib
    d = Path(a.dir)
    src, out = d / f"size_order_probe_{os.getpid()}.fq", d / f"size_order_probe_{os.getpid()}.out.fq"
    sizes = (skewed if a.skewed else like_e2e_bench)(src, a.reads)
    sizes = sizes[sizes > 0]
    print(f"input: {'skewed' if a.skewed else 'e2e_bench'}, {a.reads} reads, {src.stat().st_size} bytes, {len(sizes)} clusters, largest {int(sizes.max())}, "
          f"{int((sizes > 255).sum())} above 255 members, {int((sizes == 1).sum())} singletons", flush=True)
    runs = [("SIZEOUT alone", str(_lib.CLI_PATH), {"FQD_FAST_SIZEOUT": "1"}),
            ("SORT=size SIZEOUT", str(_lib.CLI_PATH), {"FQD_FAST_SIZEOUT": "1", "FQD_FAST_SORT": "size"}),
            ("SORT=size MINSIZE=2 SIZEOUT", str(_lib.CLI_PATH), {"FQD_FAST_SIZEOUT": "1", "FQD_FAST_SORT": "size", "FQD_FAST_MINSIZE": "2"})]
    if a.other_cli:
        runs.insert(0, ("SIZEOUT alone, other build", a.other_cli, {"FQD_FAST_SIZEOUT": "1"}))
    try:
        for rep in range(a.repeat):
            for name, cli, env in runs:
                out.unlink(missing_ok=True)
                r = subprocess.run([cli, "-i", str(src), "-o", str(out), "--fast", "-v"], capture_output=True, text=True, timeout=600,
                                   env=dict(os.environ, FQD_HOST_TIMING="1", **env))
                print(f"== {name} ({rep}): rc={r.returncode}, output {out.stat().st_size if out.exists() else None} bytes")
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
