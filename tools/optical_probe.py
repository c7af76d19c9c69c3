#!/usr/bin/env python3
"""Stage times of FQD_FAST_OPTICAL=D next to the run without the switch.
The input has tools/e2e_bench.py's shape (N single-end reads of 150 bases drawn from a pool of 0.8 N, numpy's default_rng(1),
the pool and the draws in that order) under Illumina-style names `@M01:7:FC1:1:<tile>:<x>:<y>`, tile one of 96, x and y nine
digits with leading zeros: a read lands anywhere on a tile (x, y below 100 000), except that three copies in ten of an earlier
read sit within 1 000 pixels of the first read of their sequence, on its tile — the optical duplicates.  With --cap, 65 536
reads chosen without replacement are one sequence more (poly-G) on one tile, a chain in x with steps of D whose first member
in the input comes last: the largest cluster the split takes, at its most sweeps.
  python tools/optical_probe.py [--reads N] [--distance D] [--cap] [--repeat K] [--dir /tmp] [--other-cli PATH]
--other-cli: another build's CLI (the parent commit's), timed without the switch in the same alternation.
Prints, per run, the `fast:` lines and the stage clock's lines of FQD_HOST_TIMING=1 that §17 quotes.
"""
import argparse
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

KEEP = ("fast: ", "ordered/resident: dedup on the GPU", "ordered/resident: survivors out of HBM", "process: main() took", "processed, out of which",
        "not optical duplicates")
L = 150
CAP = 65536


def digits(values, width):
    out = np.empty((len(values), width), np.uint8)
    v = values.astype(np.int64).copy()
    for d in range(width):
        out[:, width - 1 - d] = ord("0") + (v % 10)
        v //= 10
    return out


def flowcell(path, n, distance, cap):
    rng = np.random.default_rng(1)
    pool = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=(int(n * 0.8) + 2, L))
    idx = rng.integers(0, len(pool) - 1, size=n)
    tile = 1101 + rng.integers(0, 96, size=n)
    x, y = rng.integers(0, 100_000, size=n), rng.integers(0, 100_000, size=n)
    _, first = np.unique(idx, return_index=True)
    first_of = np.empty(len(pool), np.int64)
    first_of[np.unique(idx)] = first
    near = (rng.random(n) < 0.3) & (first_of[idx] != np.arange(n))
    f = first_of[idx[near]]
    tile[near] = tile[f]
    x[near] = x[f] + rng.integers(0, 1000, size=int(near.sum()))
    y[near] = y[f] + rng.integers(0, 1000, size=int(near.sum()))
    if cap:
        members = np.sort(rng.choice(n, min(n, CAP), replace=False))
        pool[-1] = ord("G")
        idx[members] = len(pool) - 1
        tile[members] = 2101
        x[members] = 1000 + distance * np.arange(len(members))[::-1]
        y[members] = 500
    head = np.frombuffer(b"@M01:7:FC1:1:", np.uint8)
    w = len(head) + 4 + 1 + 9 + 1 + 9
    with open(path, "wb") as out:
        for a in range(0, n, 500_000):
            m = min(500_000, n - a)
            s = slice(a, a + m)
            rec = np.empty((m, w + 1 + L + 3 + L + 1), np.uint8)
            rec[:, :len(head)] = head
            at = len(head)
            rec[:, at:at + 4] = digits(tile[s], 4); rec[:, at + 4] = ord(":")
            rec[:, at + 5:at + 14] = digits(x[s], 9); rec[:, at + 14] = ord(":")
            rec[:, at + 15:at + 24] = digits(y[s], 9)
            rec[:, w] = 10
            rec[:, w + 1:w + 1 + L] = pool[idx[s]]
            rec[:, w + 1 + L] = 10; rec[:, w + 2 + L] = ord("+"); rec[:, w + 3 + L] = 10
            rec[:, w + 4 + L:w + 4 + 2 * L] = ord("I")
            rec[:, w + 4 + 2 * L] = 10
            out.write(rec.tobytes())
    return np.bincount(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--distance", type=int, default=2500)
    ap.add_argument("--cap", action="store_true")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--other-cli", default="")
    a = ap.parse_args()
    from fastq_dupaway_amd import _lib
    d = Path(a.dir)
    src, out = d / f"optical_probe_{os.getpid()}.fq", d / f"optical_probe_{os.getpid()}.out.fq"
    sizes = flowcell(src, a.reads, a.distance, a.cap)
    sizes = sizes[sizes > 0]
    print(f"input: {a.reads} reads, {src.stat().st_size} bytes, {len(sizes)} clusters, largest {int(sizes.max())}, {int((sizes == 1).sum())} singletons, "
          f"{int(((sizes > 1) & (sizes <= 8)).sum())} of 2 .. 8, {int((sizes > 8).sum())} above 8", flush=True)
    runs = [("no switch", str(_lib.CLI_PATH), {}),
            ("CLUSTERS=1 (linked, not split)", str(_lib.CLI_PATH), {"FQD_FAST_CLUSTERS": "1"}),
            (f"OPTICAL={a.distance}", str(_lib.CLI_PATH), {"FQD_FAST_OPTICAL": str(a.distance)})]
    if a.other_cli:
        runs.insert(0, ("no switch, other build", a.other_cli, {}))
    try:
        for rep in range(a.repeat):
            for name, cli, env in runs:
                out.unlink(missing_ok=True)
                Path(str(out) + ".clusters").unlink(missing_ok=True)
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
        src.unlink(missing_ok=True); out.unlink(missing_ok=True); Path(str(out) + ".clusters").unlink(missing_ok=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
