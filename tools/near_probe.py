#!/usr/bin/env python3
"""Stage times of FQD_FAST_HAMMING=D next to the run without the switch.
The input has tools/e2e_bench.py's shape (N single-end reads of 150 bases drawn from a pool of 0.8 N, numpy's default_rng(1),
the pool and the draws in that order); then --share of the reads that repeat an earlier one get 1 .. D + 1 substituted bases
at random places (another letter of ACGT), so that most of them are near copies of their sequence and some are not.
  python tools/near_probe.py [--reads N] [--distance D] [--share 0.3] [--repeat K] [--dir /tmp] [--no-cli]
Part 1, through the binding: the reads in GPU memory, fqd_submit_linked + fqd_owners (the engine phase), fqd_near_merge with
its stage_ms (seeds + sort + groups, verification, sweeps) and counts, K times.
Part 2, through the CLI with FQD_HOST_TIMING=1: the run without the switch, the run with it, and `--compare-seq tail-hamming
--distance D` on the same file: the `fast:` lines, the stage clock's lines and main()'s wall time.
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

KEEP = ("fast: ", "ordered/resident: dedup on the GPU", "ordered/resident: survivors out of HBM", "process: main() took", "processed, out of which", "were taken for copies")
L = 150


def reads_with_errors(n, distance, share):
    rng = np.random.default_rng(1)
    pool = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=(int(n * 0.8) + 2, L))
    idx = rng.integers(0, len(pool) - 1, size=n)
    reads = pool[idx]
    _, first = np.unique(idx, return_index=True)
    repeat = np.ones(n, bool)
    repeat[first] = False
    hit = np.nonzero(repeat & (rng.random(n) < share))[0]
    count = rng.integers(1, distance + 2, size=len(hit))
    letters = np.frombuffer(b"ACGT", np.uint8)
    for k in range(distance + 1):                              # the k-th substitution of the reads that get more than k
        rows = hit[count > k]
        at = rng.integers(0, L, size=len(rows))
        old = reads[rows, at]
        reads[rows, at] = letters[(np.searchsorted(letters, old) + rng.integers(1, 4, size=len(rows))) % 4]
    return reads, len(hit)


def write_fastq(path, reads):
    n = len(reads)
    with open(path, "wb") as out:
        for a in range(0, n, 500_000):
            m = min(500_000, n - a)
            names = np.char.add(np.char.add("@r", np.arange(a, a + m).astype(str)), "\n").astype("S")
            rec = np.empty((m, L + 3 + L + 1), np.uint8)
            rec[:, :L] = reads[a:a + m]
            rec[:, L] = 10; rec[:, L + 1] = ord("+"); rec[:, L + 2] = 10
            rec[:, L + 3:L + 3 + L] = ord("I")
            rec[:, L + 3 + L] = 10
            body = rec.tobytes()
            w = rec.shape[1]
            out.write(b"".join(names[k] + body[k * w:(k + 1) * w] for k in range(m)))


def through_the_binding(reads, distance, repeat):
    import torch
    from fastq_dupaway_amd import Engine, Reads
    n = len(reads)
    bases = torch.from_numpy(reads.reshape(-1)).cuda()
    keep, link = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    owner, out = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    seg = [Reads(bases, uniform_len=L, uniform_stride=L)]
    for rep in range(repeat):
        with Engine(segments=1, capacity_reads=n) as e:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for a in range(0, n, 16 << 20):
                m = min(16 << 20, n - a)
                e.submit_linked([Reads(bases[a * L:], uniform_len=L, uniform_stride=L)], m, keep[a:], link[a:], last=a + m >= n)
            e.sync()
            t1 = time.perf_counter()
            e.owners(keep, link, n, owner)
            e.sync()
            t2 = time.perf_counter()
            info = e.near_merge(seg, owner, n, distance, out)
            t3 = time.perf_counter()
        ms = [round(x, 2) for x in info.stage_ms]
        print(f"binding ({rep}): engine {1e3 * (t1 - t0):.1f} ms, owners {1e3 * (t2 - t1):.1f} ms, near_merge {1e3 * (t3 - t2):.1f} ms = seeds+sort+groups {ms[0]} + verify {ms[1]} "
              f"+ sweeps {ms[2]} ms; nodes {info.nodes}, merged clusters {info.merged}, entries {info.entries}, groups {info.groups}, largest group {info.largest_group}, "
              f"pairs {info.pairs} ({info.pairs / max(info.nodes, 1):.3f} a node), edges {info.edges}, sweeps {info.sweeps}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--distance", type=int, default=2)
    ap.add_argument("--share", type=float, default=0.3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--no-cli", action="store_true")
    a = ap.parse_args()
    from fastq_dupaway_amd import _lib
    reads, hit = reads_with_errors(a.reads, a.distance, a.share)
    print(f"input: {a.reads} reads of {L} bases, {hit} repeats with 1 .. {a.distance + 1} substituted bases", flush=True)
    through_the_binding(reads, a.distance, a.repeat)
    if a.no_cli:
        return 0
    d = Path(a.dir)
    src, out = d / f"near_probe_{os.getpid()}.fq", d / f"near_probe_{os.getpid()}.out.fq"
    write_fastq(src, reads)
    del reads
    runs = [("no switch", ["--fast"], {}),
            (f"HAMMING={a.distance}", ["--fast"], {"FQD_FAST_HAMMING": str(a.distance)}),
            (f"--compare-seq tail-hamming --distance {a.distance}", ["--compare-seq", "tail-hamming", "--distance", str(a.distance)], {})]
    try:
        for rep in range(a.repeat):
            for name, args, env in runs:
                out.unlink(missing_ok=True)
                t0 = time.perf_counter()
                r = subprocess.run([str(_lib.CLI_PATH), "-i", str(src), "-o", str(out), "-v", *args], capture_output=True, text=True, timeout=900,
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
