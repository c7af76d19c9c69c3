#!/usr/bin/env python3
"""Stage times of FQD_FAST_PREFIX=L next to the run without the switch.
The input has tools/e2e_bench.py's shape (N single-end reads of 150 bases drawn from a pool of 0.8 N, numpy's default_rng(1),
the pool and the draws in that order); then every read is cut to a random length in --shortest .. 150, so that the copies of
a fragment are prefixes of its longest copy.
  python tools/prefix_probe.py [--reads N] [--overlap L] [--shortest 100] [--repeat K] [--dir /tmp] [--no-cli]
Part 1, through the binding: the reads in GPU memory, fqd_submit_linked + fqd_owners (the engine phase), fqd_prefix_merge with
its stage_ms (seeds + sort + groups, verification, trees) and counts, K times.
Part 2, through the CLI with FQD_HOST_TIMING=1: the run without the switch and the run with it on the same file: the `fast:`
lines, the stage clock's lines and main()'s wall time.
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
FULL = 150


def cut_reads(n, shortest):
    rng = np.random.default_rng(1)
    pool = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=(int(n * 0.8) + 1, FULL))
    idx = rng.integers(0, len(pool), size=n)
    lens = rng.integers(shortest, FULL + 1, size=n).astype(np.uint32)
    return pool[idx], lens


def write_fastq(path, reads, lens):
    n = len(reads)
    with open(path, "wb") as out:
        for a in range(0, n, 500_000):
            m = min(500_000, n - a)
            ids = np.char.add(b"@r", np.char.zfill(np.arange(a, a + m).astype("S9"), 9))
            rec = np.empty((m, 11 + 1 + FULL + 3 + FULL + 1), np.uint8)
            rec[:, :11] = np.frombuffer(b"".join(ids.tolist()), np.uint8).reshape(m, 11)
            rec[:, 11] = 10
            rec[:, 12:12 + FULL] = reads[a:a + m]
            rec[:, 12 + FULL] = 10; rec[:, 13 + FULL] = ord("+"); rec[:, 14 + FULL] = 10
            rec[:, 15 + FULL:15 + 2 * FULL] = ord("I")
            rec[:, 15 + 2 * FULL] = 10
            keep = np.ones(rec.shape, bool)
            beyond = np.arange(FULL)[None, :] >= lens[a:a + m, None]
            keep[:, 12:12 + FULL] = ~beyond
            keep[:, 15 + FULL:15 + 2 * FULL] = ~beyond
            out.write(rec[keep].tobytes())


def through_the_binding(reads, lens, overlap, repeat):
    import torch
    from fastq_dupaway_amd import Engine, Reads
    n = len(reads)
    offs = np.zeros(n, np.uint64)
    np.cumsum(lens[:-1], out=offs[1:])
    packed = reads[np.arange(FULL)[None, :] < lens[:, None]]
    bases = torch.from_numpy(np.concatenate([packed, np.zeros(16, np.uint8)])).cuda()
    d_off, d_len = torch.from_numpy(offs.view(np.int64)).cuda(), torch.from_numpy(lens.view(np.int32)).cuda()
    keep, link = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    owner, out = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    seg = [Reads(bases, d_off, d_len)]
    for rep in range(repeat):
        with Engine(segments=1, capacity_reads=n, capacity_bases=int(lens.sum())) as e:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for a in range(0, n, 16 << 20):
                m = min(16 << 20, n - a)
                e.submit_linked([Reads(bases, d_off[a:], d_len[a:])], m, keep[a:], link[a:], last=a + m >= n)
            e.sync()
            t1 = time.perf_counter()
            e.owners(keep, link, n, owner)
            e.sync()
            t2 = time.perf_counter()
            info = e.prefix_merge(seg, owner, n, overlap, out)
            t3 = time.perf_counter()
        ms = [round(x, 2) for x in info.stage_ms]
        print(f"binding ({rep}): engine {1e3 * (t1 - t0):.1f} ms, owners {1e3 * (t2 - t1):.1f} ms, prefix_merge {1e3 * (t3 - t2):.1f} ms = seeds+sort+groups {ms[0]} + verify {ms[1]} "
              f"+ trees {ms[2]} ms; nodes {info.nodes}, eligible {info.eligible}, merged clusters {info.merged}, groups {info.groups}, largest group {info.largest_group}, "
              f"pairs {info.pairs} ({info.pairs / max(info.nodes, 1):.3f} a node), related {info.related}, children {info.children}, deepest {info.deepest}, jumps {info.jumps}",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--shortest", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--no-cli", action="store_true")
    a = ap.parse_args()
    from fastq_dupaway_amd import _lib
    reads, lens = cut_reads(a.reads, a.shortest)
    print(f"input: {a.reads} reads cut to {a.shortest} .. {FULL} bases, {int(lens.sum())} bases in all", flush=True)
    through_the_binding(reads, lens, a.overlap, a.repeat)
    if a.no_cli:
        return 0
    d = Path(a.dir)
    src, out = d / f"prefix_probe_{os.getpid()}.fq", d / f"prefix_probe_{os.getpid()}.out.fq"
    write_fastq(src, reads, lens)
    del reads
    runs = [("no switch", {}), (f"PREFIX={a.overlap}", {"FQD_FAST_PREFIX": str(a.overlap)})]
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
