#!/usr/bin/env python3
"""Stage times of FQD_FAST_HAMMING=D next to the run without the switch.
The input has tools/e2e_bench.py's shape (N single-end reads of 150 bases drawn from a pool of 0.8 N, numpy's default_rng(1),
the pool and the draws in that order); then --share of the reads that repeat an earlier one get 1 .. D + 1 substituted bases
at random places (another letter of ACGT), so that most of them are near copies of their sequence and some are not.
  python tools/near_probe.py [--reads N] [--distance D] [--share 0.3] [--repeat K] [--dir /tmp] [--no-cli] [--umi BASES]
Part 1, through the binding: the reads in GPU memory, fqd_submit_linked + fqd_owners (the engine phase), fqd_near_merge with
its stage_ms (seeds + sort + groups, verification, sweeps) and counts, K times.
Part 2, through the CLI with FQD_HOST_TIMING=1: the run without the switch, the run with it, and `--compare-seq tail-hamming
--distance D` on the same file: the `fast:` lines, the stage clock's lines and main()'s wall time.
--umi BASES: every fragment of the pool gets a random UMI of that many bases, which its copies carry in their names
(`@r<k>:<UMI>`).  Part 1 then times fqd_near_merge_umi — fqd_umi_find, fqd_umi_reads, the engine keyed `UMI ‖ sequence`, its
owners — next to fqd_near_merge on the same reads, one after the other in every repetition; part 2 runs FQD_FAST_UMI=colon
without and with FQD_FAST_UMI_HAMMING=D in place of the FQD_FAST_HAMMING run.
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


def reads_with_errors(n, distance, share, umi_bases=0):
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
    umis = None
    if umi_bases:                                              # (drawn last: the reads are those of the run without --umi)
        umis = rng.choice(letters, size=(len(pool), umi_bases))[idx]
    return reads, len(hit), umis


def write_fastq(path, reads, umis=None):
    n = len(reads)
    with open(path, "wb") as out:
        for a in range(0, n, 500_000):
            m = min(500_000, n - a)
            names = np.char.add("@r", np.arange(a, a + m).astype(str))
            if umis is not None:
                names = np.char.add(np.char.add(names, ":"), umis[a:a + m].copy().view(f"S{umis.shape[1]}").ravel().astype(str))
            names = np.char.add(names, "\n").astype("S")
            rec = np.empty((m, L + 3 + L + 1), np.uint8)
            rec[:, :L] = reads[a:a + m]
            rec[:, L] = 10; rec[:, L + 1] = ord("+"); rec[:, L + 2] = 10
            rec[:, L + 3:L + 3 + L] = ord("I")
            rec[:, L + 3 + L] = 10
            body = rec.tobytes()
            w = rec.shape[1]
            out.write(b"".join(names[k] + body[k * w:(k + 1) * w] for k in range(m)))


def names_on_device(umis):
    """ID lines `@:<UMI>\n` of one width in GPU memory: (text, id_start, id_len)."""
    import torch
    n, width = len(umis), umis.shape[1] + 3
    lines = np.empty((n, width), np.uint8)
    lines[:, 0] = ord("@"); lines[:, 1] = ord(":"); lines[:, 2:-1] = umis; lines[:, -1] = 10
    return (torch.from_numpy(lines.reshape(-1)).cuda(), torch.arange(n, dtype=torch.int64, device="cuda") * width,
            torch.full((n,), width, dtype=torch.int32, device="cuda"))


def through_the_binding(reads, distance, repeat, umis=None):
    import torch
    from fastq_dupaway_amd import Engine, Reads
    n = len(reads)
    bases = torch.from_numpy(reads.reshape(-1)).cuda()
    if umis is not None:
        text, id_start, id_len = names_on_device(umis)
        umi_off = torch.empty(n, dtype=torch.int32, device="cuda")
        keyed = torch.empty(n * (L + umis.shape[1]) + 64, dtype=torch.uint8, device="cuda")
        keyed_off, keyed_len = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
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
        if umis is None:
            continue
        with Engine(segments=1, capacity_reads=n, capacity_bases=n * (L + umis.shape[1])) as e:      # the same reads, keyed UMI ‖ sequence
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            found = e.umi_find(text, id_start, id_len, n, ":", umi_off)
            e.umi_reads(text, id_start, umi_off, found, seg[0], n, keyed, keyed_off, keyed_len)
            e.sync()
            t1 = time.perf_counter()
            for a in range(0, n, 16 << 20):
                m = min(16 << 20, n - a)
                e.submit_linked([Reads(keyed, keyed_off[a:], keyed_len[a:])], m, keep[a:], link[a:], last=a + m >= n)
            e.sync()
            t2 = time.perf_counter()
            e.owners(keep, link, n, owner)
            e.sync()
            t3 = time.perf_counter()
            got = e.near_merge_umi(seg, owner, None, n, distance, text, id_start, umi_off, found, out)
            t4 = time.perf_counter()
        info = got.near
        ms = [round(x, 2) for x in info.stage_ms]
        print(f"binding, UMI ({rep}): find+pack {1e3 * (t1 - t0):.1f} ms, engine {1e3 * (t2 - t1):.1f} ms, owners {1e3 * (t3 - t2):.1f} ms, near_merge_umi {1e3 * (t4 - t3):.1f} ms = "
              f"seeds+sort+groups {ms[0]} + verify {ms[1]} + sweeps {ms[2]} ms; nodes {info.nodes}, molecules {info.merged}, entries {info.entries}, groups {info.groups}, "
              f"largest group {info.largest_group}, pairs {info.pairs} ({info.pairs / max(info.nodes, 1):.3f} a node), edges {info.edges}, links {got.links}, sweeps {info.sweeps}",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--distance", type=int, default=2)
    ap.add_argument("--share", type=float, default=0.3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--umi", type=int, default=0, metavar="BASES", help="a random UMI of that many bases a fragment, in every copy's name; times fqd_near_merge_umi as well")
    a = ap.parse_args()
    from fastq_dupaway_amd import _lib
    reads, hit, umis = reads_with_errors(a.reads, a.distance, a.share, a.umi)
    print(f"input: {a.reads} reads of {L} bases, {hit} repeats with 1 .. {a.distance + 1} substituted bases" + (f", a UMI of {a.umi} bases a fragment" if a.umi else ""), flush=True)
    through_the_binding(reads, a.distance, a.repeat, umis)
    if a.no_cli:
        return 0
    d = Path(a.dir)
    src, out = d / f"near_probe_{os.getpid()}.fq", d / f"near_probe_{os.getpid()}.out.fq"
    write_fastq(src, reads, umis)
    del reads
    runs = [("no switch", ["--fast"], {}),
            (f"HAMMING={a.distance}", ["--fast"], {"FQD_FAST_HAMMING": str(a.distance)}),
            (f"--compare-seq tail-hamming --distance {a.distance}", ["--compare-seq", "tail-hamming", "--distance", str(a.distance)], {})]
    if a.umi:
        runs = [("no switch", ["--fast"], {}), ("UMI=colon", ["--fast"], {"FQD_FAST_UMI": "colon"}),
                (f"UMI=colon UMI_HAMMING={a.distance}", ["--fast"], {"FQD_FAST_UMI": "colon", "FQD_FAST_UMI_HAMMING": str(a.distance)})]
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
