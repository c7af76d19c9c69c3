#!/usr/bin/env python3
"""Stage time of FQD_FAST_CONSENSUS=1 next to the run without the switch.
The input is tools/near_probe.py's: N single-end reads of 150 bases drawn from a pool of 0.8 N, --share of the repeats with
1 .. D + 1 substituted bases, every quality byte 'I'.
  python tools/consensus_probe.py [--reads N] [--distance D] [--share 0.3] [--repeat K] [--dir /tmp] [--no-cli]
Part 1, through the binding: the reads as FASTQ records of one size in GPU memory (names of 8 digits), fqd_submit_linked +
fqd_owners + fqd_near_merge + fqd_group_owners for the clusters, then fqd_consensus over a fresh copy of the text, K times: the
call's wall time (it returns after the stream has drained), its counts, the sequence and quality bytes of the members it read
and the rate they make.
Part 2, through the CLI with FQD_HOST_TIMING=1: FQD_FAST_HAMMING=D without and with the switch on the same file: the `fast:`
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
sys.path.insert(0, str(ROOT / "tools"))

import near_probe                                              # noqa: E402  (the input and its FASTQ file)

KEEP = near_probe.KEEP + ("were replaced by",)
L = near_probe.L
NAME = 10                                                      # '@', 8 digits, '\n'
REC = NAME + L + 3 + L + 1


def records_on_device(reads):
    """(text, start, size, seq_off, seq_len) on the device: record k is `@<k in 8 digits>\\n<bases>\\n+\\n<I x 150>\\n`."""
    import torch
    n = len(reads)
    text = torch.empty((n, REC), dtype=torch.uint8, device="cuda")
    k = torch.arange(n, device="cuda")
    text[:, 0] = ord("@")
    for d in range(8):
        text[:, 8 - d] = (48 + (k // 10 ** d) % 10).to(torch.uint8)
    text[:, NAME - 1] = 10
    text[:, NAME:NAME + L] = torch.from_numpy(reads).cuda()
    text[:, NAME + L] = 10; text[:, NAME + L + 1] = ord("+"); text[:, NAME + L + 2] = 10
    text[:, NAME + L + 3:NAME + L + 3 + L] = ord("I")
    text[:, REC - 1] = 10
    start = k * REC
    return (text.reshape(-1), start, torch.full((n,), REC, dtype=torch.int32, device="cuda"), start + NAME, torch.full((n,), L, dtype=torch.int32, device="cuda"))


def through_the_binding(reads, distance, repeat):
    import torch
    from fastq_dupaway_amd import Engine, Reads
    n = len(reads)
    text, start, size, seq_off, seq_len = records_on_device(reads)
    keep, link = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    owner, merged = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    perm, head = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    seg = [Reads(text, seq_off, seq_len)]
    with Engine(segments=1, capacity_reads=n) as e:
        for a in range(0, n, 16 << 20):
            m = min(16 << 20, n - a)
            e.submit_linked([Reads(text, seq_off[a:], seq_len[a:])], m, keep[a:], link[a:], last=a + m >= n)
        e.sync()
        e.owners(keep, link, n, owner)
        e.near_merge(seg, owner, n, distance, merged)
        clusters = e.group_owners(merged, n, perm, head)
        e.sync()
        print(f"binding: {n} records in {clusters} clusters", flush=True)
        for rep in range(repeat):
            work = text.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = e.consensus(perm, head, n, work, start, size, seq_off, seq_len)
            ms = 1e3 * (time.perf_counter() - t0)
            read = 2 * L * info.members
            print(f"binding ({rep}): consensus {ms:.2f} ms; {info.clusters} clusters of {info.members} records voted, largest {info.largest}, {info.bases_changed} bases in "
                  f"{info.reads_changed} reads replaced; {read} sequence and quality bytes read, {read / ms / 1e6:.1f} GB/s", flush=True)
            del work


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
    reads, hit, _ = near_probe.reads_with_errors(a.reads, a.distance, a.share)
    print(f"input: {a.reads} reads of {L} bases, {hit} repeats with 1 .. {a.distance + 1} substituted bases", flush=True)
    through_the_binding(reads, a.distance, a.repeat)
    if a.no_cli:
        return 0
    d = Path(a.dir)
    src, out = d / f"consensus_probe_{os.getpid()}.fq", d / f"consensus_probe_{os.getpid()}.out.fq"
    near_probe.write_fastq(src, reads)
    del reads
    runs = [(f"HAMMING={a.distance}", {"FQD_FAST_HAMMING": str(a.distance)}),
            (f"HAMMING={a.distance} CONSENSUS=1", {"FQD_FAST_HAMMING": str(a.distance), "FQD_FAST_CONSENSUS": "1"})]
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
