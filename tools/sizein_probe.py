#!/usr/bin/env python3
"""Stage times of FQD_FAST_SIZEIN=1 next to the run with FQD_FAST_SIZEOUT=1 alone.  The input is
tools/e2e_bench.py's (its generator, its seed: N single-end reads of 150 bases drawn from a pool of 0.8 N).  A round is: the
run with FQD_FAST_SIZEOUT=1 over the input, whose output is kept; FQD_FAST_SIZEIN=1 FQD_FAST_SIZEOUT=1 over that output, every
record of which carries `;size=N` (and whose output must be that input again, byte for byte); and FQD_FAST_SIZEIN=1
FQD_FAST_SIZEOUT=1 over the input itself, which carries no annotation: the same records as the first run through the new
kernels.
  python tools/sizein_probe.py [--reads N] [--repeat K] [--dir /tmp] [--other-cli PATH]
--other-cli: another build's CLI (the parent commit's), timed with FQD_FAST_SIZEOUT=1 alone in the same alternation.
Prints, per run, the `fast:` lines and the stage clock's lines of FQD_HOST_TIMING=1 that §16 quotes.
"""
import argparse
import filecmp
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

KEEP = ("fast: ", "ordered/resident: dedup on the GPU", "ordered/resident: survivors out of HBM", "process: main() took", "processed, out of which")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--other-cli", default="")
    a = ap.parse_args()
    from fastq_dupaway_amd import _lib
    import size_order_probe
    d = Path(a.dir)
    src, derep, out = (d / f"sizein_probe_{os.getpid()}{x}.fq" for x in ("", ".derep", ".out"))
    sizes = size_order_probe.like_e2e_bench(src, a.reads)
    sizes = sizes[sizes > 0]
    print(f"input: e2e_bench, {a.reads} reads, {src.stat().st_size} bytes, {len(sizes)} clusters, largest {int(sizes.max())}", flush=True)
    here = str(_lib.CLI_PATH)
    both = {"FQD_FAST_SIZEIN": "1", "FQD_FAST_SIZEOUT": "1"}
    runs = [("SIZEOUT alone", here, {"FQD_FAST_SIZEOUT": "1"}, src, derep),
            ("SIZEIN SIZEOUT on that output", here, both, derep, out),
            ("SIZEIN SIZEOUT on the input", here, both, src, out)]
    if a.other_cli:
        runs.insert(0, ("SIZEOUT alone, other build", a.other_cli, {"FQD_FAST_SIZEOUT": "1"}, src, out))
    try:
        for rep in range(a.repeat):
            for name, cli, env, source, target in runs:
                target.unlink(missing_ok=True)
                r = subprocess.run([cli, "-i", str(source), "-o", str(target), "--fast", "-v"], capture_output=True, text=True, timeout=600,
                                   env=dict(os.environ, FQD_HOST_TIMING="1", **env))
                print(f"== {name} ({rep}): rc={r.returncode}, output {target.stat().st_size if target.exists() else None} bytes")
                for line in (r.stdout + r.stderr).splitlines():
                    if any(k in line for k in KEEP):
                        print("   " + line.strip())
                if r.returncode != 0:
                    print(r.stderr[-2000:])
                    return 1
                if source == derep:
                    print(f"   reproduces its input: {filecmp.cmp(derep, out, shallow=False)}")
                elif target == out and not (a.other_cli and cli == a.other_cli):
                    print(f"   equals the run with SIZEOUT alone: {filecmp.cmp(derep, out, shallow=False)}")
                sys.stdout.flush()
    finally:
        for f in (src, derep, out):
            f.unlink(missing_ok=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
