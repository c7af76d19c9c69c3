#!/usr/bin/env python3
"""What FQD_FAST_STRAND=both adds on the device: times fqd_canonical_reads alone over synthetic reads (fqd_synth_reads,
no duplicates: uniform ACGT with an N now and then), holds a sample of its output against the Python statement
(tests/strand_reference.py) and records, for the same batch on the same run, the encoder's time — over the reads as
given (uniform descriptors) and over the canonical ones (ragged descriptors) — from the engine's own profile.

    python tools/strand_probe.py N LEN se|pe [--repeat 3]

One JSON line per repeat.  With the count asked for the call drains the engine's stream itself, so wall time around it
is its device time plus a few launches and one synchronisation.  bytes_moved = what the kernel has to move: the sequence
bytes read once and written once, plus the descriptors it writes (12 bytes a record and mate, 1 byte a record)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from fastq_dupaway_amd import Engine, Reads  # noqa: E402
import strand_reference as ref  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def encode_ms(segs, S, n, batch, step, keep):
    """(device time of the encoder over the n records, its launches), from the engine's profile (FQD_FLAG_PROFILE), whose
    encode_ms is the SUM over the launches."""
    with Engine(segments=S, capacity_reads=n, profile=True) as e:
        for lo in range(0, n, batch):
            m = min(batch, n - lo)
            e.submit([step(s, lo) for s in segs], m, keep=keep[lo:], final=lo + m == n)
        e.sync()
        p = e.profile()
    return p["encode_ms"], p["encode_launches"]


def check_sample(mates, L, out, offs, lens, flipped, lo, m):
    given = [x[lo * L:(lo + m) * L].cpu().numpy().reshape(m, L) for x in mates]
    got_flip = flipped[lo:lo + m].cpu().numpy()
    at = int(offs[0][lo].item())
    got = out[at:at + len(mates) * m * L].cpu().numpy().reshape(m, len(mates) * L)
    if len(mates) == 1:
        rows, flip = ref.canon_se_rows(given[0])
    else:
        (c0, c1), flip = ref.canon_pe_rows(given[0], given[1])
        rows = np.concatenate([c0, c1], axis=1)
    assert np.array_equal(got, rows), "canonical bytes differ from the statement"
    assert np.array_equal(got_flip, flip), "flipped differs from the statement"
    for s in range(len(mates)):
        exp = (np.arange(lo, lo + m, dtype=np.uint64) * np.uint64(len(mates)) + np.uint64(s)) * np.uint64(L)
        assert np.array_equal(offs[s][lo:lo + m].cpu().numpy().view(np.uint64), exp), "offsets differ"
        assert bool((lens[s][lo:lo + m] == L).all()), "lengths differ"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("length", type=int)
    ap.add_argument("layout", choices=["se", "pe"])
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    n, L, S, batch = a.n, a.length, 2 if a.layout == "pe" else 1, 16 << 20
    mates = [torch.empty(n * L + 64, dtype=torch.uint8, device="cuda") for _ in range(S)]
    out = torch.empty(S * n * L + 64, dtype=torch.uint8, device="cuda")
    offs = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(S)]
    lens = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(S)]
    flipped = torch.empty(n, dtype=torch.uint8, device="cuda")
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    given = [Reads(x, uniform_len=L, uniform_stride=L) for x in mates]
    with Engine(segments=S) as e:
        for s in range(S):
            e.synth_reads(7, 0, n, L, 0, s, mates[s], None)
        e.sync()
        small = min(n, 1 << 16)                                  # first launches load the code objects
        e.canonical_reads(given, small, out, offs[0], lens[0], flipped, offs[1] if S == 2 else None, lens[1] if S == 2 else None, count=True)
        for r in range(a.repeat):
            turned, ms = timed(lambda: e.canonical_reads(given, n, out, offs[0], lens[0], flipped, offs[1] if S == 2 else None,
                                                         lens[1] if S == 2 else None, out_capacity=S * n * L, count=True))
            m = min(n, 50_000)
            check_sample(mates, L, out, offs, lens, flipped, 0, m)
            check_sample(mates, L, out, offs, lens, flipped, n - m, m)
            assert int(flipped.sum().item()) == turned
            moved = 2 * S * n * L + n * (12 * S + 1)
            canon = [Reads(out, offsets=offs[s], lengths=lens[s]) for s in range(S)]
            enc_given = encode_ms(given, S, n, batch, lambda d, lo: Reads(d.bases[lo * L:], uniform_len=L, uniform_stride=L), keep)
            enc_canon = encode_ms(canon, S, n, batch, lambda d, lo: Reads(d.bases, offsets=d.offsets[lo:], lengths=d.lengths[lo:]), keep)
            print(json.dumps({"records": n, "length": L, "layout": a.layout, "turned": turned, "canonical_reads_ms": round(ms, 2),
                              "bytes_moved": moved, "GB_per_s": round(moved / ms / 1e6, 1),
                              "encode_given_uniform_ms": round(enc_given[0], 2), "encode_canonical_ragged_ms": round(enc_canon[0], 2),
                              "encode_launches": [enc_given[1], enc_canon[1]]}), flush=True)


if __name__ == "__main__":
    main()
