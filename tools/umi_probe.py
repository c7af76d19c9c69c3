#!/usr/bin/env python3
"""What FQD_FAST_UMI adds on the device: times fqd_umi_find and fqd_umi_reads alone over synthetic reads (fqd_synth_reads,
no duplicates, the records tools/strand_probe.py times fqd_canonical_reads over) under ID lines of bcl-convert's form with
an 8-base UMI behind the last colon, holds a sample of the output against the Python statement (tests/umi_reference.py)
and records, for the same batch on the same run, the encoder's time — over the reads as given (uniform descriptors) and
over the keyed ones (ragged descriptors) — from the engine's own profile.

    python tools/umi_probe.py N LEN se|pe [--repeat 3]

One JSON line per repeat.  fqd_umi_find drains the engine's stream itself; fqd_umi_reads is timed with a synchronisation
behind it, so wall time round either is its device time plus a few launches and one synchronisation.  Bytes the two calls
have to move: find — the ID lines read once, 12 bytes of descriptors read and 4 written a record; reads — mate 1's
sequence bytes read once and written once, the UMI bases read and written, 12 bytes a record read (ID start, UMI offset)
and 12 written (offset, length).  pe: mate 2 is not touched by either call; it only enters the encoder's times."""
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
import umi_reference as ref  # noqa: E402

HEAD, TAIL, DIGITS, UMI = b"@A00:7:", b" 1:N:0:ATCACG\n", 9, 8


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


def id_lines(n):
    """n ID lines "@A00:7:<9 digits>:<8 bases> 1:N:0:ATCACG\\n" of one width, built on the device; returns (text, width, UMI offset)."""
    W = len(HEAD) + DIGITS + 1 + UMI + len(TAIL)
    text = torch.empty((n, W), dtype=torch.uint8, device="cuda")
    text[:, :len(HEAD)] = torch.frombuffer(bytearray(HEAD), dtype=torch.uint8).cuda()
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    for d in range(DIGITS):
        text[:, len(HEAD) + DIGITS - 1 - d] = ((idx // 10 ** d) % 10 + ord("0")).to(torch.uint8)
    del idx
    at = len(HEAD) + DIGITS
    text[:, at] = ord(":")
    letters = torch.frombuffer(bytearray(b"ACGT"), dtype=torch.uint8).cuda()
    gen = torch.Generator(device="cuda").manual_seed(11)
    step = 1 << 24
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        text[lo:hi, at + 1:at + 1 + UMI] = letters[torch.randint(0, 4, (hi - lo, UMI), device="cuda", generator=gen)]
    text[:, at + 1 + UMI:] = torch.frombuffer(bytearray(TAIL), dtype=torch.uint8).cuda()
    return text.reshape(-1), W, at + 1


def check_sample(text, W, umi_at, mate, L, umi_off, out, off, ln, lo, m):
    lines = text[lo * W:(lo + m) * W].cpu().numpy().reshape(m, W)
    assert ref.umi_of(lines[0].tobytes(), b":") == (umi_at, lines[0, umi_at:umi_at + UMI].tobytes())
    seqs = mate[lo * L:(lo + m) * L].cpu().numpy().reshape(m, L)
    at = int(off[lo].item())
    got = out[at:at + m * (UMI + L)].cpu().numpy().reshape(m, UMI + L)
    assert np.array_equal(got, np.concatenate([lines[:, umi_at:umi_at + UMI], seqs], axis=1)), "keyed bytes differ from the statement"
    assert bool((umi_off[lo:lo + m] == umi_at).all()), "UMI offsets differ"
    exp = np.arange(lo, lo + m, dtype=np.uint64) * np.uint64(UMI + L)
    assert np.array_equal(off[lo:lo + m].cpu().numpy().view(np.uint64), exp), "offsets differ"
    assert bool((ln[lo:lo + m] == UMI + L).all()), "lengths differ"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("length", type=int)
    ap.add_argument("layout", choices=["se", "pe"])
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    n, L, S, batch = a.n, a.length, 2 if a.layout == "pe" else 1, 16 << 20
    mates = [torch.empty(n * L + 64, dtype=torch.uint8, device="cuda") for _ in range(S)]
    text, W, umi_at = id_lines(n)
    start = torch.arange(n, dtype=torch.int64, device="cuda") * W
    id_len = torch.full((n,), W, dtype=torch.int32, device="cuda")
    umi_off = torch.empty(n, dtype=torch.int32, device="cuda")
    out = torch.empty(n * (UMI + L) + 64, dtype=torch.uint8, device="cuda")
    off = torch.empty(n, dtype=torch.int64, device="cuda")
    ln = torch.empty(n, dtype=torch.int32, device="cuda")
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    given = [Reads(x, uniform_len=L, uniform_stride=L) for x in mates]
    with Engine(segments=S) as e:
        for s in range(S):
            e.synth_reads(7, 0, n, L, 0, s, mates[s], None)
        e.sync()
        small = min(n, 1 << 16)                                  # first launches load the code objects
        info = e.umi_find(text, start, id_len, small, ":", umi_off)
        e.umi_reads(text, start, umi_off, info, given[0], small, out, off, ln)
        e.sync()
        for r in range(a.repeat):
            info, find_ms = timed(lambda: e.umi_find(text, start, id_len, n, ":", umi_off))
            assert (info.n_bases, info.umi_len, info.joiners, info.bad_record) == (UMI, UMI, 0, ref.NO_RECORD)

            def pack():
                e.umi_reads(text, start, umi_off, info, given[0], n, out, off, ln, out_capacity=n * (UMI + L))
                e.sync()
            _, reads_ms = timed(pack)
            m = min(n, 50_000)
            check_sample(text, W, umi_at, mates[0], L, umi_off, out, off, ln, 0, m)
            check_sample(text, W, umi_at, mates[0], L, umi_off, out, off, ln, n - m, m)
            find_bytes = n * (W + 12 + 4)
            reads_bytes = n * (2 * L + 2 * UMI + 12 + 12)
            keyed = [Reads(out, offsets=off, lengths=ln)] + given[1:]
            enc_given = encode_ms(given, S, n, batch, lambda d, lo: Reads(d.bases[lo * L:], uniform_len=L, uniform_stride=L), keep)
            enc_keyed = encode_ms(keyed, S, n, batch, lambda d, lo: Reads(d.bases, offsets=d.offsets[lo:], lengths=d.lengths[lo:]) if d.offsets is not None
                                  else Reads(d.bases[lo * L:], uniform_len=L, uniform_stride=L), keep)
            print(json.dumps({"records": n, "length": L, "layout": a.layout, "id_line_bytes": W, "umi_bases": UMI,
                              "umi_find_ms": round(find_ms, 2), "find_bytes": find_bytes, "find_GB_per_s": round(find_bytes / find_ms / 1e6, 1),
                              "umi_reads_ms": round(reads_ms, 2), "reads_bytes": reads_bytes, "reads_GB_per_s": round(reads_bytes / reads_ms / 1e6, 1),
                              "both_ms": round(find_ms + reads_ms, 2),
                              "byte_ratio_to_canonical": round((W + 2 * L + UMI) / (2 * S * L), 3),
                              "encode_given_uniform_ms": round(enc_given[0], 2), "encode_keyed_ragged_ms": round(enc_keyed[0], 2),
                              "encode_launches": [enc_given[1], enc_keyed[1]]}), flush=True)


if __name__ == "__main__":
    main()
