#!/usr/bin/env python3
"""What FQD_FAST_KEEP / FQD_FAST_CLUSTERS add on the device: times fqd_owners, fqd_group_owners, fqd_seq_pick_best and
fqd_heads_to_keep over synthetic reads (fqd_synth_reads: 150 bp, about 20 % duplicates, chains allowed) submitted
through fqd_submit_linked in 16 Mi batches, and holds the flags against the generator's closed-form ones.

    python tools/owner_probe.py --reads 100000000 [--dup-permille 200] [--repeat 3]

One JSON line per repeat.  The calls drain the engine's stream themselves, so wall time around a call is its device
time plus one launch and one synchronisation."""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fastq_dupaway_amd import Engine, Reads  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--dup-permille", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    n, L, batch = a.reads, a.length, 16 << 20
    bases = torch.empty(n * L + 64, dtype=torch.uint8, device="cuda")
    expect = torch.empty(n, dtype=torch.uint8, device="cuda")
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    link = torch.empty(n, dtype=torch.int32, device="cuda")
    owner = torch.empty(n, dtype=torch.int32, device="cuda")
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    head = torch.empty(n, dtype=torch.uint8, device="cuda")
    score = torch.randint(0, 6000, (n,), dtype=torch.int32, device="cuda")   # a 150-base quality line sums to about this much
    for r in range(a.repeat):
        with Engine(segments=1, capacity_reads=n, capacity_bases=n * L) as e:
            e.synth_reads(7, 0, n, L, a.dup_permille, 0, bases, expect)
            e.sync()

            def submit():
                for lo in range(0, n, batch):
                    m = min(batch, n - lo)
                    e.submit_linked([Reads(bases[lo * L:], uniform_len=L, uniform_stride=L)], m, keep[lo:], link[lo:], last=lo + m == n)
                e.sync()
            _, t_submit = timed(submit)
            assert torch.equal(keep, expect), "keep flags differ from the generator's"
            _, t_owners = timed(lambda: e.owners(keep, link, n, owner))
            clusters, t_group = timed(lambda: e.group_owners(owner, n, perm, head))
            assert clusters == int(expect.sum().item())
            moved, t_pick = timed(lambda: e.seq_pick_best(score, head, n, perm))
            _, t_keep = timed(lambda: e.heads_to_keep(perm, head, n, keep))
            assert int(keep.sum().item()) == clusters
        print(json.dumps({"reads": n, "length": L, "dup_permille": a.dup_permille, "clusters": clusters, "moved": moved,
                          "submit_linked_ms": round(t_submit, 2), "owners_ms": round(t_owners, 2), "group_owners_ms": round(t_group, 2),
                          "pick_ms": round(t_pick, 2), "heads_to_keep_ms": round(t_keep, 2)}), flush=True)


if __name__ == "__main__":
    main()
