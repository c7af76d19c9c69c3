#!/usr/bin/env python3
"""Times the device half of the sequence-based modes on synthetic reads and checks it.
  python tools/seq_probe.py <n_reads> <len> [se|pe] [reps]
Reads come from fqd_synth_reads (bench.py's duplicate model: 30 % copies of earlier reads), then 5 % get one
substitution (near duplicates for tail-hamming) and 5 % are cut short (prefixes for loose).  Per mode it times keys +
sort (fqd_sort_seqs), heads (fqd_seq_heads) and the output plan (fqd_output_plan); it times fqd_sort_tags on the same
uncut spans against fqd_sort_seqs and checks that both permutations are identical; it checks the heads of a sorted
prefix against the CPU restatement (tests/seq_reference.py).  Prints one JSON line."""
import json
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np
import torch

from fastq_dupaway_amd import Engine
from fastq_dupaway_amd._lib import SEQ_HAMMING, SEQ_LOOSE, SEQ_TIGHT
import seq_reference as ref


def timed(fn, reps):
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best, out


def main():
    n, L = int(sys.argv[1]), int(sys.argv[2])
    paired = len(sys.argv) > 3 and sys.argv[3] == "pe"
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    dev = torch.device("cuda")
    S = 2 if paired else 1
    g = torch.Generator(device=dev); g.manual_seed(11)
    mates, full = [], []
    with Engine(segments=S) as e:
        for s in range(S):
            bases = torch.empty(n * L + 64, dtype=torch.uint8, device=dev)
            e.synth_reads(1234, 0, n, L, 300, s, bases)
            e.sync()
            sub = torch.nonzero(torch.rand(n, device=dev, generator=g) < 0.05).squeeze(1)
            at = sub * L + torch.randint(0, L, (sub.numel(),), device=dev, generator=g)
            bases[at] = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (sub.numel(),), device=dev, generator=g)]
            offs = torch.arange(n, dtype=torch.int64, device=dev) * L
            lens = torch.full((n,), L, dtype=torch.int32, device=dev)
            full.append((bases, offs, lens.clone(), n))
            cut = torch.rand(n, device=dev, generator=g) < 0.05
            lens[cut] = torch.randint(0, L, (int(cut.sum()),), device=dev, generator=g, dtype=torch.int32)
            mates.append((bases, offs, lens, n))
        m2 = mates[1] if paired else None
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        head = torch.empty(n, dtype=torch.uint8, device=dev)
        sizes = (mates[0][2] + 1).to(torch.int32)
        src_off = torch.empty(n, dtype=torch.int64, device=dev); plen = torch.empty(n, dtype=torch.int32, device=dev)
        dst_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        line = {"probe": "seq", "reads": n, "len": L, "paired": paired}
        line["sort_ms"], _ = timed(lambda: e.sort_seqs(mates[0], perm, m2), reps)
        # the sequences of a sorted prefix, for the restatement (a prefix of the scan is the scan of the prefix)
        k = 4000
        idx = perm[:k].long()
        rows = []
        for m in mates:
            at = m[1][idx].unsqueeze(1) + torch.arange(L, device=dev)
            rows.append((m[0][at].cpu().numpy(), m[2][idx].cpu().numpy()))
        seqs = [tuple(r[j, :int(l[j])].tobytes() for r, l in rows) for j in range(k)]
        for name, mode in (("tight", SEQ_TIGHT), ("loose", SEQ_LOOSE), ("hamming", SEQ_HAMMING)):
            ms, heads = timed(lambda: e.seq_heads(mates[0], perm, mode, 2, head, m2), reps)
            pm, _ = timed(lambda: e.output_plan(head, perm, n, mates[0][1], sizes, src_off, plen, dst_off), reps)
            line[f"{name}_heads_ms"] = round(ms, 3); line[f"{name}_plan_ms"] = round(pm, 3); line[f"{name}_heads"] = heads
            line[f"{name}_device_ms"] = round(line["sort_ms"] + ms + pm, 3)
            exp = ref.heads({SEQ_TIGHT: ref.TIGHT, SEQ_LOOSE: ref.LOOSE, SEQ_HAMMING: ref.HAMMING}[mode], 2, seqs)
            line[f"{name}_prefix_ok"] = head[:k].cpu().numpy().tolist() == exp
        line["sort_ms"] = round(line["sort_ms"], 3)
        # fqd_sort_tags on the uncut spans (equal lengths: the '\n' changes nothing) against fqd_sort_seqs on the same
        perm_s = torch.empty(n, dtype=torch.int32, device=dev); perm_t = torch.empty(n, dtype=torch.int32, device=dev)
        if not paired:
            b, o, l, _ = full[0]
            line["sort_seqs_uncut_ms"] = round(timed(lambda: e.sort_seqs(full[0], perm_s), reps)[0], 3)
            line["sort_tags_uncut_ms"] = round(timed(lambda: e.sort_tags(b, o, l, n, perm_t), reps)[0], 3)
            line["perms_identical"] = bool(torch.equal(perm_s, perm_t))
            line["speedup_vs_sort_tags"] = round(line["sort_tags_uncut_ms"] / line["sort_seqs_uncut_ms"], 2)
    line["when"] = time.strftime("%Y-%m-%d %H:%M:%S")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
