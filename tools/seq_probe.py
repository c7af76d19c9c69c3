#!/usr/bin/env python3
"""Times the device half of the sequence-based modes on synthetic reads and checks it.
  python tools/seq_probe.py <n_reads> <len> [se|pe] [reps] [--keep best]
Reads come from fqd_synth_reads (bench.py's duplicate model: 30 % copies of earlier reads), then 5 % get one
substitution (near duplicates for tail-hamming) and 5 % are cut short (prefixes for loose).  Per mode it times keys +
sort (fqd_sort_seqs), heads (fqd_seq_heads) and the output plan (fqd_output_plan); it times fqd_sort_tags on the same
uncut spans against fqd_sort_seqs and checks that both permutations are identical; it checks the heads of a sorted
prefix against the CPU restatement (tests/seq_reference.py).  With `--keep best` it also builds whole FASTQ records
(a 20-byte ID line, the read, '+', a random quality line) around the reads of mate 1, times fqd_seq_scores and
fqd_seq_pick_best alone (the pick on the heads of `tight`, on a fresh copy of the order each time) and checks both against
numpy and the restatement (tests/seq_keep_reference.py) on a prefix.  Prints one JSON line."""
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


def keep_best_leg(e, line, bases, n, L, perm, head, reps, dev):
    """FQD_SEQ_KEEP=best: the two calls alone, on whole records of 2 L + 25 bytes around the reads."""
    import seq_keep_reference as keep
    R = 2 * L + 25
    g = torch.Generator(device=dev); g.manual_seed(12)
    rec = torch.empty((n, R), dtype=torch.uint8, device=dev)
    rec[:, 0] = ord("@"); rec[:, 1:20] = ord("r"); rec[:, 20] = ord("\n")
    rec[:, 21:21 + L] = bases[:n * L].view(n, L)
    rec[:, 21 + L] = ord("\n"); rec[:, 22 + L] = ord("+"); rec[:, 23 + L] = ord("\n")
    for lo in range(0, n, 1 << 24):                          # the quality lines, a piece at a time
        hi = min(n, lo + (1 << 24))
        rec[lo:hi, 24 + L:24 + 2 * L] = torch.randint(33, 75, (hi - lo, L), device=dev, generator=g, dtype=torch.uint8)
    rec[:, 24 + 2 * L] = ord("\n")
    text = torch.cat([rec.view(-1), torch.zeros(64, dtype=torch.uint8, device=dev)])
    del rec
    offs = torch.arange(n, dtype=torch.int64, device=dev) * R
    sizes = torch.full((n,), R, dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.int32, device=dev)
    ms, _ = timed(lambda: e.seq_scores((text, offs, sizes, n), score), reps)
    line["keep_scores_ms"] = round(ms, 3)
    line["keep_scores_quality_gb_per_s"] = round(n * L / ms / 1e6, 1)      # the quality bytes alone, over the call's time
    order = torch.empty_like(perm)
    best, moved = None, 0
    for _ in range(reps):
        order.copy_(perm)
        ms, moved = timed(lambda: e.seq_pick_best(score, head, n, order), 1)
        best = ms if best is None else min(best, ms)
    line["keep_pick_ms"] = round(best, 3); line["keep_clusters_changed"] = moved
    # a prefix: the scores by numpy, the pick of the whole clusters among the first places by the restatement
    k = min(n, 4000)
    qual = text[:k * R].view(k, R)[:, 24 + L:24 + 2 * L].cpu().numpy().astype(np.int64)
    line["keep_scores_prefix_ok"] = bool(np.array_equal(score[:k].cpu().numpy().view(np.uint32), (qual - 33).sum(axis=1)))
    h = head[:k + 1].cpu().numpy()
    m = k if n == k else int(np.nonzero(h)[0][-1])            # the last head among them ends whole clusters
    p0 = perm[:m].cpu().numpy().view(np.uint32).tolist()
    sc = dict(zip(p0, score[perm[:m].long()].cpu().numpy().view(np.uint32).tolist()))
    exp, _ = keep.pick(p0, h[:m].tolist(), sc)
    line["keep_pick_prefix_ok"] = order[:m].cpu().numpy().view(np.uint32).tolist() == exp


def main():
    argv = list(sys.argv)
    keep_best = False
    if "--keep" in argv:
        at = argv.index("--keep")
        if argv[at + 1:at + 2] != ["best"]:
            sys.exit("--keep takes 'best'")
        keep_best = True
        del argv[at:at + 2]
    sys.argv = argv
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
        if keep_best:
            e.seq_heads(mates[0], perm, SEQ_TIGHT, 2, head, m2)
            keep_best_leg(e, line, mates[0][0], n, L, perm, head, reps, dev)
    line["when"] = time.strftime("%Y-%m-%d %H:%M:%S")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
