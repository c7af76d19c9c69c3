#!/usr/bin/env python3
"""What FQD_FAST_UMI_MISMATCH adds on the device: a synthetic library of molecules x PCR copies x a per-base UMI error rate
goes through the run's steps — the pass keyed UMI ‖ sequence (pass A), the exact owners, grouping and counts, the reset, the
pass keyed by sequence alone (pass B), fqd_umi_merge, fqd_group_owners over the merged owners — each timed on its own, three
repeats; whole sequence groups at the start and at the end of the file are held against the sequential Python statement
(tests/umi_merge_reference.py) on every repeat.

    python tools/umi_merge_probe.py --reads N [--length 100] [--copies 4] [--umis-per-fragment 3] [--error 0.01] [--distance 1]

One JSON line per repeat, appended to profiles/umi_merge_probe.jsonl.  Wall time round each step with a synchronisation
behind it.  fqd_umi_merge reports its own three stages (nodes: count and scan; group: compaction write, sort, pack, classes;
merge: the networks and the spread) from the waits it has anyway.  A fragment is one sequence; a molecule is a UMI on a
fragment; a read copies a molecule, each UMI base wrong with probability --error."""
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
import umi_merge_reference as ref  # noqa: E402

HEAD, TAIL, DIGITS, UMI = b"@A00:7:", b" 1:N:0:ATCACG\n", 9, 8
BATCH = 16 << 20


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def make_library(n, L, copies, per_fragment, error, seed):
    """(reads n x L, UMIs n x 8, both uint8 on the device) in shuffled order."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    letters = torch.frombuffer(bytearray(b"ACGT"), dtype=torch.uint8).cuda()
    molecules = max(1, n // copies)
    fragments = max(1, molecules // per_fragment)
    frag_seq = torch.randint(0, 4, (fragments, L), device="cuda", generator=gen, dtype=torch.uint8)
    mol_frag = torch.randint(0, fragments, (molecules,), device="cuda", generator=gen)
    mol_umi = torch.randint(0, 4, (molecules, UMI), device="cuda", generator=gen, dtype=torch.uint8)
    reads = torch.empty((n, L), dtype=torch.uint8, device="cuda")
    umis = torch.empty((n, UMI), dtype=torch.uint8, device="cuda")
    step = 1 << 22
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        mol = torch.randint(0, molecules, (hi - lo,), device="cuda", generator=gen)
        reads[lo:hi] = letters[frag_seq[mol_frag[mol]].long()]
        u = mol_umi[mol]
        wrong = torch.rand((hi - lo, UMI), device="cuda", generator=gen) < error
        shift = torch.randint(1, 4, (hi - lo, UMI), device="cuda", generator=gen, dtype=torch.uint8)
        umis[lo:hi] = letters[torch.where(wrong, (u + shift) % 4, u).long()]
    return reads, umis


def id_lines(umis):
    """ID lines "@A00:7:<9 digits>:<8 bases> 1:N:0:ATCACG\\n" of one width round the given UMIs; returns (text, width)."""
    n = umis.shape[0]
    W = len(HEAD) + DIGITS + 1 + UMI + len(TAIL)
    text = torch.empty((n, W), dtype=torch.uint8, device="cuda")
    text[:, :len(HEAD)] = torch.frombuffer(bytearray(HEAD), dtype=torch.uint8).cuda()
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    for d in range(DIGITS):
        text[:, len(HEAD) + DIGITS - 1 - d] = ((idx // 10 ** d) % 10 + ord("0")).to(torch.uint8)
    at = len(HEAD) + DIGITS
    text[:, at] = ord(":")
    text[:, at + 1:at + 1 + UMI] = umis
    text[:, at + 1 + UMI:] = torch.frombuffer(bytearray(TAIL), dtype=torch.uint8).cuda()
    return text.reshape(-1), W


def check_groups(umis, owner_seq, owner_out, distance, max_group, where):
    """The whole sequence groups of the records in `where` against the statement."""
    wanted = torch.unique(owner_seq[where])
    members = torch.nonzero(torch.isin(owner_seq, wanted)).reshape(-1)
    idx = members.cpu().numpy()
    u = umis[members].cpu().numpy()
    seq = owner_seq[members].cpu().numpy()
    exp, info, *_ = ref.merge([x.tobytes() for x in u], [int(s) for s in seq], distance, max_group)
    got = owner_out[members].cpu().numpy().view(np.uint32)
    assert np.array_equal(got, idx[exp].astype(np.uint32)), "merged owners differ from the statement"
    return len(idx), info["groups"], info["merged"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, required=True)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--umis-per-fragment", type=int, default=3)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--distance", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "umi_merge_probe.jsonl"))
    a = ap.parse_args()
    n, L = a.reads, a.length
    reads, umis = make_library(n, L, a.copies, a.umis_per_fragment, a.error, 11)
    text, W = id_lines(umis)
    bases = torch.cat([reads.reshape(-1), torch.zeros(64, dtype=torch.uint8, device="cuda")])
    del reads
    start = torch.arange(n, dtype=torch.int64, device="cuda") * W
    id_len = torch.full((n,), W, dtype=torch.int32, device="cuda")
    i32 = lambda: torch.empty(n, dtype=torch.int32, device="cuda")
    umi_off, ln, link, owner_exact, owner_seq, size, perm, owner_out = (i32() for _ in range(8))
    keyed = torch.empty(n * (UMI + L) + 64, dtype=torch.uint8, device="cuda")
    off = torch.empty(n, dtype=torch.int64, device="cuda")
    keep, head = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(2))
    given = Reads(bases, uniform_len=L, uniform_stride=L)

    def submit_all(e, seg_at):
        for lo in range(0, n, BATCH):
            m = min(BATCH, n - lo)
            e.submit_linked([seg_at(lo)], m, keep[lo:], link[lo:], last=lo + m == n)
        e.sync()

    with Engine(segments=1, capacity_reads=n, capacity_bases=n * (UMI + L)) as e:
        info = e.umi_find(text, start, id_len, n, ":", umi_off)
        e.umi_reads(text, start, umi_off, info, given, n, keyed, off, ln, out_capacity=n * (UMI + L))
        e.sync()
        for r in range(a.repeat + 1):                            # (the first round loads the code objects and is not reported)
            e.reset()
            _, pass_a = timed(lambda: submit_all(e, lambda lo: Reads(keyed, offsets=off[lo:], lengths=ln[lo:])))
            _, owners_a = timed(lambda: e.owners(keep, link, n, owner_exact))
            exact, group_a = timed(lambda: e.group_owners(owner_exact, n, perm, head))
            _, sizes_a = timed(lambda: e.cluster_sizes(perm, head, n, size, levels=False))
            _, reset_ms = timed(e.reset)
            _, pass_b = timed(lambda: submit_all(e, lambda lo: Reads(bases[lo * L:], uniform_len=L, uniform_stride=L)))
            _, owners_b = timed(lambda: e.owners(keep, link, n, owner_seq))
            got, merge_ms = timed(lambda: e.umi_merge(text, start, umi_off, info, owner_exact, owner_seq, size, n, a.distance, owner_out))
            assert got.over_limit_first == ref.NO_RECORD and got.nodes == exact
            clusters, group_merged = timed(lambda: e.group_owners(owner_out, n, perm, head))
            assert clusters == got.nodes - got.merged
            edge = min(n, 2000)
            checked = [check_groups(umis, owner_seq, owner_out, a.distance, got.max_group, slice(0, edge)),
                       check_groups(umis, owner_seq, owner_out, a.distance, got.max_group, slice(n - edge, n))]
            if r == 0:
                continue
            stages = [round(float(x), 2) for x in got.stage_ms[:3]]
            line = {"reads": n, "length": L, "umi_bases": UMI, "copies": a.copies, "umis_per_fragment": a.umis_per_fragment, "error": a.error,
                    "distance": a.distance, "exact_clusters": int(got.nodes), "groups_of_several": int(got.groups), "merged": int(got.merged),
                    "largest_group": int(got.largest), "sweeps": int(got.sweeps), "merged_clusters": int(clusters),
                    "pass_a_ms": round(pass_a, 2), "owners_a_ms": round(owners_a, 2), "group_owners_exact_ms": round(group_a, 2),
                    "cluster_sizes_ms": round(sizes_a, 2), "reset_ms": round(reset_ms, 2), "pass_b_ms": round(pass_b, 2), "owners_b_ms": round(owners_b, 2),
                    "umi_merge_ms": round(merge_ms, 2), "merge_stage_nodes_ms": stages[0], "merge_stage_group_ms": stages[1],
                    "merge_stage_networks_ms": stages[2], "networks_share": round(stages[2] / max(sum(stages), 1e-9), 3),
                    "group_owners_merged_ms": round(group_merged, 2),
                    "checked_records_groups_merged": checked}
            print(json.dumps(line), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
