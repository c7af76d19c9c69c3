"""Inputs and the numpy reference for fqd_output_offsets / fqd_output_plan / fqd_copy_spans (csrc/fqd_join.hip) at the
edges of their units: a lane takes 8 entries, a tile is 2048 (kOffTile), the tile sums are scanned by one workgroup of
1024 lanes (16 waves of 64 tiles) that loops over 1024 tiles at a time (scan_tiles_kernel).  131 072 = 64 x 2048 entries
fill the first wave of that scan, 2 097 152 = 1024 x 2048 its first round.  numpy only, seeded; the reference is
numpy's cumsum in uint64.  tests/test_edge_inputs.py holds the inputs to their claims, tests/test_gpu_plan_edges.py
holds the kernels to the reference."""
import numpy as np

LANE, TILE, WAVE_TILES, ROUND_TILES = 8, 2048, 64, 1024
NS = (1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 131_071, 131_072, 131_073,
      2_097_151, 2_097_152, 2_097_153, 2_097_152 + 2048 + 3)
KEEPS = ("all", "none", "first", "last", "alternating", "random")
BIG_KEEPS = ("all", "random", "last")                       # for the sizes above 131 073
SIZES = ("small", "wide")
U32_MAX = 0xFFFFFFFF


def keeps_for(n: int):
    return KEEPS if n <= 131_073 else BIG_KEEPS


def keep_flags(kind: str, n: int, rng) -> np.ndarray:
    keep = np.zeros(n, np.uint8)
    if kind == "all":
        keep[:] = 1
    elif kind == "first":
        keep[0] = 1
    elif kind == "last":
        keep[-1] = 1
    elif kind == "alternating":
        keep[0::2] = 1
    elif kind == "random":
        keep[:] = rng.random(n) < 0.5
    else:
        assert kind == "none"
    return keep


def make(n: int, keep_kind: str, size_kind: str):
    """n entries over a table of n_rec > n records: idx is a prefix of a permutation of the records, starts are random
    numbers below 2^40 (the text itself is never touched by the plan).  `wide` sizes cover the whole uint32 range, with
    0xFFFFFFFF at the first and the last kept entry, with the index list and without it."""
    rng = np.random.default_rng([n, KEEPS.index(keep_kind), SIZES.index(size_kind)])
    n_rec = n + n // 4 + 3
    keep = keep_flags(keep_kind, n, rng)
    idx = rng.permutation(n_rec)[:n].astype(np.uint32)
    starts = rng.integers(0, 1 << 40, n_rec, dtype=np.uint64)
    if size_kind == "small":
        sizes = rng.integers(0, 401, n_rec).astype(np.uint32)
        sizes[rng.random(n_rec) < 0.05] = 0
    else:
        sizes = rng.integers(0, 1 << 32, n_rec, dtype=np.uint64).astype(np.uint32)
        kept = np.flatnonzero(keep)
        for k in kept[[0, -1]] if len(kept) else ():
            sizes[idx[k]] = U32_MAX
            sizes[k] = U32_MAX
    return dict(n=n, n_rec=n_rec, keep=keep, idx=idx, starts=starts, sizes=sizes)


def plan_reference(case, use_idx: bool):
    """src_off, len, dst_off (uint64, uint32, uint64) per entry and the total."""
    r = case["idx"].astype(np.int64) if use_idx else np.arange(case["n"])
    lens = np.where(case["keep"] == 1, case["sizes"][r], 0).astype(np.uint64)
    inc = np.cumsum(lens, dtype=np.uint64)
    return case["starts"][r], lens.astype(np.uint32), inc - lens, int(inc[-1])


def offsets_reference(case):
    """dest per record (int64, -1 where the record is not kept) and the total."""
    _, _, dst, total = plan_reference(case, True)
    dest = np.full(case["n_rec"], -1, dtype=np.int64)
    kept = case["keep"] == 1
    dest[case["idx"][kept]] = dst[kept].view(np.int64)
    return dest, total


# ---- fqd_copy_spans behind a 2^33 bias --------------------------------------------------------------------------------
SPAN_BIAS = 1 << 33
SPAN_EDGES = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 127, 128, 129, 143, 144, 145, 300, 322, 399, 400)


def span_case():
    """Records of 0..400 bytes (the 16-byte edges of the eight copying lanes among them) at unaligned places of a text."""
    rng = np.random.default_rng(33)
    n_rec, n = 6000, 5000
    sizes = rng.integers(0, 401, n_rec).astype(np.uint32)
    sizes[:len(SPAN_EDGES)] = SPAN_EDGES
    gaps = rng.integers(0, 7, n_rec).astype(np.uint64)
    starts = (np.cumsum(sizes.astype(np.uint64) + gaps) - sizes).astype(np.uint64) + np.uint64(3)
    text = rng.integers(1, 256, int(starts[-1]) + int(sizes[-1]) + 16, dtype=np.uint8)
    idx = rng.permutation(n_rec)[:n].astype(np.uint32)
    idx[:len(SPAN_EDGES)] = rng.permutation(len(SPAN_EDGES))             # every edge length is among the entries
    idx[len(SPAN_EDGES):] = rng.permutation(np.arange(len(SPAN_EDGES), n_rec))[:n - len(SPAN_EDGES)]
    keep = (rng.random(n) < 0.8).astype(np.uint8)
    keep[:len(SPAN_EDGES)] = 1
    return dict(n=n, n_rec=n_rec, keep=keep, idx=idx, starts=starts, sizes=sizes, text=text)


def span_window(case) -> np.ndarray:
    """What the output holds: the kept records in entry order, side by side."""
    t, s, z = case["text"], case["starts"], case["sizes"]
    return np.concatenate([t[int(s[r]):int(s[r]) + int(z[r])] for r, k in zip(case["idx"], case["keep"]) if k])
