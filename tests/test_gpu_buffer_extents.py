"""Every entry point of include/fqdupaway.h that takes a caller's device buffer, run with its buffers inside a guarded arena
(tests/guarded_arena.py): nothing outside the extents the header states is stored to, no const input changes, and the
results do not depend on what lies around a buffer or on where it lies — below or beyond byte 2^32 of a text.

A case is a function case(A) -> dict: it builds its inputs through the allocator A (A.inp / A.out / A.inout / A.text), calls
A.ready(), calls one entry point through fastq_dupaway_amd.Engine and returns its outputs (device tensors, host values, or
callables evaluated after the run).  Every case runs
  plain   every buffer a tensor of its own, as the other tests allocate,
  ff      in the arena, guards of 0xFF: no base, no newline, no digit,
  nl      in the arena, guards of '\\n',
  far     (cases with a byte buffer addressed by offsets) that buffer in a 4.5 GiB arena, the first of a case across byte 2^32
          and the others beyond it, the arena's base handed over so that the offset VALUES exceed 2^32,
and asserts: the arena's check passes; the outputs of all runs are byte-identical (entries the header calls meaningless are
masked by the case); the plain run's outputs are not trivial.  What the outputs MEAN is held against references by the
other test files; equality with the plain run is the check here.  Unwritten output entries are pre-set to 0xA5 in every run.

Shapes: record counts from {1, 63, 64, 65, 255, 256, 257, 1025}, read lengths from {1, 15, 16, 17, 31, 32, 33, 150, 151}."""
import ctypes as C
import random
import re
import struct
import zlib

import numpy as np
import pytest
import torch

import bgzf_cases
import consensus_cases as cc
import gunzip_cases
import inflate_cases
import join_edge_cases as jc
import near_cases
import optical_cases as oc
import plan_edge_cases as pc
import scan_edge_cases as sc
from guarded_arena import GUARD, TORCH_OF, Arena, to_torch_bits
from fastq_dupaway_amd import Engine, Reads, _lib, declared_symbols, load_library

pytestmark = pytest.mark.gpu

POISON = 0xA5
P32, P64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
NONE32 = 0xFFFFFFFF
ARENA_BYTES = 48 << 20
FAR_BYTES = (9 << 30) // 2                                    # 4.5 GiB
u8, u32, u64 = np.uint8, np.uint32, np.uint64
SHAPES = [(1, 1), (63, 15), (64, 16), (65, 17), (255, 31), (256, 32), (257, 33), (1025, 150), (257, 151)]     # (records, read length)


# ---- the allocator a case sees -----------------------------------------------------------------------------------------------------

class Text:
    """A byte buffer addressed through offsets: hand `base` to the library and add `bias` to every offset; `view` is the bytes."""
    def __init__(self, base, bias, view):
        self.base, self.bias, self.view = base, bias, view


class Alloc:
    def __init__(self, mode, far=None):
        self.mode = mode
        self.arena = None if mode == "plain" else Arena("cuda", ARENA_BYTES, 10 if mode == "nl" else 0xFF)
        self.far = far if mode == "far" else None
        self.far_next = None
        if self.far is not None:
            self.far.reset(0xFF)

    def _take(self, name, dtype, count, role):
        if self.arena is None:
            return torch.empty(count, dtype=TORCH_OF[np.dtype(dtype)], device="cuda")
        return self.arena.take(name, dtype, count, role)

    def inp(self, name, a, role="in"):
        a = np.ascontiguousarray(a).reshape(-1)
        t = self._take(name, a.dtype, a.size, role)
        t.copy_(to_torch_bits(a))
        return t

    def inout(self, name, a):
        return self.inp(name, a, "inout")

    def out(self, name, dtype, count, preset=None):
        t = self._take(name, dtype, count, "out")
        if preset is None:
            t.view(torch.uint8).fill_(POISON)
        else:
            t.copy_(to_torch_bits(np.ascontiguousarray(np.broadcast_to(np.asarray(preset, dtype), (count,)))))
        return t

    def text(self, name, a, role="in"):
        """a: the bytes (numpy uint8), or a byte count for an output, which is pre-set to 0xA5."""
        a = np.full(a, POISON, u8) if isinstance(a, int) else np.ascontiguousarray(a, u8).reshape(-1)
        if self.far is None:
            t = self.inp(name, a, role)
            return Text(t, 0, t)
        if self.far_next is None:
            at = ((1 << 32) - a.size // 2 - 1) | 1              # across byte 2^32, at an odd address
        else:
            at = self.far_next
        self.far_next = (max(at + a.size, 1 << 32) + 2 * GUARD) | 1
        t = self.far.take(name, u8, a.size, role, at=at)
        t.copy_(to_torch_bits(a))
        return Text(self.far.mem, at, t)

    def ready(self):
        for a in (self.arena, self.far):
            if a is not None:
                a.seal()
        torch.cuda.synchronize()

    def check(self):
        for a in (self.arena, self.far):
            if a is not None:
                a.check()


class FarHolder:
    arena = None

    def get(self):
        if self.arena is None:                                  # a failure here is the test's failure
            self.arena = Arena("cuda", FAR_BYTES, 0xFF, windowed=True)
        return self.arena


@pytest.fixture(scope="module")
def far_holder():
    h = FarHolder()
    yield h
    h.arena = None
    torch.cuda.empty_cache()


def host(v):
    if isinstance(v, torch.Tensor):
        return v.cpu().numpy().copy()
    if callable(v):
        return host(v())
    if isinstance(v, (list, tuple)):
        return [host(x) for x in v]
    return v


def same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)
    if isinstance(a, list):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def first_difference(a, b):
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape:
        at = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
        return f"{len(at)} entries differ, the first at {int(at[0])}: {a.reshape(-1)[at[0]]} against {b.reshape(-1)[at[0]]}"
    return f"{a!r} against {b!r}"[:400]


def run_case(fn, mode, far_holder):
    A = Alloc(mode, far_holder.get() if mode == "far" else None)
    out = fn(A)
    torch.cuda.synchronize()
    A.check()
    nontrivial = out.pop("_nontrivial")
    mask = out.pop("_mask", {})
    got = {k: host(v) for k, v in out.items()}
    for k, m in mask.items():
        got[k] = np.where(host(m), got[k], 0)
    return got, nontrivial


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

ACGTN = np.frombuffer(b"ACGTN", u8)


def bits(t, dtype):
    return t.cpu().numpy().view(dtype)


def dup_reads(seed, n, lens, ragged=False):
    """Per mate the n reads (lists of uint8 arrays): about half of the records are copies of earlier ones; ragged: a pool
    read's length, 1 .. lens[m], is its own, so copies stay copies."""
    rng = np.random.default_rng(seed)
    pool_n = max(1, (n + 1) // 2)
    pick = rng.integers(0, pool_n, n)
    mates = []
    for L in lens:
        pool = rng.choice(ACGTN, size=(pool_n, L), p=[.24, .24, .24, .24, .04])
        plen = rng.integers(1, L + 1, pool_n) if ragged else np.full(pool_n, L)
        plen[0] = L
        mates.append([pool[p, :plen[p]] for p in pick])
    return mates


def first_index(keys):
    seen = {}
    return np.array([seen.setdefault(k, i) for i, k in enumerate(keys)], u32)


def uniform_bytes(reads, stride):
    """Read i at i * stride, 0xEE between the reads, the buffer ending with the last read's last byte."""
    n, L = len(reads), len(reads[0])
    flat = np.full((n - 1) * stride + L, 0xEE, u8)
    for i, r in enumerate(reads):
        flat[i * stride:i * stride + L] = r
    return flat


def ragged_bytes(reads, seed):
    """Back to back with gaps of 0 .. 3 bytes of 0xEE, the first read at byte 0, the last one ending the buffer."""
    rng = np.random.default_rng(seed)
    gaps = rng.integers(0, 4, len(reads))
    gaps[0] = 0
    lens = np.array([len(r) for r in reads], u32)
    offs = (np.cumsum(gaps + lens) - lens).astype(u64)
    flat = np.full(int(offs[-1]) + int(lens[-1]), 0xEE, u8)
    for o, r in zip(offs, reads):
        flat[int(o):int(o) + len(r)] = r
    return flat, offs, lens


def mate_lengths(L, S):
    return (L,) if S == 1 else (L, L - 1 if L > 1 else 1)


class Segs:
    """The descriptors of one batch layout, placed through the allocator; part(a) = the batch that starts at record a."""
    def __init__(self, A, tag, mates, layout):
        self.parts = []
        for m, reads in enumerate(mates):
            L = len(reads[0])
            if layout == "ragged":
                flat, offs, lens = ragged_bytes(reads, 5 + m)
                T = A.text(f"{tag}.bases{m}", flat)
                self.parts.append((T.base, A.inp(f"{tag}.offsets{m}", offs + u64(T.bias)), A.inp(f"{tag}.lengths{m}", lens), 0, 0))
            else:
                stride = L if layout == "noslack" else 2 * L + 19
                self.parts.append((A.inp(f"{tag}.bases{m}", uniform_bytes(reads, stride)), None, None, L, stride))

    def part(self, a=0):
        return [Reads(b[a * stride:], uniform_len=L, uniform_stride=stride) if o is None else Reads(b, offsets=o[a:], lengths=l[a:])
                for b, o, l, L, stride in self.parts]


class Words:
    """Raw device memory as something torch can alias."""
    def __init__(self, ptr, n_words):
        self.__cuda_array_interface__ = {"shape": (n_words,), "typestr": "<i8", "data": (ptr, False), "version": 3, "strides": None}


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def encoded(n, lens):
    """[hash, key words] of dup_reads(n, lens) as a host array (n, W + 1), by a plain fqd_encode_uniform, once."""
    def make():
        mates = dup_reads(11 * n + lens[0], n, lens)
        with Engine(segments=len(lens)) as e:
            W = e.key_words(lens[0], lens[1] if len(lens) > 1 else 0)
            rec = torch.empty(n * (W + 1), dtype=torch.int64, device="cuda")
            segs = [Reads(torch.from_numpy(uniform_bytes(r, len(r[0]))).cuda(), uniform_len=len(r[0]), uniform_stride=len(r[0]))
                    for r in mates]
            e.encode_uniform(segs, n, rec)
            e.sync()
        keys = [tuple(bytes(r[i]) for r in mates) for i in range(n)]
        return bits(rec, u64).reshape(n, W + 1).copy(), first_index(keys)
    return cached(("encoded", n, lens), make)


# ---- the dedup core ----------------------------------------------------------------------------------------------------------------

def insert_paths(e):
    """(launches of bucket_dedup_kernel, launches of insert_kernel) so far, from the engine's profile."""
    p = e.profile()
    return [int(p["dedup_launches"]), int(p["insert_launches"])]


def paths_are_the_column_s(paths, counts, two_batches):
    """FQD_BULK_MIN=0: an engine's first batch takes the bulk path (the table is empty), a second batch of at most 684 records the
    atomic one (12 n < the table's slots); FQD_BULK_MIN=-1: the atomic path alone.  Pinned here so that a change of the table's
    geometry cannot make both columns run one kernel unseen."""
    import os
    if os.environ["FQD_BULK_MIN"] == "-1":
        return all(bulk == 0 and atomic >= 1 for bulk, atomic in paths)
    return all(bulk >= 1 and (atomic >= 1 or not (two_batches and n >= 64)) for (bulk, atomic), n in zip(paths, counts) if n >= 63)


def case_submit(A, kind, S, layout):
    runs = []
    for n, L in SHAPES:
        mates = dup_reads(7 * n + L + S, n, mate_lengths(L, S), ragged=layout == "ragged")
        segs = Segs(A, f"n{n}L{L}", mates, layout)
        keep = A.out(f"n{n}L{L}.keep", u8, n)
        link = A.out(f"n{n}L{L}.link", u32, n) if kind == "linked" else None
        runs.append((n, segs, keep, link))
    A.ready()
    paths = []
    for n, segs, keep, link in runs:
        cuts = [0, n // 3, n] if n >= 64 else [0, n]              # a second batch starts at a record of its own
        with Engine(segments=S, no_stage=layout == "nostage", profile=True) as e:
            for a, b in zip(cuts[:-1], cuts[1:]):
                last = b == n
                if kind == "linked":
                    e.submit_linked(segs.part(a), b - a, keep[a:], link[a:], last=last)
                else:
                    e.submit(segs.part(a), b - a, keep[a:], final=last and kind == "final")
            e.sync()
            paths.append(insert_paths(e))
    out = {f"keep{k}": r[2] for k, r in enumerate(runs)}
    out["paths"] = paths
    if kind == "linked":                                           # which earlier copy a link names is the schedule's; that it was written is not
        out.update({f"link_written{k}": (lambda r=r: bits(r[3], u32) != P32) for k, r in enumerate(runs)})
        out["links_are_earlier"] = lambda: all(bool(np.all((bits(r[3], u32) < np.arange(r[0])) | (bits(r[3], u32) == P32))) for r in runs)
    out["_nontrivial"] = lambda o: all(0 < int(o[f"keep{k}"].sum()) < r[0] for k, r in enumerate(runs) if r[0] >= 63) and o.get("links_are_earlier", True) \
        and paths_are_the_column_s(o["paths"], [r[0] for r in runs], two_batches=True)
    return out


def case_encode_uniform(A, S, no_stage, layout):
    runs = []
    with Engine(segments=S, no_stage=no_stage) as e:
        for n, L in SHAPES:
            lens = mate_lengths(L, S)
            segs = Segs(A, f"n{n}L{L}", dup_reads(n + L, n, lens), layout)
            W = e.key_words(lens[0], lens[1] if S == 2 else 0)
            runs.append((n, segs, A.out(f"n{n}L{L}.records", u64, n * (W + 1))))
        A.ready()
        for n, segs, rec in runs:
            e.encode_uniform(segs.part(), n, rec)
        e.sync()
    out = {f"records{k}": r[2] for k, r in enumerate(runs)}
    out["_nontrivial"] = lambda o: all(len(np.unique(o[f"records{k}"])) > 2 for k in range(1, len(runs)))
    return out


def case_encode_padded(A, S, layout):
    runs = []
    with Engine(segments=S, no_stage=layout == "nostage") as e:
        for n, L in SHAPES:
            lens = mate_lengths(L, S)
            segs = Segs(A, f"n{n}L{L}", dup_reads(n + L, n, lens, ragged=layout != "uniform"), "ragged" if layout == "nostage" else layout)
            K = e.padded_key_words(lens[0], lens[1] if S == 2 else 0)
            runs.append((n, segs, A.out(f"n{n}L{L}.records", u64, n * (K + 1)), lens))
        A.ready()
        for n, segs, rec, lens in runs:
            e.encode_padded(segs.part(), n, lens[0], lens[1] if S == 2 else 0, rec)
        e.sync()
    out = {f"records{k}": r[2] for k, r in enumerate(runs)}
    out["_nontrivial"] = lambda o: all(len(np.unique(o[f"records{k}"])) > 2 for k in range(1, len(runs)))
    return out


# ---- the split halves ----------------------------------------------------------------------------------------------------------------

PART_SHAPES = [(1, (150,)), (65, (17,)), (257, (33,)), (1025, (150,)), (257, (150, 149))]


def case_partition_keys(A, parts):
    runs = []
    for n, lens in PART_SHAPES:
        rec, _ = encoded(n, lens)
        W = rec.shape[1] - 1
        t = f"n{n}W{W}"
        runs.append((n, W, A.inp(t + ".records", rec), A.out(t + ".out_keys", u64, n * W), A.out(t + ".counts", u64, parts), A.out(t + ".origin", u32, n)))
    A.ready()
    with Engine(segments=1) as e:
        for n, W, rec, keys, counts, origin in runs:
            e.partition_keys(rec, n, W, parts, keys, counts, origin)
        e.sync()
    out = {f"{name}{k}": r[3 + j] for k, r in enumerate(runs) for j, name in enumerate(("keys", "counts", "origin"))}
    out["_nontrivial"] = lambda o: int(o["counts3"].view(u64).sum()) == 1025 and len(np.unique(o["origin3"])) == 1025
    return out


def case_partition_slabs(A, parts, room):
    runs = []
    for n, lens in PART_SHAPES:
        rec, _ = encoded(n, lens)
        W = rec.shape[1] - 1
        cap = {"fits": n, "spills_a_little": max(1, n // parts - 1 if parts > 1 else n - 3), "spills_nearly_all": 1}[room]
        slots = parts * cap + n
        t = f"n{n}W{W}"
        runs.append((n, W, cap, A.inp(t + ".records", rec), A.out(t + ".out_keys", u64, slots * W), A.out(t + ".counts", u64, parts),
                     A.out(t + ".origin", u32, slots)))
    A.ready()
    with Engine(segments=1) as e:
        for n, W, cap, rec, keys, counts, origin in runs:
            e.partition_slabs(rec, n, W, parts, cap, keys, counts, origin)
        e.sync()
    out = {f"{name}{k}": r[4 + j] for k, r in enumerate(runs) for j, name in enumerate(("keys", "counts", "origin"))}

    def nontrivial(o):
        origin, cap = o["origin3"].view(u32), runs[3][2]
        filled = origin[(origin != NONE32) & (origin != P32)]
        spilled = int(((origin[parts * cap:] != NONE32) & (origin[parts * cap:] != P32)).sum())
        return np.array_equal(np.sort(filled), np.arange(1025)) and (room == "fits") == (spilled == 0)
    out["_nontrivial"] = nontrivial
    return out


def case_encode_slabs(A, hashed, parts, exact, room):
    runs = []
    for n, lens in [(1025, (150,)), (257, (33,)), (1025, (150, 150))]:
        S = len(lens)
        chunk = 256
        G = -(-n // chunk)
        sub_cap = chunk if room == "fits" else 8
        W = int(load_library().fqd_key_words(lens[0], lens[1] if S == 2 else 0))
        mates = dup_reads(n + lens[0] + S, n, lens)
        t = f"n{n}L{lens[0]}S{S}"
        bases = [A.inp(f"{t}.bases{m}", uniform_bytes(mates[m], lens[m] + 7)) for m in range(S)]       # stride L + 7: the one-pass form applies
        segs = [Reads(bases[m], uniform_len=lens[m], uniform_stride=lens[m] + 7) for m in range(S)]
        used = parts * G * sub_cap
        bufs = dict(keys=A.out(t + ".out_keys", u64, (used + n) * W), hashes=A.out(t + ".out_hashes", u64, used) if hashed else None,
                    counts=A.out(t + ".chunk_counts", u64, parts * G), totals=A.out(t + ".totals", u64, parts + 1), origin=A.out(t + ".origin", u32, used + n))
        runs.append((n, S, segs, chunk, G, sub_cap, bufs))
    A.ready()
    for n, S, segs, chunk, G, sub_cap, b in runs:
        with Engine(segments=S) as e:
            if hashed:
                e.encode_slabs_hashed(segs, n, parts, chunk, G, sub_cap, b["keys"], b["hashes"], b["counts"], b["totals"], b["origin"], exact=exact)
            else:
                e.encode_slabs(segs, n, parts, chunk, G, sub_cap, b["keys"], b["counts"], b["totals"], b["origin"], exact=exact)
            e.sync()
    out = {f"{name}{k}": t for k, r in enumerate(runs) for name, t in r[6].items() if t is not None}

    def nontrivial(o):
        ok = True
        for k, r in enumerate(runs):
            n, parts_total = r[0], int(o[f"totals{k}"].view(u64)[:parts].sum())
            ok = ok and parts_total == n and int(o[f"counts{k}"].view(u64).sum()) == n
            ok = ok and (exact or int(o[f"totals{k}"].view(u64)[parts]) == 0)
        return ok
    out["_nontrivial"] = nontrivial
    return out


def case_insert(A, how):
    """how: keys / slabs / slabs_hashed.  The keys lie in the engine's own store (fqd_reserve_keys); keep, the slab counts and
    the hashes are the caller's."""
    runs = []
    for n, lens in PART_SHAPES[1:]:
        rec, first = encoded(n, lens)
        t = f"n{n}L{lens[0]}S{len(lens)}"
        if how == "keys":
            runs.append((n, lens, rec, first, None, None, A.out(t + ".keep", u8, n), None))
            continue
        n_slabs, cap = 3, -(-n // 2)
        cuts = [0, cap, cap + n // 4, n]                             # a full slab and two partial ones
        counts = np.array([cuts[j + 1] - cuts[j] for j in range(3)], u64)
        assert counts.max() <= cap and counts.sum() == n
        hashes = None
        if how == "slabs_hashed":
            h = np.full((n_slabs, cap), 0x1234567, u64)
            for j in range(3):
                h[j, :int(counts[j])] = rec[cuts[j]:cuts[j + 1], 0]
            hashes = A.inout(t + ".hashes", h)
        runs.append((n, lens, rec, first, cuts, A.inp(t + ".slab_count", counts), A.out(t + ".keep", u8, n if how == "keys" else n_slabs * cap), hashes))
    A.ready()
    paths = []
    for n, lens, rec, first, cuts, slab_count, keep, hashes in runs:
        S, W = len(lens), rec.shape[1] - 1
        shape = (lens[0], lens[1] if S == 2 else 0)
        wire = torch.from_numpy(rec[:, 1:].copy().view(np.int64)).cuda()
        with Engine(segments=S, profile=True) as e:
            if how == "keys":
                slot = torch.as_tensor(Words(e.reserve_keys(n, *shape), n * W), device="cuda")
                slot.copy_(wire.view(-1))
                torch.cuda.synchronize()
                e.insert_keys(slot, n, *shape, keep)
            else:
                cap = keep.numel() // 3
                slot = torch.as_tensor(Words(e.reserve_keys(3 * cap, *shape), 3 * cap * W), device="cuda").view(3, cap, W)
                slot.fill_(-1)
                for j in range(3):
                    slot[j, :cuts[j + 1] - cuts[j]] = wire[cuts[j]:cuts[j + 1]]
                torch.cuda.synchronize()
                if how == "slabs":
                    e.insert_slabs(slot, 3, cap, slab_count, *shape, keep)
                else:
                    e.insert_slabs_hashed(slot, hashes, 3, cap, slab_count, *shape, keep)
            e.sync()
            paths.append(insert_paths(e))
    out, mask = {"paths": paths}, {}
    for k, (n, lens, rec, first, cuts, slab_count, keep, hashes) in enumerate(runs):
        out[f"keep{k}"] = keep
        if how != "keys":                                            # "keep has n_slabs * slab_cap entries; those of unused slots mean nothing"
            cap = keep.numel() // 3
            m = np.zeros((3, cap), bool)
            for j in range(3):
                m[j, :cuts[j + 1] - cuts[j]] = True
            mask[f"keep{k}"] = m.reshape(-1)
        if hashes is not None:
            out[f"hashes{k}"] = hashes
    out["_mask"] = mask

    def nontrivial(o):
        for k, (n, lens, rec, first, cuts, *_rest) in enumerate(runs):
            want = (first == np.arange(n)).astype(u8)
            got = o[f"keep{k}"] if how == "keys" else np.concatenate([o[f"keep{k}"].reshape(3, -1)[j, :cuts[j + 1] - cuts[j]] for j in range(3)])
            if not np.array_equal(got, want) or not 0 < int(want.sum()) < n:
                return False
        return paths_are_the_column_s(o["paths"], [r[0] for r in runs], two_batches=False)
    out["_nontrivial"] = nontrivial
    return out


def case_widen_keys(A):
    """An owner of 60-base keys goes on with padded keys of reads up to 96 bases: the store is the engine's, the flags the caller's."""
    n = 257
    mates = dup_reads(3, n, (96,), ragged=True)
    first = [r[:60] for r in mates[0]]
    first = [np.concatenate([r, np.full(60 - len(r), ord("A"), u8)]) for r in first]
    later = [mates[0][i] if i % 2 else first[i] for i in range(n)]         # every other record repeats a 60-base key of the first stage
    s1 = Segs(A, "stage1", [first], "uniform")
    s2 = Segs(A, "stage2", [later], "ragged")
    keep1, keep2 = A.out("keep1", u8, n), A.out("keep2", u8, n)
    A.ready()
    with Engine(segments=1) as e:
        W1, W2 = e.key_words(60, 0), e.padded_key_words(96, 0)
        rec = torch.empty(n * (W1 + 1), dtype=torch.int64, device="cuda")
        e.encode_uniform(s1.part(), n, rec)
        e.sync()
        slot = torch.as_tensor(Words(e.reserve_keys(n, 60, 0), n * W1), device="cuda")
        slot.copy_(rec.view(n, W1 + 1)[:, 1:].contiguous().view(-1))
        torch.cuda.synchronize()
        e.insert_keys(slot, n, 60, 0, keep1)
        e.sync()
        e.widen_keys(W2)
        rec = torch.zeros(n * (W2 + 1), dtype=torch.int64, device="cuda")
        e.encode_padded(s2.part(), n, 96, 0, rec)
        e.sync()
        slot = torch.as_tensor(Words(e.reserve_keys(n, W2, _lib.OPAQUE_KEYS), n * W2), device="cuda")
        slot.copy_(rec.view(n, W2 + 1)[:, 1:].contiguous().view(-1))
        torch.cuda.synchronize()
        e.insert_keys(slot, n, W2, _lib.OPAQUE_KEYS, keep2)
        e.sync()
    return dict(keep1=keep1, keep2=keep2, _nontrivial=lambda o: 0 < int(o["keep1"].sum()) < n and int(o["keep2"][0::2].sum()) == 0 and int(o["keep2"].sum()) > 0)


def case_scatter_flags(A):
    runs = []
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        rng = np.random.default_rng(n)
        m = max(1, (2 * n) // 3)
        origin = np.full(n, NONE32, u32)
        origin[np.sort(rng.permutation(n)[:m])] = rng.permutation(m).astype(u32)
        runs.append((n, A.inp(f"n{n}.flags", rng.integers(0, 2, n).astype(u8)), A.inp(f"n{n}.origin", origin), A.out(f"n{n}.keep_out", u8, m)))
    A.ready()
    with Engine(segments=1) as e:
        for n, flags, origin, keep in runs:
            e.scatter_flags(flags, origin, n, keep)
        e.sync()
    out = {f"keep{k}": r[3] for k, r in enumerate(runs)}
    out["_nontrivial"] = lambda o: 0 < int(o["keep7"].sum()) < len(o["keep7"]) and not (o["keep7"] == POISON).any()
    return out


# ---- records, join and output ------------------------------------------------------------------------------------------------------

def case_count_lines(A):
    texts = [np.frombuffer(t, u8) for _, t, _ in sc.small_cases()] + [np.frombuffer(t, u8) for _, t in sc.line_count_cases()]
    texts += [t[:k] for t in texts[:2] for k in (1, 15, 16, 17, 255, 257)]
    placed = [A.text(f"text{k}", t) for k, t in enumerate(texts)]
    A.ready()
    with Engine(segments=1) as e:
        counts = [e.count_lines(T.view, len(t)) for T, t in zip(placed, texts)]
    return dict(counts=counts, _nontrivial=lambda o: o["counts"] == [int((t == 10).sum()) for t in texts] and max(o["counts"]) > 100)


def case_scan_records(A):
    runs = []
    for k, (name, text, K) in enumerate(sc.small_cases()):
        t = np.frombuffer(text, u8)
        n_rec = int((t == 10).sum()) // K
        T = A.text(f"{name}{K}.text", t)
        arrays = [A.out(f"{name}{K}.{what}", dt, n_rec) for what, dt in (("start", u64), ("seq_off", u64), ("id_len", u32), ("seq_len", u32), ("size", u32))]
        runs.append((T, len(t), K, n_rec, arrays))
    A.ready()
    oks = []
    with Engine(segments=1) as e:
        for T, n, K, n_rec, arrays in runs:
            oks.append(e.scan_records(T.view, n, K, n_rec, *arrays))
    out = {f"{what}{k}": r[4][j] for k, r in enumerate(runs) for j, what in enumerate(("start", "seq_off", "id_len", "seq_len", "size"))}
    out["well_formed"] = oks
    out["_nontrivial"] = lambda o: all(o["well_formed"]) and any(len(np.unique(o[f"seq_len{k}"])) > 3 for k in range(len(runs)))
    return out


def id_lines_of(lines):
    """Lines back to back with 1 .. 8 newlines in front of each: (text, id_start, id_len)."""
    parts, starts, at = [], [], 0
    for k, line in enumerate(lines):
        pad = 1 + k % 8
        parts.append(b"\n" * pad)
        at += pad
        starts.append(at)
        parts.append(line)
        at += len(line)
    return np.frombuffer(b"".join(parts), u8), np.array(starts, u64), np.array([len(x) for x in lines], u32)


def case_extract_tags(A):
    text, starts, lens, _, _ = jc.extract_text()
    lines = jc.extract_lines()
    runs = []
    for tag, (t, s, l) in (("phases", (np.frombuffer(text, u8), np.array(starts, u64), np.array(lens, u32))),
                           ("flush", id_lines_of(lines)[0:3])):
        if tag == "flush":                                           # the first line starts the text, the last line ends it
            t, s = t[int(s[0]):], s - s[0]
        T = A.text(tag + ".text", t)
        n = len(s)
        runs.append((T, n, A.inp(tag + ".id_start", s + u64(T.bias)), A.inp(tag + ".id_len", l), A.out(tag + ".tag_off", u64, n), A.out(tag + ".tag_len", u32, n)))
    A.ready()
    with Engine(segments=1) as e:
        for T, n, s, l, off, ln in runs:
            e.extract_tags(T.base, s, l, n, off, ln)
        e.sync()
    out = {}
    for k, (T, n, s, l, off, ln) in enumerate(runs):
        out[f"tag_off{k}"] = lambda off=off, T=T: bits(off, u64) - u64(T.bias)
        out[f"tag_len{k}"] = ln
    out["_nontrivial"] = lambda o: len(np.unique(o["tag_len0"])) > 5
    return out


def tag_lists():
    want = ("ragged_255", "fixed_129", "heads_33", "prefix_chain", "bits_129", "census_last_161")
    lists = [(name, tags) for name, tags, _ in jc.sort_cases() if name in want]
    lists += [("stable_%d_%s" % (n, kind), jc.stable_tags(n, kind)) for n, kind in ((1, "all_equal"), (257, "period_64"), (1025, "bytes_256"))]
    return lists


def place_tags(A, tag, tags, seed=None):
    """The tags back to back (gaps of 0 .. 2 bytes with a seed), the first at byte 0, the last ending the buffer."""
    rng = random.Random(seed)
    parts, offs, at = [], [], 0
    for k, t in enumerate(tags):
        gap = rng.randrange(3) if seed is not None and k else 0
        parts.append(b"\xEE" * gap)
        at += gap
        offs.append(at)
        parts.append(bytes(t))
        at += len(t)
    T = A.text(tag + ".bytes", np.frombuffer(b"".join(parts), u8))
    return (T.base, A.inp(tag + ".offsets", np.array(offs, u64) + u64(T.bias)), A.inp(tag + ".lengths", np.array([len(t) for t in tags], u32)), len(tags))


def case_sort_tags(A):
    runs = []
    for name, tags in tag_lists():
        runs.append((place_tags(A, name, tags, seed=1), A.out(name + ".perm", u32, len(tags))))
    A.ready()
    with Engine(segments=1) as e:
        for t, perm in runs:
            e.sort_tags(*t, perm)
        e.sync()
    out = {f"perm{k}": r[1] for k, r in enumerate(runs)}
    out["_nontrivial"] = lambda o: all(np.array_equal(np.sort(o[f"perm{k}"]), np.arange(len(o[f"perm{k}"]))) for k in range(len(runs))) and \
        any(not np.array_equal(o[f"perm{k}"], np.arange(len(o[f"perm{k}"]))) for k in range(len(runs)))
    return out


def case_join_tags(A):
    want = ("heads_33", "heads_lengths_differ", "run_00_short", "run_03_hex30", "pairs_2049_alternating")
    runs = []
    for name, a, b, _ in jc.join_cases():
        if name not in want:
            continue
        ta, tb = place_tags(A, name + ".a", a, seed=2), place_tags(A, name + ".b", b)
        na, nb = len(a), len(b)
        outs = [A.out(f"{name}.{what}", u32, cnt) for what, cnt in (("perm_a", na), ("perm_b", nb), ("match_a", na), ("match_b", nb),
                                                                    ("pair_a", min(na, nb)), ("pair_b", min(na, nb)))]
        runs.append((ta, tb, outs))
    assert len(runs) == len(want)
    A.ready()
    pairs = []
    with Engine(segments=1) as e:
        for ta, tb, outs in runs:
            pairs.append(e.join_tags(ta, tb, *outs))
    out = {f"{what}{k}": r[2][j] for k, r in enumerate(runs) for j, what in enumerate(("perm_a", "perm_b", "match_a", "match_b", "pair_a", "pair_b"))}
    out["n_pairs"] = pairs
    out["_nontrivial"] = lambda o: max(o["n_pairs"]) > 100 and (o["match_a4"].view(u32) == NONE32).any()
    return out


def case_count_tags_le(A):
    lists = tag_lists()
    placed = [(place_tags(A, name, tags, seed=3), place_tags(A, name + ".other", tags[::-1][:7] + [b"", b"\xff"])) for name, tags in lists]
    A.ready()
    counts = []
    with Engine(segments=1) as e:
        for t, other in placed:
            counts.append([e.count_tags_le(t, other, k) for k in range(other[3])])
    return dict(counts=counts, _nontrivial=lambda o: len({c for row in o["counts"] for c in row}) > 10)


def case_sample_tags(A):
    runs = []
    for name, tags in tag_lists():
        n = len(tags)
        for n_samples, stride in ((1, 1), (min(n, 7), 16), (min(n, 64), 33)):
            t = f"{name}.s{n_samples}x{stride}"
            runs.append((place_tags(A, t, tags, seed=4), n_samples, stride, A.out(t + ".out_bytes", u8, n_samples * stride), A.out(t + ".out_len", u32, n_samples)))
    A.ready()
    with Engine(segments=1) as e:
        for t, n_samples, stride, ob, ol in runs:
            e.sample_tags(t, n_samples, stride, ob, ol)
        e.sync()
    out = {}
    for k, (t, n_samples, stride, ob, ol) in enumerate(runs):
        out[f"len{k}"] = ol
        out[f"bytes{k}"] = ob
    # the bytes of a sample behind its length are not promised: compare only the tag's own
    out["_mask"] = {f"bytes{k}": (lambda r=r: (np.arange(r[2])[None, :] < bits(r[4], u32)[:, None]).reshape(-1)) for k, r in enumerate(runs)}
    out["_nontrivial"] = lambda o: any(len(np.unique(o[f"len{k}"])) > 1 for k in range(len(runs)))
    return out


def case_classify_tags(A):
    runs = []
    for name, tags in tag_lists():
        for n_split in (1, 7, 64):
            split = sorted({bytes(t)[:256] for t in tags})
            split = sorted(split[(k * len(split)) // n_split] for k in range(n_split))
            stride = max(1, max(len(s) for s in split))
            sb = np.full(max(1, (n_split - 1) * stride + len(split[-1])), 0xEE, u8)       # the last splitter ends the buffer (an empty one: one byte, no null pointer)
            for k, s in enumerate(split):
                sb[k * stride:k * stride + len(s)] = np.frombuffer(s, u8)
            t = f"{name}.k{n_split}"
            runs.append((place_tags(A, t, tags, seed=5), A.inp(t + ".split_bytes", sb), stride, A.inp(t + ".split_len", np.array([len(s) for s in split], u32)),
                         n_split, A.out(t + ".range", u32, len(tags))))
    A.ready()
    with Engine(segments=1) as e:
        for t, sb, stride, sl, n_split, rng_out in runs:
            e.classify_tags(t, sb, stride, sl, n_split, rng_out)
        e.sync()
    out = {f"range{k}": r[5] for k, r in enumerate(runs)}
    out["_nontrivial"] = lambda o: sum(len(np.unique(o[f"range{k}"])) > 3 for k in range(len(runs))) > 3
    return out


COUNTS = (1, 63, 64, 65, 255, 256, 257, 1025)


def case_range_keep(A):
    runs = [(n, A.inp(f"n{n}.range", np.random.default_rng(n).integers(0, 3, n).astype(u32)), A.out(f"n{n}.keep", u8, n)) for n in COUNTS]
    A.ready()
    with Engine(segments=1) as e:
        counts = [e.range_keep(r, n, 1, keep) for n, r, keep in runs]
    out = {f"keep{k}": r[2] for k, r in enumerate(runs)}
    out["counts"] = counts
    out["_nontrivial"] = lambda o: o["counts"] == [int(o[f"keep{k}"].sum()) for k in range(len(runs))] and 0 < o["counts"][-1] < 1025
    return out


def case_max_u32(A):
    runs = []
    for n in COUNTS:
        v = np.random.default_rng(n).integers(0, 1 << 31, n).astype(u32)
        v[-1] = 0xFFFFFF00 + n % 7                                    # the largest is the last entry
        runs.append((n, A.inp(f"n{n}.values", v)))
    A.ready()
    with Engine(segments=1) as e:
        got = [e.max_u32(v, n) for n, v in runs]
    return dict(max=got, _nontrivial=lambda o: o["max"] == [0xFFFFFF00 + n % 7 for n in COUNTS])


def case_gather_seqs(A):
    runs = []
    for n in COUNTS:
        rng = np.random.default_rng(n)
        rows = max(1, n // 2)
        runs.append((n, A.inp(f"n{n}.idx", rng.integers(0, rows, n).astype(u32)), A.inp(f"n{n}.off_table", rng.integers(2 ** 32, 2 ** 44, rows, dtype=u64)),
                     A.inp(f"n{n}.len_table", rng.integers(0, 2 ** 32, rows, dtype=u64).astype(u32)), A.out(f"n{n}.off_out", u64, n), A.out(f"n{n}.len_out", u32, n)))
    A.ready()
    with Engine(segments=1) as e:
        for n, idx, ot, lt, oo, lo in runs:
            e.gather_seqs(idx, n, ot, lt, oo, lo)
        e.sync()
    out = {f"{what}{k}": r[4 + j] for k, r in enumerate(runs) for j, what in enumerate(("off", "len"))}
    out["_nontrivial"] = lambda o: len(np.unique(o["off7"])) > 100 and int(o["off7"].view(u64).min()) >= 2 ** 32
    return out


SPAN_LENGTHS = [0, 1, 15, 16, 17, 31, 33, 300]


def case_copy_spans(A):
    """Every rotation of the span lengths, so that each length is once the first span (flush with dst's start) and once the last
    (flush with its end); the sources lie at every address mod 16 and the first and last source bytes are span bytes too."""
    rng = np.random.default_rng(1)
    runs = []
    for r in range(len(SPAN_LENGTHS)):
        lens = np.array((SPAN_LENGTHS[r:] + SPAN_LENGTHS[:r]) * 3, u32)
        n = len(lens)
        gaps = rng.integers(0, 5, n)
        gaps[0] = 0
        src_off = (np.cumsum(gaps + lens) - lens).astype(u64)
        src = rng.integers(1, 255, int(src_off[-1] + lens[-1]), dtype=u8)
        order = rng.permutation(n)                                     # the spans are not copied in source order
        dst_off = np.zeros(n, u64)
        dst_off[order] = (np.cumsum(lens[order]) - lens[order]).astype(u64)
        T = A.text(f"r{r}.src", src)
        runs.append((n, T, A.inp(f"r{r}.src_off", src_off + u64(T.bias)), A.inp(f"r{r}.len", lens), A.out(f"r{r}.dst", u8, int(lens.sum())),
                     A.inp(f"r{r}.dst_off", dst_off), src, src_off, lens, dst_off))
    A.ready()
    with Engine(segments=1) as e:
        for n, T, so, ln, dst, do, *_ in runs:
            e.copy_spans(T.base, so, ln, n, dst, do)
        e.sync()
    out = {f"dst{k}": r[4] for k, r in enumerate(runs)}

    def nontrivial(o):
        for k, (n, T, so, ln, dst, do, src, src_off, lens, dst_off) in enumerate(runs):
            want = np.zeros(int(lens.sum()), u8)
            for s, l, d in zip(src_off, lens, dst_off):
                want[int(d):int(d) + int(l)] = src[int(s):int(s) + int(l)]
            if not np.array_equal(o[f"dst{k}"], want):
                return False
        return True
    out["_nontrivial"] = nontrivial
    return out


def labelled_records(seed, n, annotated):
    """n FASTQ records whose ID lines' first words end at every place mod 16; annotated: every third carries `;size=<k>`."""
    rng = random.Random(seed)
    recs, label_at, cut = [], [], []
    for i in range(n):
        word = b"@" + bytes(rng.choice(b"abcdefgh0123:") for _ in range(i % 40))
        ann = b";size=%d" % rng.choice([1, 9, 10, 99, 12345, 2 ** 31 - 1]) if annotated and i % 3 == 0 else b""
        rest = rng.choice([b"", b" 1:N:0", b"\tx", b" " + b"c" * 70])
        L = SPAN_LENGTHS[i % 8] if i % 2 else rng.randrange(1, 152)
        seq = bytes(rng.choice(b"ACGT") for _ in range(L))
        recs.append(word + ann + rest + b"\n" + seq + b"\n+\n" + b"I" * L + b"\n")
        label_at.append(len(word))
        cut.append(len(ann))
    return recs, np.array(label_at, u32), np.array(cut, u32)


def case_copy_labelled(A, relabel):
    runs = []
    for n in (1, 63, 65, 257):
        recs, label_at, cut = labelled_records(n, n, relabel)
        rng = np.random.default_rng(n)
        size = rng.choice(np.array([1, 9, 10, 99, 100, 54321, 2 ** 31 - 1], u32), n)
        keep = rng.random(n) < 0.7
        keep[0] = keep[-1] = True
        rec_size = np.array([len(r) for r in recs], u32)
        digits = np.array([len(str(int(s))) for s in size], u32)
        lens = np.where(keep, rec_size - cut + 6 + digits, 0).astype(u32)
        src_off = (np.cumsum(rec_size) - rec_size).astype(u64)
        dst_off = (np.cumsum(lens) - lens).astype(u64)
        T = A.text(f"n{n}.src", np.frombuffer(b"".join(recs), u8))
        t = f"n{n}"
        runs.append((n, T, A.inp(t + ".src_off", src_off + u64(T.bias)), A.inp(t + ".len", lens), A.inp(t + ".label_at", label_at),
                     A.inp(t + ".cut", cut) if relabel else None, A.inp(t + ".size", size), A.out(t + ".dst", u8, int(lens.sum())), A.inp(t + ".dst_off", dst_off)))
    A.ready()
    with Engine(segments=1) as e:
        for n, T, so, ln, la, cut, size, dst, do in runs:
            if relabel:
                e.copy_relabelled(T.base, so, ln, la, cut, size, n, dst, do)
            else:
                e.copy_labelled(T.base, so, ln, la, size, n, dst, do)
        e.sync()
    out = {f"dst{k}": r[7] for k, r in enumerate(runs)}
    out["_nontrivial"] = lambda o: all(not (o[f"dst{k}"] == POISON).any() and bytes(o[f"dst{k}"]).count(b";size=") == int((bits(r[3], u32) > 0).sum())
                                       for k, r in enumerate(runs))
    return out


def case_output_plan(A, offsets):
    runs = []
    for n in (1, 9, 513, 2049):
        for keep_kind in ("random", "alternating", "last"):
            if keep_kind not in pc.keeps_for(n):
                continue
            for size_kind in pc.SIZES:
                c = pc.make(n, keep_kind, size_kind)
                t = f"n{n}.{keep_kind}.{size_kind}"
                ins = [A.inp(t + ".keep", c["keep"]), A.inp(t + ".idx", c["idx"]), A.inp(t + ".sizes", c["sizes"])]
                if offsets:
                    outs = [A.out(t + ".dest", u64, c["n_rec"], preset=0x0123456789ABCDEF)]
                else:
                    ins.append(A.inp(t + ".starts", c["starts"]))
                    outs = [A.out(t + ".src_off", u64, n), A.out(t + ".len", u32, n), A.out(t + ".dst_off", u64, n)]
                runs.append((n, ins, outs))
    A.ready()
    totals = []
    with Engine(segments=1) as e:
        for n, ins, outs in runs:
            if offsets:
                totals.append(e.output_offsets(ins[0], ins[1], n, ins[2], outs[0]))
            else:
                totals.append(e.output_plan(ins[0], ins[1], n, ins[3], ins[2], *outs))
    out = {f"out{k}.{j}": t for k, r in enumerate(runs) for j, t in enumerate(r[2])}
    out["totals"] = totals
    out["_nontrivial"] = lambda o: max(o["totals"]) > 2 ** 32 and any((o[f"out{k}.0"].view(u64) == 0x0123456789ABCDEF).any() for k in range(len(runs))) == offsets
    return out


# ---- codecs --------------------------------------------------------------------------------------------------------------------------

def case_bgzf_deflate(A, effort):
    big = bgzf_cases.fastq_text(420, 1)
    rnd = np.random.default_rng(7).integers(0, 256, 70_001, dtype=u8).tobytes()
    texts = [(b"@", 4), (bgzf_cases.fastq_text(10, 2), 4), (big[:65279], 4), (big[:65280], 4), (big[:65281], 4), (bgzf_cases.fasta_text(300, 5), 2), (rnd, 4)]
    with Engine(segments=1) as e:
        runs = [(A.inp(f"t{k}.src", np.frombuffer(t, u8)), len(t), lines, A.out(f"t{k}.dst", u8, e.bgzf_bound(len(t)))) for k, (t, lines) in enumerate(texts)]
        A.ready()
        sizes = [e.bgzf_deflate(src, n, dst, lines, effort) for src, n, lines, dst in runs]          # dst_capacity = dst.numel() = the bound, exactly
    out = {f"dst{k}": r[3] for k, r in enumerate(runs)}
    out["sizes"] = sizes

    def nontrivial(o):
        for k, (t, _) in enumerate(texts):
            if gunzip_all(bytes(o[f"dst{k}"][:o["sizes"][k]])) != t or not (o[f"dst{k}"][o["sizes"][k]:] == POISON).all():
                return False
        return o["sizes"][3] < 65280 and o["sizes"][6] > 70000
    out["_nontrivial"] = nontrivial
    return out


def gunzip_all(raw):
    out = b""
    while raw:
        d = zlib.decompressobj(31)
        out += d.decompress(raw)
        raw = d.unused_data
    return out


def walk(raw):
    """comp_off, comp_len, out_off, out_len, crc of every BGZF member with data."""
    rows, at, out = [], 0, 0
    while at < len(raw):
        total = struct.unpack_from("<H", raw, at + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", raw, at + total - 8)
        if isize:
            rows.append((at + 18, total - 26, out, isize, crc))
            out += isize
        at += total
    a = np.array(rows, u64).reshape(-1, 5)
    return a[:, 0].copy(), a[:, 1].astype(u32), a[:, 2].copy(), a[:, 3].astype(u32), a[:, 4].astype(u32), out


def damaged_members(n_members):
    """A damaged member between two good ones, and the last one."""
    return (1, n_members - 1)


def inflate_inputs():
    def make():
        want = ("level1", "stored", "fixed_huffman", "tiny_members", "short_periods", "one_byte", "empty_members_between", "members_of_64k")
        got = [(name, data, raw) for name, data, raw in inflate_cases.cases() if name in want]
        name, data, raw = got[0]
        co, cl, *_ = walk(raw)
        dmg = bytearray(raw)
        assert len(co) >= 4
        for m in damaged_members(len(co)):
            dmg[int(co[m]) + int(cl[m]) // 2] ^= 0x10
        return got + [("damaged", data, bytes(dmg))]
    return cached("inflate", make)


def case_bgzf_inflate(A, use_async):
    runs = []
    for name, data, raw in inflate_inputs():
        co, cl, oo, ol, crc, total = walk(raw)
        last = int(co[-1]) + int(cl[-1])                              # comp ends with the last member's stream: no trailer, no slack
        comp = A.text(name + ".comp", np.frombuffer(raw, u8)[:last])
        text = A.text(name + ".text", total, role="out")              # exactly sum(out_len) bytes
        args = [A.inp(name + ".comp_off", co + u64(comp.bias)), A.inp(name + ".comp_len", cl), A.inp(name + ".out_off", oo + u64(text.bias)),
                A.inp(name + ".out_len", ol), A.inp(name + ".crc", crc)]
        bad = A.inout(name + ".bad_counters", np.zeros(2, u64)) if use_async else None
        runs.append((name, comp, text, args, len(co), bad, data))
    A.ready()
    n_bad = []
    with Engine(segments=1) as e:
        for name, comp, text, args, n, bad, data in runs:
            if use_async:
                e._p(comp.base)                                        # orders the engine behind torch's copies, as every binding call does
                e._check(e._L.fqd_bgzf_inflate_async(e._h, comp.base.data_ptr(), *[a.data_ptr() for a in args], n, text.base.data_ptr(), bad.data_ptr()))
            else:
                n_bad.append(e.bgzf_inflate(comp.base, *args, n, text.base))
        e.sync()
    out = {"n_bad": n_bad if not use_async else (lambda: [int(bits(r[5], u64).sum()) for r in runs])}
    mask = {}
    for k, (name, comp, text, args, n, bad, data) in enumerate(runs):
        out[f"text{k}"] = text.view
        if name == "damaged":                                          # a damaged member's own out_len bytes mean nothing; every other byte does
            _, _, oo, ol, _, _ = walk(inflate_inputs()[-1][2])
            undamaged = np.ones(len(data), bool)
            for m in damaged_members(len(oo)):
                undamaged[int(oo[m]):int(oo[m]) + int(ol[m])] = False
            assert 0 < int((~undamaged).sum()) < len(data) // 4
            mask[f"text{k}"] = undamaged
    out["_mask"] = mask

    def nontrivial(o):
        want = np.frombuffer(runs[-1][6], u8)
        return o["n_bad"][:-1] == [0] * (len(runs) - 1) and o["n_bad"][-1] >= 1 and all(bytes(o[f"text{k}"]) == r[6] for k, r in enumerate(runs[:-1])) \
            and np.array_equal(o[f"text{len(runs) - 1}"], np.where(undamaged, want, 0))       # the neighbours of a damaged member hold their own text
    out["_nontrivial"] = nontrivial
    return out


def gunzip_header_len(raw):
    flg, at = raw[3], 10
    if flg & 4:
        at += 2 + struct.unpack_from("<H", raw, at)[0]
    if flg & 8:
        at = raw.index(b"\0", at) + 1
    if flg & 16:
        at = raw.index(b"\0", at) + 1
    if flg & 2:
        at += 2
    return at


def case_gunzip(A, room, arriving=False):
    """room 0: text_cap is the text's size exactly; -1: one byte too small, which must give ok = 0.  The packed input is followed
    by its documented 32 readable bytes and nothing more."""
    def make():
        fq, fa = bgzf_cases.fastq_text(600, 3), bgzf_cases.fasta_text(300, 5)
        m = gunzip_cases.member
        return [("level6", fq, m(fq, 6)), ("level1", fq, m(fq, 1)), ("fixed", fq[:70_000], m(fq[:70_000], 6, zlib.Z_FIXED)),
                ("header_fields", fa, m(fa, 6, header=gunzip_cases.header_with_fields())), ("flushes", fq, m(fq, 6, flush_every=30_001)),
                ("two_members", fq[:50_000] + fa, m(fq[:50_000], 6) + m(fa, 9)), ("tiny", b"@r\nACGT\n+\nIIII\n", m(b"@r\nACGT\n+\nIIII\n", 6))]
    runs = []
    for name, data, raw in cached("gunzip", make):
        h = gunzip_header_len(raw)
        packed = A.text(name + ".deflate", np.frombuffer(raw[h:] + b"\0" * 32, u8))
        runs.append((packed, len(raw) - h, A.text(name + ".text", len(data) + room, role="out"), data))
    A.ready()
    got = []
    with Engine(segments=1) as e:
        for packed, avail, text, data in runs:
            ok, n, used, crc = e.gunzip(packed.view, avail, text.view, arrived=C.c_uint64(avail) if arriving else None)
            got.append((ok, n if ok else 0, used if ok else 0, crc if ok else 0))
        e.sync()
    out = {"results": got}
    if room == 0:
        out.update({f"text{k}": r[2].view for k, r in enumerate(runs)})
    out["_nontrivial"] = lambda o: all(g[0] == (room == 0) for g in o["results"]) and (room < 0 or all(bytes(o[f"text{k}"]) == r[3] for k, r in enumerate(runs)))
    return out


# ---- the linked-mode stages over one resident text -------------------------------------------------------------------------------

def resident_run():
    """One FASTQ file of 257 records for every linked-mode stage: clusters of exact copies (1, 2, 3, 9 and 65 members, reads of 31,
    33, 150 and 151 bases, qualities of their own) dealt to record numbers at random; ID lines of the seven Illumina fields with
    a UMI as the eighth, the members of a cluster a few pixels apart, two UMIs a cluster one substitution apart; a few clusters
    one substitution from another one.  Host arrays: the record scan's, the exact owners, (perm, head), sizes."""
    def make():
        rng = random.Random(12)
        sizes = [65, 9, 9, 3, 3, 2, 2, 2, 1, 1, 1, 1] + [2] * 20 + [1] * 50 + [3] * 16 + [9] * 2 + [1] * 2
        clusters, names, umis = [], [], []
        for k, m in enumerate(sizes):
            L = (150, 151, 33, 31)[k % 4]
            if k % 5 == 4:                                             # one substitution from the cluster four before it (same length), under its UMIs
                t = near_cases.substituted(clusters[k - 4][0][0], [L // 2], rng)
                umi, near = umis[k - 4]
            else:
                t = cc.template(rng, L)
                umi = bytes(rng.choice(b"ACGT") for _ in range(8))
                near = near_cases.substituted(umi, [3], rng)
            umis.append((umi, near))
            clusters.append([(t, cc.qualities(rng, L, pool=b"#+5:?DII~")) for _ in range(m)])
            x0, y0 = rng.randrange(1000, 30000), rng.randrange(1000, 30000)
            names.append([oc.id_line(oc.SURFACE if k % 7 else b"M01:7:FC1:2", 1101 + k % 3, x0 + rng.randrange(0, 40) * (j % 3), y0 + rng.randrange(0, 8),
                                     behind=b":" + (umi if j % 4 else near))[1:-1] for j in range(m)])
        assert sum(sizes) == 257
        rows, perm, head = cc.scattered(rng, clusters)
        where = {id(member): (c, j) for c, cl in enumerate(clusters) for j, member in enumerate(cl)}      # scattered() deals the member objects themselves
        flat_names = [names[c][j] for c, j in (where[id(row)] for row in rows)]
        text, start, size, seq_off, seq_len = cc.laid_out(rows, align=1, rng=random.Random(3), names=flat_names)
        text = np.frombuffer(bytes(text), u8)[:int(start[-1]) + int(size[-1])].copy()      # the last record ends the text
        n = len(rows)
        seqs = [rows[i][0] for i in range(n)]
        owner = first_index(seqs)
        umis = [flat_names[i].split(b":")[7].split(b" ")[0] for i in range(n)]
        owner_exact = first_index(list(zip(umis, seqs)))
        csize = np.zeros(n, u32)
        for r, o in enumerate(owner):
            csize[o] += 1
        esize = np.zeros(n, u32)
        for o in owner_exact:
            esize[o] += 1
        return dict(n=n, text=text, start=start, size=size, seq_off=seq_off, seq_len=seq_len, id_len=(seq_off - start).astype(u32), perm=perm, head=head,
                    owner=owner, owner_exact=owner_exact, csize=csize, esize=esize, seqs=seqs, rows=rows, names=flat_names)
    return cached("resident", make)


class Resident:
    """The resident run's text and arrays placed through the allocator; the offsets carry the text's bias."""
    def __init__(self, A, want, role="in"):
        self.R = R = resident_run()
        self.n = R["n"]
        self.T = A.text("text", R["text"], role)
        self.text = self.T.base
        for name in want:
            a = R[name]
            if name in ("start", "seq_off"):
                a = a + u64(self.T.bias)
            setattr(self, name, A.inp(name, a))


def groups_of(owner):
    """(perm, head) of fqd_group_owners' statement."""
    order = np.lexsort((np.arange(len(owner)), owner))
    head = np.ones(len(owner), u8)
    head[1:] = owner[order][1:] != owner[order][:-1]
    return order.astype(u32), head


def upstream(key, fn):
    """A stage's input that an earlier stage makes: computed once on plain tensors."""
    return cached(("upstream", key), fn)


def plain_umi_find():
    def make():
        R = resident_run()
        A = Alloc("plain")
        X = Resident(A, ["start", "id_len"])
        off = A.out("umi_off", u32, X.n)
        with Engine(segments=1) as e:
            info = e.umi_find(X.text, X.start, X.id_len, X.n, ":", off)
        return bits(off, u32).copy(), info
    return upstream("umi_find", make)


def plain_places():
    def make():
        A = Alloc("plain")
        X = Resident(A, ["start", "id_len"])
        outs = [A.out(w, u32, X.n) for w in ("tile", "x", "y", "surface")]
        with Engine(segments=1) as e:
            info = e.read_places(X.text, X.start, X.id_len, X.n, *outs)
        assert info.bad_record == _lib.UMI_NO_RECORD
        return [bits(t, u32).copy() for t in outs]
    return upstream("places", make)


def case_owners(A):
    R = resident_run()
    n = R["n"]
    keep = (R["owner"] == np.arange(n)).astype(u8)
    link = np.full(n, P32, u32)                                        # a link names ANY earlier record of the key: the one before, or the first
    members = {}
    for i, o in enumerate(R["owner"]):
        members.setdefault(int(o), []).append(i)
        if not keep[i]:
            link[i] = members[int(o)][-2] if i % 2 else int(o)
    d_keep, d_link, owner = A.inp("keep", keep), A.inp("link", link), A.out("owner", u32, n)
    A.ready()
    with Engine(segments=1) as e:
        e.owners(d_keep, d_link, n, owner)
    return dict(owner=owner, _nontrivial=lambda o: np.array_equal(o["owner"].view(u32), R["owner"]) and int(keep.sum()) < n)


def case_group_owners(A):
    R = resident_run()
    runs = [(n, A.inp(f"n{n}.owner", R["owner"][:n]), A.out(f"n{n}.perm", u32, n), A.out(f"n{n}.head", u8, n)) for n in (1, 63, 64, 65, 255, 256, 257)]
    A.ready()
    with Engine(segments=1) as e:
        clusters = [e.group_owners(o, n, p, h) for n, o, p, h in runs]
    out = {f"perm{k}": r[2] for k, r in enumerate(runs)}
    out.update({f"head{k}": r[3] for k, r in enumerate(runs)})
    out["clusters"] = clusters
    want = groups_of(R["owner"])
    out["_nontrivial"] = lambda o: np.array_equal(o["perm6"].view(u32), want[0]) and np.array_equal(o["head6"], want[1]) and 1 < o["clusters"][6] < 257
    return out


def case_heads_to_keep(A):
    R = resident_run()
    n = R["n"]
    perm, head, keep = A.inp("perm", R["perm"]), A.inp("head", R["head"]), A.out("keep", u8, n)
    A.ready()
    with Engine(segments=1) as e:
        e.heads_to_keep(perm, head, n, keep)
    return dict(keep=keep, _nontrivial=lambda o: 0 < int(o["keep"].sum()) < n and set(o["keep"].tolist()) == {0, 1})


def case_owners_to_keep(A):
    R = resident_run()
    runs = [(n, A.inp(f"n{n}.owner", R["owner"][:n]), A.out(f"n{n}.keep", u8, n)) for n in (1, 63, 64, 65, 255, 256, 257)]
    A.ready()
    with Engine(segments=1) as e:
        for n, o, k in runs:
            e.owners_to_keep(o, n, k)
        e.sync()
    out = {f"keep{k}": r[2] for k, r in enumerate(runs)}
    out["_nontrivial"] = lambda o: np.array_equal(o["keep6"], (R["owner"] == np.arange(257)).astype(u8)) and 0 < int(o["keep6"].sum()) < 257
    return out


def case_cluster_sizes(A, weighted):
    R = resident_run()
    n = R["n"]
    perm, head, size = A.inp("perm", R["perm"]), A.inp("head", R["head"]), A.out("size", u32, n)
    weight = A.inp("weight", (1 + np.arange(n) % 5).astype(u32)) if weighted else None
    A.ready()
    with Engine(segments=1) as e:
        if weighted:
            levels, over = e.cluster_weights(perm, head, weight, n, size)
            extra = [over.over_record, over.over_sum]
        else:
            levels, extra = e.cluster_sizes(perm, head, n, size), []
    return dict(size=size, levels=list(levels.clusters) + list(levels.records) + [levels.largest] + extra,
                _nontrivial=lambda o: int(o["size"].view(u32).max()) >= 65 and int((o["size"].view(u32) == 0).sum()) > 0)


def case_size_labels(A):
    X = Resident(A, ["start", "id_len", "size"])
    R = X.R
    keep = A.inp("keep", R["head"][np.argsort(R["perm"])])
    csize = A.inp("csize", np.where(R["csize"] > 0, R["csize"] * 37, 0).astype(u32))
    label_at, out_size = A.out("label_at", u32, X.n), A.out("out_size", u32, X.n)
    A.ready()
    with Engine(segments=1) as e:
        e.size_labels(X.text, X.start, X.id_len, X.size, keep, csize, X.n, label_at, out_size)
    return dict(label_at=label_at, out_size=out_size,
                _nontrivial=lambda o: len(np.unique(o["label_at"])) >= 3 and len(np.unique(o["out_size"].view(u32) - R["size"])) >= 3)


def case_size_filter(A):
    R = resident_run()
    n = R["n"]
    size = A.inp("size", R["csize"])
    keep = A.inout("keep", (R["csize"] > 0).astype(u8))
    A.ready()
    with Engine(segments=1) as e:
        dropped = e.size_filter(size, n, 2, 9, keep)
    return dict(keep=keep, dropped=list(dropped), _nontrivial=lambda o: o["dropped"][0] > 0 and 0 < int(o["keep"].sum()) < int((R["csize"] > 0).sum()))


def case_size_order(A, ex):
    R = resident_run()
    n = R["n"]
    csize = R["csize"].copy()
    csize[csize == 65] = 300                                           # one cluster above 255 members: the second tier has work
    keep = (csize > 0) & (np.arange(n) % 7 != 3)
    perm, head, size, d_keep = A.inp("perm", R["perm"]), A.inp("head", R["head"]), A.inp("size", csize), A.inp("keep", keep.astype(u8))
    order = A.out("order", u32, n)
    A.ready()
    with Engine(segments=1) as e:
        if ex:
            W, info = e.size_order_info(perm, head, size, d_keep, n, order)
            extra = [info.written, info.large, info.largest, info.tier2_passes]
        else:
            W, extra = e.size_order(perm, head, size, d_keep, n, order), []
    return dict(order=order, written=[W] + extra, _nontrivial=lambda o: 1 < o["written"][0] < n and int((o["order"].view(u32) == P32).sum()) == n - o["written"][0])


def case_take_u32(A):
    runs = []
    for n in COUNTS:
        rng = np.random.default_rng(n)
        rows = max(1, n // 2)
        runs.append((n, A.inp(f"n{n}.values", rng.integers(0, 2 ** 32, rows, dtype=u64).astype(u32)), A.inp(f"n{n}.idx", rng.integers(0, rows, n).astype(u32)),
                     A.out(f"n{n}.out", u32, n)))
    A.ready()
    with Engine(segments=1) as e:
        for n, v, i, o in runs:
            e.take_u32(v, i, n, o)
        e.sync()
    out = {f"out{k}": r[3] for k, r in enumerate(runs)}
    out["_nontrivial"] = lambda o: len(np.unique(o["out7"])) > 100
    return out


def sizein_file(A):
    recs, label_at, cut = labelled_records(9, 257, True)
    rec_size = np.array([len(r) for r in recs], u32)
    start = (np.cumsum(rec_size) - rec_size).astype(u64)
    id_len = np.array([r.index(b"\n") + 1 for r in recs], u32)
    T = A.text("text", np.frombuffer(b"".join(recs), u8))
    return T, start, id_len, rec_size, label_at, cut


def case_size_annotations(A, with_expect):
    """with_expect: the call over file 2, which holds file 1's weights against the annotations it meets."""
    T, start, id_len, rec_size, label_at, cut = sizein_file(A)
    n = len(start)
    d_start, d_len = A.inp("start", start + u64(T.bias)), A.inp("id_len", id_len)
    weights = [re.search(rb";size=(\d+)", r[:int(l)]) for r, l in zip(labelled_records(9, 257, True)[0], id_len)]
    expect = A.inp("expect", np.array([int(m.group(1)) if m else 1 + k % 5 for k, m in enumerate(weights)], u32)) if with_expect else None
    outs = [A.out(w, u32, n) for w in ("weight", "label_at", "cut")]
    A.ready()
    with Engine(segments=1) as e:
        info = e.size_annotations(T.base, d_start, d_len, n, expect, *outs)
    return dict(weight=outs[0], label_at=outs[1], cut=outs[2], info=[info.bad_record, info.bad_reason, info.annotated, info.total_weight],
                _nontrivial=lambda o: o["info"][0] == _lib.UMI_NO_RECORD and o["info"][2] == 86 and np.array_equal(o["label_at"].view(u32), label_at)
                and np.array_equal(o["cut"].view(u32), cut))


def case_size_relabel(A):
    runs = []
    for n in COUNTS:
        rng = np.random.default_rng(n)
        runs.append((n, A.inp(f"n{n}.rec_size", rng.integers(40, 400, n).astype(u32)), A.inp(f"n{n}.keep", (rng.random(n) < 0.6).astype(u8)),
                     A.inp(f"n{n}.size", rng.choice(np.array([1, 9, 10, 99, 100, 2 ** 31 - 1], u32), n)), A.inp(f"n{n}.cut", rng.integers(0, 17, n).astype(u32)),
                     A.out(f"n{n}.out_size", u32, n)))
    A.ready()
    with Engine(segments=1) as e:
        for n, rs, k, s, c, o in runs:
            e.size_relabel(rs, k, s, c, n, o)
    out = {f"out_size{k}": r[5] for k, r in enumerate(runs)}
    out["_nontrivial"] = lambda o: len(np.unique(o["out_size7"])) > 50
    return out


def case_canonical_reads(A, S, layout):
    runs = []
    for n, L in SHAPES:
        lens = mate_lengths(L, S)
        mates = dup_reads(5 * n + L, n, lens, ragged=layout == "ragged")
        segs = Segs(A, f"n{n}L{L}", mates, layout)
        total = sum(len(r) for m in mates for r in m)
        t = f"n{n}L{L}"
        outs = dict(out=A.out(t + ".out", u8, total), off0=A.out(t + ".out_off0", u64, n), len0=A.out(t + ".out_len0", u32, n), flipped=A.out(t + ".flipped", u8, n),
                    off1=A.out(t + ".out_off1", u64, n) if S == 2 else None, len1=A.out(t + ".out_len1", u32, n) if S == 2 else None)
        runs.append((n, segs, outs))
    A.ready()
    turned = []
    with Engine(segments=S) as e:
        for n, segs, o in runs:
            turned.append(e.canonical_reads(segs.part(), n, o["out"], o["off0"], o["len0"], o["flipped"], o["off1"], o["len1"], count=True))
    out = {f"{name}{k}": t for k, r in enumerate(runs) for name, t in r[2].items() if t is not None}
    out["turned"] = turned
    out["_nontrivial"] = lambda o: all(0 < t < r[0] for t, r in zip(o["turned"][1:], runs[1:])) and not (o["out7"] == POISON).any()
    return out


def case_umi_find(A):
    X = Resident(A, ["start", "id_len"])
    off = A.out("umi_off", u32, X.n)
    A.ready()
    with Engine(segments=1) as e:
        info = e.umi_find(X.text, X.start, X.id_len, X.n, ":", off)
    return dict(umi_off=off, info=[info.n_bases, info.umi_len, info.joiners, info.bad_record, info.bad_reason],
                _nontrivial=lambda o: o["info"] == [8, 8, 0, _lib.UMI_NO_RECORD, 0] and len(np.unique(o["umi_off"])) >= 3)


def case_umi_reads(A, layout):
    R = resident_run()
    umi_off, info = plain_umi_find()
    X = Resident(A, ["start"])
    if layout == "ragged":                                             # the sequences where they lie in the text
        mate = Reads(X.text, offsets=A.inp("seq_off", R["seq_off"] + u64(X.T.bias)), lengths=A.inp("seq_len", R["seq_len"]))
    else:
        reads = [np.frombuffer(s[:31], u8) for s in R["seqs"]]
        mate = Reads(A.inp("bases", uniform_bytes(reads, 31)), uniform_len=31, uniform_stride=31)
    total = int(sum(len(s) if layout == "ragged" else 31 for s in R["seqs"])) + 8 * X.n
    d_off = A.inp("umi_off", umi_off)
    out, out_off, out_len = A.out("out", u8, total), A.out("out_off", u64, X.n), A.out("out_len", u32, X.n)
    A.ready()
    with Engine(segments=1) as e:
        e.umi_reads(X.text, X.start, d_off, info, mate, X.n, out, out_off, out_len)
        e.sync()
    return dict(out=out, out_off=out_off, out_len=out_len, _nontrivial=lambda o: not (o["out"] == POISON).any() and int(o["out_off"].view(u64)[-1]) + int(o["out_len"].view(u32)[-1]) == total)


def case_umi_merge(A):
    R = resident_run()
    umi_off, info = plain_umi_find()
    X = Resident(A, ["start"])
    ins = [A.inp("umi_off", umi_off), A.inp("owner_exact", R["owner_exact"]), A.inp("owner_seq", R["owner"]), A.inp("size", R["esize"])]
    owner_out = A.out("owner_out", u32, X.n)
    A.ready()
    with Engine(segments=1) as e:
        got = e.umi_merge(X.text, X.start, ins[0], info, ins[1], ins[2], ins[3], X.n, 1, owner_out)
    return dict(owner_out=owner_out, info=[got.nodes, got.groups, got.merged, got.largest, got.sweeps, got.over_limit_nodes, got.over_limit_first],
                _nontrivial=lambda o: o["info"][2] > 0 and o["info"][0] > o["info"][1] > 0 and not np.array_equal(o["owner_out"].view(u32), R["owner_exact"]))


def case_read_places(A):
    X = Resident(A, ["start", "id_len"])
    outs = [A.out(w, u32, X.n) for w in ("tile", "x", "y", "surface")]
    A.ready()
    with Engine(segments=1) as e:
        info = e.read_places(X.text, X.start, X.id_len, X.n, *outs)
    return dict(tile=outs[0], x=outs[1], y=outs[2], surface=outs[3], info=[info.bad_record, info.bad_reason, info.other_surface],
                _nontrivial=lambda o: o["info"][0] == _lib.UMI_NO_RECORD and o["info"][2] > 0 and len(np.unique(o["x"])) > 50 and len(np.unique(o["tile"])) == 3)


def case_optical_split(A):
    R = resident_run()
    X = Resident(A, ["start", "perm", "head"])
    places = [A.inp(w, a) for w, a in zip(("tile", "x", "y", "surface"), plain_places())]
    owner_out = A.out("owner_out", u32, X.n)
    A.ready()
    with Engine(segments=1) as e:
        got = e.optical_split(X.perm, X.head, X.text, X.start, *places, X.n, 20, owner_out)
    return dict(owner_out=owner_out, info=[got.clusters_in, got.clusters_out, got.split, got.largest, got.sweeps, got.over_limit_members, got.over_limit_first],
                _nontrivial=lambda o: o["info"][2] > 0 and o["info"][1] > o["info"][0] and o["info"][3] == 65 and not np.array_equal(o["owner_out"].view(u32), R["owner"]))


def near_info(got):
    return [got.nodes, got.merged, got.entries, got.groups, got.pairs, got.edges, got.largest_group, got.sweeps, got.over_limit_first, got.over_limit_nodes]


def case_near_merge(A, with_umi, flags, with_link=False):
    R = resident_run()
    X = Resident(A, ["start"])
    segs = [Reads(X.text, offsets=A.inp("seq_off", R["seq_off"] + u64(X.T.bias)), lengths=A.inp("seq_len", R["seq_len"]))]
    owner_h = R["owner_exact"] if with_umi else R["owner"]
    owner, owner_out = A.inp("owner", owner_h), A.out("owner_out", u32, X.n)
    if with_umi:
        umi_off, info = plain_umi_find()
        d_off = A.inp("umi_off", umi_off)
        # a link as fqd_umi_merge leaves it: at a node, the earlier node it was merged into — here the first record of the node's sequence
        link = A.inp("link", R["owner"]) if with_link else None
    A.ready()
    with Engine(segments=1) as e:
        if with_umi:
            got = e.near_merge_umi(segs, owner, link, X.n, 1, X.text, X.start, d_off, info, owner_out, flags)
            said = near_info(got.near) + [got.links]
        else:
            said = near_info(e.near_merge(segs, owner, X.n, 1, owner_out, flags))
    return dict(owner_out=owner_out, info=said, _nontrivial=lambda o: o["info"][0] - o["info"][1] > 0 and o["info"][5] > 0
                and not np.array_equal(o["owner_out"].view(u32), owner_h) and (not with_link or o["info"][-1] > 0))


def second_file(A, X, whole=False):
    """Mate 2 of record i = record n - 1 - i of a second copy of the text: (bytes, offsets, lengths, n), sequences or whole records."""
    R = X.R
    T2 = A.text("text2", R["text"])
    off, ln = (R["start"], R["size"]) if whole else (R["seq_off"], R["seq_len"])
    return (T2.base, A.inp("off2", off[::-1] + u64(T2.bias)), A.inp("len2", ln[::-1]), X.n)


def pair_order(R, paired):
    seqs, n = R["seqs"], R["n"]
    return np.array(sorted(range(n), key=lambda i: (seqs[i] + b"\n", seqs[n - 1 - i] + b"\n" if paired else b"", i)), u32)


def whole_records(A, X):
    R = X.R
    return (X.text, X.start, A.inp("rec_len", R["size"]), X.n)


def case_seq_scores(A, paired):
    X = Resident(A, ["start"])
    rec = whole_records(A, X)
    rec2 = second_file(A, X, whole=True) if paired else None
    score = A.out("score", u32, X.n)
    A.ready()
    with Engine(segments=1) as e:
        e.seq_scores(rec, score, rec2)
    return dict(score=score, _nontrivial=lambda o: len(np.unique(o["score"])) > 100)


def case_seq_pick_best(A):
    R = resident_run()
    n = R["n"]
    rng = np.random.default_rng(4)
    score, head, perm = A.inp("score", rng.integers(0, 50, n).astype(u32)), A.inp("head", R["head"]), A.inout("perm", R["perm"])
    A.ready()
    with Engine(segments=1) as e:
        moved = e.seq_pick_best(score, head, n, perm)
    return dict(perm=perm, moved=moved, _nontrivial=lambda o: o["moved"] > 5 and not np.array_equal(o["perm"].view(u32), R["perm"]))


def case_consensus(A, flags):
    """The text is inout: every byte that is no sequence or quality byte of a written record of a cluster of two or more must come
    back as it was."""
    R = resident_run()
    X = Resident(A, ["start", "size", "seq_off", "seq_len", "perm", "head"], role="inout")
    changed = A.inout("changed", np.zeros(X.n, u8))
    A.ready()
    with Engine(segments=1) as e:
        info = e.consensus(X.perm, X.head, X.n, X.text, X.start, X.size, X.seq_off, X.seq_len, flags, changed)
    may_change = np.zeros(len(R["text"]), bool)
    for r in R["perm"][(R["head"] == 1) & (R["csize"][R["perm"]] > 1)]:
        s, q, L = int(R["seq_off"][r]), int(R["start"][r]) + int(R["size"][r]) - 1 - int(R["seq_len"][r]), int(R["seq_len"][r])
        may_change[s:s + L] = True
        may_change[q:q + L] = True
    return dict(text=X.T.view, changed=changed, info=[info.clusters, info.members, info.bases_changed, info.reads_changed, info.largest],
                outside=lambda: bool(np.array_equal(X.T.view.cpu().numpy()[~may_change], R["text"][~may_change])),
                _nontrivial=lambda o: o["outside"] and o["info"][0] > 30 and o["info"][4] == 65 and int((o["text"] != R["text"]).sum()) > 1000)


def seq_spans(A, X, tag="seq"):
    R = X.R
    return (X.text, A.inp(tag + "_off", R["seq_off"] + u64(X.T.bias)), A.inp(tag + "_len", R["seq_len"]), X.n)


def case_sort_seqs(A, paired):
    X = Resident(A, [])
    spans, perm = seq_spans(A, X), A.out("perm", u32, X.n)
    mate2 = second_file(A, X) if paired else None
    A.ready()
    with Engine(segments=1) as e:
        e.sort_seqs(spans, perm, mate2)
    want = pair_order(X.R, paired)
    return dict(perm=perm, _nontrivial=lambda o: np.array_equal(o["perm"].view(u32), want))


def case_seq_heads(A, mode, paired):
    X = Resident(A, [])
    spans = seq_spans(A, X)
    mate2 = second_file(A, X) if paired else None
    perm, head = A.inp("perm", pair_order(X.R, paired)), A.out("head", u8, X.n)
    A.ready()
    with Engine(segments=1) as e:
        heads = e.seq_heads(spans, perm, mode, 2, head, mate2)
    return dict(head=head, heads=heads, _nontrivial=lambda o: 1 < o["heads"] < X.n + paired and int(o["head"].sum()) == o["heads"])


def case_seq_prefix_keys(A, paired):
    X = Resident(A, [])
    spans = seq_spans(A, X)
    size1 = A.inp("size1", X.R["size"])
    mate2 = second_file(A, X) if paired else None
    size2 = A.inp("size2", X.R["size"][::-1]) if paired else None
    key, nbytes = A.out("key", u64, X.n), A.out("bytes", u32, X.n)
    A.ready()
    with Engine(segments=1) as e:
        info = e.seq_prefix_keys(spans, key=key, mate2=mate2, size1=size1, size2=size2, bytes_=nbytes)
    return dict(key=key, bytes=nbytes, info=[info.longest[0], info.longest[1], info.bad_byte, info.record_bytes] + list(info.first_with),
                _nontrivial=lambda o: o["info"][:3] == [151, 151 if paired else 0, -1] and o["info"][3] == (2 if paired else 1) * int(X.R["size"].sum())
                and len(np.unique(o["key"])) > 50)


def case_seq_plan_ranges(A):
    runs = []
    for n in COUNTS:
        rng = np.random.default_rng(n)
        runs.append((n, A.inp(f"n{n}.key", rng.integers(0, 40, n).astype(u64) << u64(56)), A.inp(f"n{n}.bytes", rng.integers(100, 700, n).astype(u32)),
                     A.inp(f"n{n}.bytes_mate1", rng.integers(0, 100, n).astype(u32)), A.out(f"n{n}.range_of", u32, n)))
    A.ready()
    plans = []
    with Engine(segments=1) as e:
        for n, key, nbytes, m1, range_of in runs:
            plans.append(list(e.seq_plan_ranges(key, nbytes, n, 5000, range_of, bytes_mate1=m1)))
    out = {f"range_of{k}": r[4] for k, r in enumerate(runs)}
    out["plans"] = plans
    out["_nontrivial"] = lambda o: o["plans"][7][0] > 10 and len(np.unique(o["range_of7"])) == o["plans"][7][0]
    return out


def case_synth_reads(A):
    runs = [(n, L, A.out(f"n{n}L{L}.bases", u8, n * L), A.out(f"n{n}L{L}.expect_keep", u8, n)) for n, L in SHAPES]
    A.ready()
    with Engine(segments=1) as e:
        for n, L, bases, expect in runs:
            e.synth_reads(5, 0, n, L, 300, 0, bases, expect)
        e.sync()
    out = {f"bases{k}": r[2] for k, r in enumerate(runs)}
    out.update({f"expect{k}": r[3] for k, r in enumerate(runs)})
    out["_nontrivial"] = lambda o: 0 < int(o["expect7"].sum()) < 1025 and set(np.unique(o["bases7"]).tolist()) <= set(b"ACGTN")
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, entry, variant, fn, far=False, env=None):
        self.entries = (entry,) if isinstance(entry, str) else entry
        self.id = "+".join(self.entries) + (f"[{variant}]" if variant else "")
        self.fn, self.far, self.env = fn, far, env or {}


def table():
    T = []
    bind = lambda f, *a: (lambda A: f(A, *a))
    for bulk in ("0", "-1"):                                          # FQD_BULK_MIN: the bulk and the atomic insert path
        env = {"FQD_BULK_MIN": bulk}
        for kind, entry in (("submit", "fqd_submit"), ("final", "fqd_submit_final"), ("linked", "fqd_submit_linked")):
            for S in (1, 2):
                for layout in ("uniform", "noslack", "ragged", "nostage"):
                    T.append(Case(entry, f"{'se' if S == 1 else 'pe'}-{layout}-bulk_min{bulk}", bind(case_submit, kind, S, layout), far=layout == "ragged", env=env))
        for how in ("keys", "slabs", "slabs_hashed"):
            T.append(Case("fqd_insert_" + how, f"bulk_min{bulk}", bind(case_insert, how), env=env))
        T.append(Case("fqd_widen_keys", f"bulk_min{bulk}", case_widen_keys, far=True, env=env))
    for S in (1, 2):
        for no_stage in (False, True):
            for layout in ("uniform", "noslack"):
                T.append(Case("fqd_encode_uniform", f"{'se' if S == 1 else 'pe'}-{layout}{'-nostage' if no_stage else ''}", bind(case_encode_uniform, S, no_stage, layout)))
        for layout in ("ragged", "uniform", "nostage"):
            T.append(Case("fqd_encode_padded", f"{'se' if S == 1 else 'pe'}-{layout}", bind(case_encode_padded, S, layout), far=layout != "uniform"))
    for parts in (1, 3, 16):
        T.append(Case("fqd_partition_keys", f"parts{parts}", bind(case_partition_keys, parts)))
        for room in ("fits", "spills_a_little", "spills_nearly_all"):
            T.append(Case("fqd_partition_slabs", f"parts{parts}-{room}", bind(case_partition_slabs, parts, room)))
        for hashed in (False, True):
            for exact in (False, True):
                for room in ("fits", "full_sub_slabs"):
                    T.append(Case("fqd_encode_slabs_hashed" if hashed else "fqd_encode_slabs", f"parts{parts}-{'exact' if exact else 'one_pass'}-{room}",
                                  bind(case_encode_slabs, hashed, parts, exact, room)))
    T.append(Case("fqd_scatter_flags", "", case_scatter_flags))
    # linked-mode stages
    T += [Case("fqd_owners", "", case_owners), Case("fqd_group_owners", "", case_group_owners), Case("fqd_heads_to_keep", "", case_heads_to_keep),
          Case("fqd_owners_to_keep", "", case_owners_to_keep), Case("fqd_cluster_sizes", "", bind(case_cluster_sizes, False)),
          Case("fqd_cluster_weights", "", bind(case_cluster_sizes, True)), Case("fqd_size_labels", "", case_size_labels, far=True),
          Case("fqd_size_filter", "", case_size_filter), Case("fqd_size_order", "", bind(case_size_order, False)),
          Case("fqd_size_order_ex", "", bind(case_size_order, True)), Case("fqd_take_u32", "", case_take_u32),
          Case("fqd_size_annotations", "file1", bind(case_size_annotations, False), far=True),
          Case("fqd_size_annotations", "file2_with_expect", bind(case_size_annotations, True), far=True), Case("fqd_size_relabel", "", case_size_relabel),
          Case("fqd_umi_find", "", case_umi_find, far=True), Case("fqd_umi_merge", "", case_umi_merge, far=True),
          Case("fqd_read_places", "", case_read_places, far=True), Case("fqd_optical_split", "", case_optical_split, far=True),
          Case("fqd_seq_pick_best", "", case_seq_pick_best), Case("fqd_seq_plan_ranges", "", case_seq_plan_ranges)]
    for paired, ends in ((False, "se"), (True, "pe")):                 # pe: mate2 / rec2 / size2 are given, in a text of their own
        T += [Case("fqd_seq_scores", ends, bind(case_seq_scores, paired), far=True), Case("fqd_sort_seqs", ends, bind(case_sort_seqs, paired), far=True),
              Case("fqd_seq_prefix_keys", ends, bind(case_seq_prefix_keys, paired), far=True)]
        for mode, name in ((_lib.SEQ_TIGHT, "tight"), (_lib.SEQ_LOOSE, "loose"), (_lib.SEQ_HAMMING, "hamming")):
            T.append(Case("fqd_seq_heads", f"{ends}-{name}", bind(case_seq_heads, mode, paired), far=True))
    for layout in ("ragged", "uniform"):
        T.append(Case("fqd_umi_reads", layout, bind(case_umi_reads, layout), far=True))
        for S in (1, 2):
            T.append(Case("fqd_canonical_reads", f"{'se' if S == 1 else 'pe'}-{layout}", bind(case_canonical_reads, S, layout), far=layout == "ragged"))
    for flags, name in ((0, "seeds"), (_lib.NEAR_WEAK_SEEDS, "weak_seeds")):
        T.append(Case("fqd_near_merge", name, bind(case_near_merge, False, flags), far=True))
        T.append(Case("fqd_near_merge_umi", name, bind(case_near_merge, True, flags), far=True))
        T.append(Case("fqd_near_merge_umi", name + "-with_link", bind(case_near_merge, True, flags, True), far=True))
    for flags, name in ((0, "tiers"), (_lib.CONSENSUS_SMALL_TIERS, "small_tiers")):
        T.append(Case("fqd_consensus", name, bind(case_consensus, flags), far=True))
    # records, join and output
    T += [Case("fqd_count_lines", "", case_count_lines, far=True), Case("fqd_scan_records", "", case_scan_records, far=True),
          Case("fqd_extract_tags", "", case_extract_tags, far=True), Case("fqd_sort_tags", "", case_sort_tags, far=True),
          Case("fqd_join_tags", "", case_join_tags, far=True), Case("fqd_gather_seqs", "", case_gather_seqs), Case("fqd_copy_spans", "", case_copy_spans, far=True),
          Case("fqd_copy_labelled", "", bind(case_copy_labelled, False), far=True), Case("fqd_copy_relabelled", "", bind(case_copy_labelled, True), far=True),
          Case("fqd_output_offsets", "", bind(case_output_plan, True)), Case("fqd_output_plan", "", bind(case_output_plan, False)),
          Case("fqd_count_tags_le", "", case_count_tags_le, far=True), Case("fqd_sample_tags", "", case_sample_tags, far=True),
          Case("fqd_classify_tags", "", case_classify_tags, far=True), Case("fqd_range_keep", "", case_range_keep), Case("fqd_max_u32", "", case_max_u32)]
    # codecs
    small_units = {"FQD_GUNZIP_UNIT_KB": "8"}                          # several units in a stream of 200 KB
    T += [Case(("fqd_bgzf_deflate", "fqd_bgzf_deflate_ex"), "fast", bind(case_bgzf_deflate, "fast")), Case("fqd_bgzf_deflate_ex", "search", bind(case_bgzf_deflate, "high")),
          Case("fqd_bgzf_inflate", "", bind(case_bgzf_inflate, False), far=True), Case("fqd_bgzf_inflate_async", "", bind(case_bgzf_inflate, True), far=True),
          Case("fqd_gunzip", "exact_room", bind(case_gunzip, 0), far=True, env=small_units),
          Case("fqd_gunzip", "one_byte_short", bind(case_gunzip, -1), far=True, env=small_units),
          Case("fqd_gunzip_arriving", "exact_room", bind(case_gunzip, 0, True), far=True, env=small_units),
          Case("fqd_synth_reads", "", case_synth_reads)]
    return T


TABLE = table()
# hipErrorIllegalAddress, hipErrorLaunchFailure, hipErrorIllegalInstruction, hipErrorMisalignedAddress as hipGetErrorString words them
# (FqdError carries that text): the context is gone after these.  An allocation that fails, or a bad argument, is none of them.
GPU_FAULT_WORDS = ("illegal memory access", "illegal address", "unspecified launch failure", "launch failure", "illegal instruction", "misaligned address")


@pytest.mark.parametrize("case", TABLE, ids=[c.id for c in TABLE])
def test_buffers_are_respected_wherever_they_lie(case, monkeypatch, far_holder):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    modes = ["plain", "ff", "nl"] + (["far"] if case.far else [])
    results = {}
    for mode in modes:
        try:
            results[mode], nontrivial = run_case(case.fn, mode, far_holder)
        except Exception as ex:                                        # after a GPU FAULT nothing more is started on the card; any other error is this test's alone
            if any(word in str(ex).lower() for word in GPU_FAULT_WORDS):
                pytest.exit(f"{case.id}, {mode} run: {ex}", returncode=3)
            raise
    plain = results["plain"]
    assert nontrivial(plain), f"{case.id}: the plain run's outputs are trivial or not what the inputs were built to give"
    for mode in modes[1:]:
        got = results[mode]
        assert got.keys() == plain.keys()
        for k in plain:
            assert same(plain[k], got[k]), f"{case.id}: '{k}' of the {mode} run differs from the plain run's: {first_difference(plain[k], got[k])}"


def test_scan_records_writes_offsets_beyond_2_to_the_32(far_holder):
    """fqd_count_lines and fqd_scan_records take a text and its length, no offsets: the offsets they WRITE pass 2^32 only in a text
    of more than 4 GiB.  The far arena's own memory holds it: 4.3 M records of 1007 bytes (an odd size: every alignment), each
    array against its arithmetic."""
    far = far_holder.get()
    far.reset()
    L = 500
    record = b"@r\n" + b"ACGT" * (L // 4) + b"\n+\n" + b"I" * L + b"\n"
    size = len(record)
    n_rec = ((1 << 32) + (64 << 20)) // size
    n = n_rec * size
    assert size == 1007 and (1 << 32) < n < far.nbytes
    try:
        far.mem[:n].view(n_rec, size).copy_(torch.frombuffer(bytearray(record), dtype=torch.uint8).cuda())
        i64, i32 = dict(dtype=torch.int64, device="cuda"), dict(dtype=torch.int32, device="cuda")
        start, seq_off = torch.full((n_rec,), -1, **i64), torch.full((n_rec,), -1, **i64)
        id_len, seq_len, sizes = torch.full((n_rec,), -1, **i32), torch.full((n_rec,), -1, **i32), torch.full((n_rec,), -1, **i32)
        torch.cuda.synchronize()
        with Engine(segments=1) as e:
            assert e.count_lines(far.mem, n) == 4 * n_rec
            assert e.scan_records(far.mem, n, 4, n_rec, start, seq_off, id_len, seq_len, sizes)
        want = torch.arange(n_rec, **i64) * size
        assert int(want[-1]) > 1 << 32
        assert torch.equal(start, want) and torch.equal(seq_off, want + 3)
        assert bool((id_len == 3).all()) and bool((seq_len == L).all()) and bool((sizes == size).all())
    finally:
        far.mem[:n] = far.fill                                         # the arena's pattern again, for the cases behind this test
        torch.cuda.synchronize()


# What the table leaves out, and why: no caller's device buffer is read or written by these.
NOT_IN_THE_TABLE = {
    # lifecycle, errors, stats and profiles: host structs only
    "fqd_abi_version", "fqd_device_count", "fqd_engine_create", "fqd_engine_destroy", "fqd_engine_reset", "fqd_engine_sync", "fqd_bad_base",
    "fqd_get_stats", "fqd_get_profile", "fqd_reset_profile", "fqd_last_error",
    # streams and ordering
    "fqd_engine_stream", "fqd_engine_wait_stream", "fqd_stream_wait_engine",
    # pure arithmetic
    "fqd_key_words", "fqd_padded_key_words", "fqd_bgzf_bound", "fqd_shard_slab_capacity",
    # gives out a place in the engine's own store (the insert cases write there)
    "fqd_reserve_keys",
    # the shard group: its buffers are the group's own; the building blocks above carry its kernels
    "fqd_shard_unique_id", "fqd_shard_create", "fqd_shard_destroy", "fqd_shard_round", "fqd_shard_flush", "fqd_shard_wait", "fqd_shard_bad_base",
    "fqd_shard_get_stats", "fqd_shard_last_error",
}


def test_every_entry_point_with_a_device_buffer_is_in_the_table():
    declared = set(declared_symbols())
    covered = {name for c in TABLE for name in c.entries}
    assert covered <= declared, covered - declared
    assert not covered & NOT_IN_THE_TABLE
    missing = declared - covered - NOT_IN_THE_TABLE
    assert not missing, f"exported, takes a caller's device buffer, and runs in no case of this file: {sorted(missing)}"
    assert NOT_IN_THE_TABLE <= declared, NOT_IN_THE_TABLE - declared
