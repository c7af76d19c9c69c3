"""ctypes wrapper over the C ABI (include/fqdupaway.h).  Plumbing only: all work
happens in lib/libfqdupaway.so on the GPU; nothing here computes a result."""
import ctypes as C
from dataclasses import dataclass
from typing import Any, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import FqdError, load_library


@dataclass
class Reads:
    """One mate's sequences for a batch (mirrors struct fqd_reads).

    bases/offsets/lengths are numpy arrays (host space), torch CUDA tensors or raw
    device pointers as int (device space).  Leave offsets and lengths None for a
    uniform batch: read i = uniform_len bytes at bases + i*uniform_stride."""
    bases: Any
    offsets: Any = None
    lengths: Any = None
    uniform_len: int = 0
    uniform_stride: int = 0


def _is_host(x) -> bool:
    return isinstance(x, np.ndarray)


def _addr(x) -> Optional[int]:
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if isinstance(x, int):
        return x
    return x.data_ptr()          # torch tensor


def _torch_stream(x) -> int:
    """hipStream_t (as an integer) of torch's current stream on the tensor's device."""
    import torch
    return int(torch.cuda.current_stream(x.device).cuda_stream)


class Engine:
    """One HBM-resident exact sequence set on one MI355X (struct fqd_engine)."""

    def __init__(self, segments: int = 1, device: int = 0, capacity_reads: int = 0, capacity_bases: int = 0,
                 stream: Optional[int] = None, profile: bool = False, no_stage: bool = False, weak_hash: bool = False):
        self._L = load_library()
        cfg = _lib.Config(device=device, segments=segments, capacity_reads=capacity_reads,
                          capacity_bases=capacity_bases, stream=stream,
                          flags=(_lib.FLAG_PROFILE if profile else 0) | (_lib.FLAG_NO_STAGE if no_stage else 0)
                          | (_lib.FLAG_WEAK_HASH if weak_hash else 0))
        h = C.c_void_p()
        rc = self._L.fqd_engine_create(C.byref(cfg), C.byref(h))
        if rc != _lib.OK:
            raise FqdError(rc, (self._L.fqd_last_error(None) or b"").decode())
        self._h = h
        self._ordered = False
        self.segments = segments

    # -- lifecycle ----------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.fqd_engine_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- ordering against the caller's stream ------------------------------------------
    # The engine runs on its own non-blocking stream and waits for nobody (include/fqdupaway.h, ORDERING RULE): whatever
    # torch queued for a tensor on ITS stream (zeros, fill_, copy_) must be ordered before the engine's work explicitly.
    # The first torch tensor among a call's arguments makes the engine wait for torch's current stream; arguments are
    # evaluated before the C function runs, so the wait is queued ahead of the call's kernels.
    def _p(self, x) -> Optional[int]:
        if x is None:
            return None
        if isinstance(x, np.ndarray):
            return x.ctypes.data
        if isinstance(x, int):
            return x
        if not self._ordered:
            self._ordered = True
            rc = self._L.fqd_engine_wait_stream(self._h, _torch_stream(x))
            if rc != _lib.OK:
                self._ordered = False
                raise FqdError(rc, (self._L.fqd_last_error(self._h) or b"").decode())
        return x.data_ptr()

    def _desc(self, segs: Sequence[Reads]):
        arr = (_lib.ReadsDesc * 2)()
        for k, s in enumerate(segs):
            arr[k].bases = self._p(s.bases)
            arr[k].offsets = self._p(s.offsets)
            arr[k].lengths = self._p(s.lengths)
            arr[k].uniform_len = s.uniform_len
            arr[k].uniform_stride = s.uniform_stride
        return arr

    def wait_stream(self, stream: Optional[int] = None):
        """The engine starts after everything queued so far on `stream` (default: torch's current stream)."""
        if stream is None:
            import torch
            stream = int(torch.cuda.current_stream().cuda_stream)
        self._check(self._L.fqd_engine_wait_stream(self._h, stream))

    def release_to(self, stream: Optional[int] = None):
        """`stream` (default: torch's current stream) continues after everything the engine has queued so far."""
        if stream is None:
            import torch
            stream = int(torch.cuda.current_stream().cuda_stream)
        self._check(self._L.fqd_stream_wait_engine(self._h, stream))

    def _check(self, rc: int):
        self._ordered = False
        if rc != _lib.OK:
            raise FqdError(rc, (self._L.fqd_last_error(self._h) or b"").decode())

    def reset(self):
        self._check(self._L.fqd_engine_reset(self._h))

    def sync(self):
        self._check(self._L.fqd_engine_sync(self._h))

    def stream_handle(self) -> int:
        """The engine's hipStream_t as an integer (wrap with torch.cuda.ExternalStream)."""
        return int(self._L.fqd_engine_stream(self._h) or 0)

    # -- the hot path ---------------------------------------------------------------
    def submit(self, segs: Sequence[Reads], n: int, keep=None, final: bool = False):
        """Dedups n more records; returns their keep flags (numpy for host input,
        the given device buffer otherwise).  final: this is the run's last batch (fqd_submit_final)."""
        if len(segs) != self.segments:
            raise ValueError(f"engine has {self.segments} mate(s) per record, got {len(segs)}")
        host = _is_host(segs[0].bases)
        for s in segs:
            if _is_host(s.bases) != host:
                raise ValueError("all mates must live in the same memory space")
            if _is_host(s.bases):
                for a, dt in ((s.bases, np.uint8), (s.offsets, np.uint64), (s.lengths, np.uint32)):
                    if a is not None and (a.dtype != dt or not a.flags["C_CONTIGUOUS"]):
                        raise ValueError(f"host arrays must be C-contiguous {dt}")
        if host:
            keep = np.empty(n, dtype=np.uint8) if keep is None else keep
        elif keep is None:
            raise ValueError("device submits need a device keep buffer")
        fn = self._L.fqd_submit_final if final else self._L.fqd_submit
        rc = fn(self._h, self._desc(segs), n, _lib.MEM_HOST if host else _lib.MEM_DEVICE, self._p(keep))
        self._check(rc)
        return keep

    def bad_base(self):
        rec, seg, pos, byte = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint8()
        self._check(self._L.fqd_bad_base(self._h, C.byref(rec), C.byref(seg), C.byref(pos), C.byref(byte)))
        return rec.value, seg.value, pos.value, byte.value

    def stats(self):
        st = _lib.Stats()
        self._check(self._L.fqd_get_stats(self._h, C.byref(st)))
        return {"records": st.records, "duplicates": st.duplicates, "table_slots": st.table_slots, "key_bytes": st.key_bytes}

    def profile(self):
        p = _lib.Profile()
        self._check(self._L.fqd_get_profile(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in _lib.Profile._fields_}

    def reset_profile(self):
        self._check(self._L.fqd_reset_profile(self._h))

    # -- sharding halves ---------------------------------------------------------------
    def key_words(self, len0: int, len1: int = 0) -> int:
        return int(self._L.fqd_key_words(len0, len1))

    def encode_uniform(self, segs: Sequence[Reads], n: int, records):
        self._check(self._L.fqd_encode_uniform(self._h, self._desc(segs), n, self._p(records)))

    def partition_keys(self, records, n: int, key_words: int, n_parts: int, out_keys, counts, origin):
        self._check(self._L.fqd_partition_keys(self._h, self._p(records), n, key_words, n_parts,
                                               self._p(out_keys), self._p(counts), self._p(origin)))

    def reserve_keys(self, n: int, len0: int, len1: int) -> int:
        """Device address of room for n keys at the tail of the key store (receive in place)."""
        slot = C.c_void_p()
        self._check(self._L.fqd_reserve_keys(self._h, n, len0, len1, C.byref(slot)))
        return slot.value

    def insert_keys(self, keys, n: int, len0: int, len1: int, keep):
        self._check(self._L.fqd_insert_keys(self._h, self._p(keys), n, len0, len1, self._p(keep)))

    def padded_key_words(self, max_len0: int, max_len1: int = 0) -> int:
        return int(self._L.fqd_padded_key_words(max_len0, max_len1))

    def encode_padded(self, segs: Sequence[Reads], n: int, max_len0: int, max_len1: int, records):
        self._check(self._L.fqd_encode_padded(self._h, self._desc(segs), n, max_len0, max_len1, self._p(records)))

    def widen_keys(self, new_words: int):
        self._check(self._L.fqd_widen_keys(self._h, new_words))

    def partition_slabs(self, records, n: int, key_words: int, n_parts: int, slab_cap: int, out_keys, counts, origin):
        self._check(self._L.fqd_partition_slabs(self._h, self._p(records), n, key_words, n_parts, slab_cap,
                                                self._p(out_keys), self._p(counts), self._p(origin)))

    def encode_slabs(self, segs: Sequence[Reads], n: int, n_parts: int, chunk_reads: int, n_chunks: int, sub_cap: int, out_keys,
                     chunk_counts, totals, origin, exact: bool = False):
        self._check(self._L.fqd_encode_slabs(self._h, self._desc(segs), n, n_parts, chunk_reads, n_chunks, sub_cap, self._p(out_keys),
                                             self._p(chunk_counts), self._p(totals), self._p(origin), 1 if exact else 0))

    def encode_slabs_hashed(self, segs: Sequence[Reads], n: int, n_parts: int, chunk_reads: int, n_chunks: int, sub_cap: int, out_keys, out_hashes,
                            chunk_counts, totals, origin, exact: bool = False):
        self._check(self._L.fqd_encode_slabs_hashed(self._h, self._desc(segs), n, n_parts, chunk_reads, n_chunks, sub_cap, self._p(out_keys), self._p(out_hashes),
                                                    self._p(chunk_counts), self._p(totals), self._p(origin), 1 if exact else 0))

    def insert_slabs_hashed(self, keys, hashes, n_slabs: int, slab_cap: int, slab_count, len0: int, len1: int, keep):
        self._check(self._L.fqd_insert_slabs_hashed(self._h, self._p(keys), self._p(hashes), n_slabs, slab_cap, self._p(slab_count), len0, len1, self._p(keep)))

    def insert_slabs(self, keys, n_slabs: int, slab_cap: int, slab_count, len0: int, len1: int, keep):
        self._check(self._L.fqd_insert_slabs(self._h, self._p(keys), n_slabs, slab_cap, self._p(slab_count), len0, len1, self._p(keep)))

    # -- --unordered ID join ---------------------------------------------------------------
    def _tags(self, bytes_, offsets, lengths, n):
        return _lib.TagsDesc(bytes=self._p(bytes_), offsets=self._p(offsets), lengths=self._p(lengths), n=n)

    def sort_tags(self, bytes_, offsets, lengths, n: int, perm):
        t = self._tags(bytes_, offsets, lengths, n)
        self._check(self._L.fqd_sort_tags(self._h, C.byref(t), self._p(perm)))

    # -- sequence-based modes (--compare-seq) -----------------------------------------------
    def sort_seqs(self, mate1, perm, mate2=None):
        """mate1 / mate2 = (bytes, offsets, lengths, n) of the sequences without '\\n'; perm (n uint32) = sorted order."""
        t1 = self._tags(*mate1)
        t2 = self._tags(*mate2) if mate2 is not None else None
        self._check(self._L.fqd_sort_seqs(self._h, C.byref(t1), C.byref(t2) if t2 is not None else None, self._p(perm)))

    def seq_heads(self, mate1, perm, mode: int, distance: int, head, mate2=None) -> int:
        """head[k] = 1 iff sorted record k is written (mode: SEQ_TIGHT / SEQ_LOOSE / SEQ_HAMMING); returns the number of heads."""
        t1 = self._tags(*mate1)
        t2 = self._tags(*mate2) if mate2 is not None else None
        heads = C.c_uint64(0)
        self._check(self._L.fqd_seq_heads(self._h, C.byref(t1), C.byref(t2) if t2 is not None else None, self._p(perm), mode, distance,
                                          self._p(head), C.byref(heads)))
        return int(heads.value)

    def seq_prefix_keys(self, mate1, key=None, mate2=None, size1=None, size2=None, bytes_=None, accumulate: bool = False):
        """The ranged run's pass over an uploaded block: key[i] (uint64) = the first 8 sequence bytes of mate 1, big-endian,
        padded with '\\n'; bytes_[i] = size1[i] + size2[i].  Returns the block's fqd_seq_block_info (_lib.SeqBlockInfo)."""
        t1 = self._tags(*mate1)
        t2 = self._tags(*mate2) if mate2 is not None else None
        info = _lib.SeqBlockInfo()
        self._check(self._L.fqd_seq_prefix_keys(self._h, C.byref(t1), C.byref(t2) if t2 is not None else None, self._p(size1), self._p(size2),
                                                int(accumulate), self._p(key), self._p(bytes_), C.byref(info)))
        return info

    def seq_plan_ranges(self, key, bytes_, n: int, target_bytes: int, range_of, max_ranges: int = 4096, bytes_mate1=None):
        """The exact plan of the ranges; returns (number of ranges, rows (key_lo, key_hi, pairs, bytes) of the first max_ranges),
        and with bytes_mate1 a third value: mate 1's bytes of every such row."""
        table = (_lib.SeqRange * max(max_ranges, 1))()
        R = C.c_uint32(0)
        self._check(self._L.fqd_seq_plan_ranges(self._h, self._p(key), self._p(bytes_), self._p(bytes_mate1), n, target_bytes, self._p(range_of),
                                                table, max_ranges, C.byref(R)))
        got = table[:min(R.value, max_ranges)]
        rows = [(t.key_lo, t.key_hi, t.pairs, t.bytes) for t in got]
        if bytes_mate1 is None:
            return int(R.value), rows
        return int(R.value), rows, [t.bytes_mate1 for t in got]

    def seq_scores(self, rec1, score, rec2=None):
        """FQD_SEQ_KEEP=best: rec1 / rec2 = (bytes, offsets, lengths, n) of the WHOLE records (length with the final '\\n');
        score[i] (n uint32, input order) = the sum of the quality bytes above '!' of record (pair) i, saturating."""
        t1 = self._tags(*rec1)
        t2 = self._tags(*rec2) if rec2 is not None else None
        self._check(self._L.fqd_seq_scores(self._h, C.byref(t1), C.byref(t2) if t2 is not None else None, self._p(score)))

    def seq_pick_best(self, score, head, n: int, perm) -> int:
        """Per cluster of head (fqd_seq_heads) the member with the highest score, the earliest on a tie, takes the head's
        place in perm (a swap); returns the number of clusters whose written member changed."""
        moved = C.c_uint64(0)
        self._check(self._L.fqd_seq_pick_best(self._h, self._p(score), self._p(head), n, self._p(perm), C.byref(moved)))
        return int(moved.value)

    # -- FQD_FAST_KEEP / FQD_FAST_CLUSTERS (csrc/fqd_owner.hip) -----------------------------------
    def submit_linked(self, segs: Sequence[Reads], n: int, keep, link, last: bool = False, memory: Optional[int] = None):
        """submit (last: submit_final) of device input that also fills link[i] (n uint32) with the engine index of an
        earlier record of the same key for every cleared flag.  memory: the fqd_mem value handed on (default: device)."""
        if len(segs) != self.segments:
            raise ValueError(f"engine has {self.segments} mate(s) per record, got {len(segs)}")
        self._check(self._L.fqd_submit_linked(self._h, self._desc(segs), n, _lib.MEM_DEVICE if memory is None else memory,
                                              self._p(keep), self._p(link), int(last)))
        return keep

    def owners(self, keep, link, n: int, owner):
        """owner[i] (n uint32) = the first record with record i's key, over all n records submitted so far."""
        self._check(self._L.fqd_owners(self._h, self._p(keep), self._p(link), n, self._p(owner)))

    def group_owners(self, owner, n: int, perm, head) -> int:
        """perm = the records ordered by owner (members in input order), head = 1 at every run's first place; returns the runs."""
        clusters = C.c_uint64(0)
        self._check(self._L.fqd_group_owners(self._h, self._p(owner), n, self._p(perm), self._p(head), C.byref(clusters)))
        return int(clusters.value)

    def heads_to_keep(self, perm, head, n: int, keep):
        """keep[perm[k]] = head[k]."""
        self._check(self._L.fqd_heads_to_keep(self._h, self._p(perm), self._p(head), n, self._p(keep)))

    # -- FQD_FAST_STRAND=both (csrc/fqd_strand.hip) ------------------------------------------------
    def canonical_reads(self, segs: Sequence[Reads], n: int, out, out_off0, out_len0, flipped, out_off1=None, out_len1=None,
                        out_capacity: Optional[int] = None, count: bool = False) -> Optional[int]:
        """The n records of segs (device memory) in the orientation they are keyed in, packed back to back into out (device
        bytes; out_capacity defaults to out.numel()): Reads(out, out_off0, out_len0) and, for pairs, Reads(out, out_off1,
        out_len1) go into submit; flipped[i] = 1 where record i was turned.  count: wait and return how many were."""
        if len(segs) != self.segments:
            raise ValueError(f"engine has {self.segments} mate(s) per record, got {len(segs)}")
        turned = C.c_uint64(0)
        cap = out.numel() if out_capacity is None else out_capacity
        self._check(self._L.fqd_canonical_reads(self._h, self._desc(segs), n, self._p(out), cap, self._p(out_off0), self._p(out_len0),
                                                self._p(out_off1), self._p(out_len1), self._p(flipped), C.byref(turned) if count else None))
        return int(turned.value) if count else None

    # -- FQD_FAST_UMI (csrc/fqd_umi.hip) ----------------------------------------------------------------
    def umi_find(self, text, id_start, id_len, n: int, sep: str, umi_off, info=True):
        """umi_off[i] (n uint32, device) = where the UMI field starts inside ID line i (id_len[i] bytes at text +
        id_start[i]): behind the last `sep` (':' or '_') of the line's first word.  Returns the call's fqd_umi_info
        (_lib.UmiInfo): record 0's shape, and the lowest refused record with its reason.  info=None hands the library a null
        pointer, which it refuses."""
        got = _lib.UmiInfo() if info else None
        self._check(self._L.fqd_umi_find(self._h, self._p(text), self._p(id_start), self._p(id_len), n, ord(sep), self._p(umi_off),
                                         C.byref(got) if info else None))
        return got

    def umi_reads(self, text, id_start, umi_off, info, mate0: Reads, n: int, out, out_off, out_len, out_capacity: Optional[int] = None):
        """Record i's key bytes — the bases of its UMI field, then mate 1's sequence (mate0, device memory) — packed back to
        back into out (device bytes; out_capacity defaults to out.numel()): Reads(out, out_off, out_len) goes into submit as
        mate 1.  info: what umi_find returned."""
        cap = out.numel() if out_capacity is None else out_capacity
        self._check(self._L.fqd_umi_reads(self._h, self._p(text), self._p(id_start), self._p(umi_off), C.byref(info) if info is not None else None,
                                          self._desc([mate0]), n, self._p(out), cap, self._p(out_off), self._p(out_len)))

    # -- FQD_FAST_UMI_MISMATCH (csrc/fqd_umi_merge.hip) ------------------------------------------------
    def umi_merge(self, text, id_start, umi_off, info, owner_exact, owner_seq, size, n: int, distance: int, owner_out, out=True):
        """owner_out[i] (n uint32, device) = the first record of record i's cluster after the exact UMI clusters of one
        sequence within `distance` mismatches were merged by the directional rule.  info: what umi_find returned;
        owner_exact / owner_seq: owners of the runs keyed UMI ‖ sequence and sequence alone; size: cluster_sizes over the
        exact grouping.  Returns the call's fqd_umi_merge_info (_lib.UmiMergeInfo); out=None hands the library a null
        pointer, which it refuses."""
        got = _lib.UmiMergeInfo() if out else None
        self._check(self._L.fqd_umi_merge(self._h, self._p(text), self._p(id_start), self._p(umi_off), C.byref(info) if info is not None else None,
                                          self._p(owner_exact), self._p(owner_seq), self._p(size), n, distance, self._p(owner_out),
                                          C.byref(got) if out else None))
        return got

    def owners_to_keep(self, owner, n: int, keep):
        """keep[i] = (owner[i] == i)."""
        self._check(self._L.fqd_owners_to_keep(self._h, self._p(owner), n, self._p(keep)))

    # -- FQD_FAST_OPTICAL (csrc/fqd_optical.hip) ------------------------------------------------------------
    def read_places(self, text, id_start, id_len, n: int, tile, x, y, surface, info=True):
        """Per record (device memory, n uint32 each): tile, x and y off the first word of its ID line
        (instrument:run:flowcell:lane:tile:x:y[:UMI]) and surface = the length of fields 1 .. 4 with their colons, with
        _lib.PLACE_SAME_SURFACE set where those bytes are record 0's.  Returns the call's fqd_places_info (_lib.PlacesInfo):
        the lowest refused record with its reason, and the records on another surface than record 0.  info=None hands the
        library a null pointer, which it refuses."""
        got = _lib.PlacesInfo() if info else None
        self._check(self._L.fqd_read_places(self._h, self._p(text), self._p(id_start), self._p(id_len), n, self._p(tile), self._p(x), self._p(y),
                                            self._p(surface), C.byref(got) if info else None))
        return got

    def optical_split(self, perm, head, text, id_start, tile, x, y, surface, n: int, distance: int, owner_out, out=True):
        """owner_out[i] (n uint32, device) = the first record of record i's optical group: the members of its cluster in
        (perm, head) (group_owners') that hang together through pairs on one surface and tile within `distance` pixels in x
        and in y.  tile .. surface: what read_places wrote.  Returns the call's fqd_optical_info (_lib.OpticalInfo); out=None
        hands the library a null pointer, which it refuses."""
        got = _lib.OpticalInfo() if out else None
        self._check(self._L.fqd_optical_split(self._h, self._p(perm), self._p(head), self._p(text), self._p(id_start), self._p(tile), self._p(x),
                                              self._p(y), self._p(surface), n, distance, self._p(owner_out), C.byref(got) if out else None))
        return got

    # -- FQD_FAST_HAMMING (csrc/fqd_near.hip) ----------------------------------------------------------------
    def near_merge(self, segs: Sequence[Reads], owner, n: int, distance: int, owner_out, flags: int = 0, out=True):
        """owner_out[i] (n uint32, device) = the first record of record i's merged cluster: the exact clusters of `owner`
        (owners' over the same n records of segs, device memory) that hang together through pairs of equal shape whose mates
        differ in at most `distance` bytes each.  flags: 0 or _lib.NEAR_WEAK_SEEDS.  Returns the call's fqd_near_info
        (_lib.NearInfo); out=None hands the library a null pointer, which it refuses."""
        if segs is not None and len(segs) != self.segments:
            raise ValueError(f"engine has {self.segments} mate(s) per record, got {len(segs)}")
        got = _lib.NearInfo() if out else None
        self._check(self._L.fqd_near_merge(self._h, self._desc(segs) if segs is not None else None, self._p(owner), n, distance, flags, self._p(owner_out),
                                           C.byref(got) if out else None))
        return got

    def near_merge_umi(self, segs: Sequence[Reads], owner, link, n: int, distance: int, text, id_start, umi_off, info, owner_out, flags: int = 0, out=True):
        """owner_out[i] (n uint32, device) = the first record of record i's molecule: the exact clusters of `owner` (owners' of
        the run keyed UMI ‖ sequence, over the same n records of segs — the sequences as they lie in the files) that hang
        together through pairs under ONE UMI, of equal shape, whose mates differ in at most `distance` bytes each, and through
        link (umi_merge's owner_out, or None for no links).  text, id_start, umi_off, info: umi_find's over file 1.  flags: 0 or
        _lib.NEAR_WEAK_SEEDS.  Returns the call's fqd_near_umi_info (_lib.NearUmiInfo: .near, .links); out=None hands the library
        a null pointer, which it refuses."""
        if segs is not None and len(segs) != self.segments:
            raise ValueError(f"engine has {self.segments} mate(s) per record, got {len(segs)}")
        got = _lib.NearUmiInfo() if out else None
        self._check(self._L.fqd_near_merge_umi(self._h, self._desc(segs) if segs is not None else None, self._p(owner), self._p(link), n, distance, flags,
                                               self._p(text), self._p(id_start), self._p(umi_off), C.byref(info) if info is not None else None,
                                               self._p(owner_out), C.byref(got) if out else None))
        return got

    # -- FQD_FAST_PREFIX (csrc/fqd_prefix.hip) ------------------------------------------------------------------
    def prefix_merge(self, segs: Sequence[Reads], owner, n: int, min_overlap: int, owner_out, span_out=None, flags: int = 0, out=True):
        """owner_out[i] (n uint32, device) = the first record of record i's merged cluster: every exact cluster of `owner`
        (owners' over the same n records of segs, device memory) whose mates have at least `min_overlap` bytes goes to the
        shortest such cluster it is a prefix of, mate by mate (the lowest record among equals).  span_out (n uint32, device, or
        None): len1 + len2 of every record.  flags: 0 or _lib.PREFIX_WEAK_SEEDS.  Returns the call's fqd_prefix_info
        (_lib.PrefixInfo); out=None hands the library a null pointer, which it refuses."""
        if segs is not None and len(segs) != self.segments:
            raise ValueError(f"engine has {self.segments} mate(s) per record, got {len(segs)}")
        got = _lib.PrefixInfo() if out else None
        self._check(self._L.fqd_prefix_merge(self._h, self._desc(segs) if segs is not None else None, self._p(owner), n, min_overlap, flags,
                                             self._p(owner_out), self._p(span_out), C.byref(got) if out else None))
        return got

    # -- FQD_FAST_CONSENSUS (csrc/fqd_consensus.hip) -----------------------------------------------------------
    def consensus(self, perm, head, n: int, text, start, size, seq_off, seq_len, flags: int = 0, changed=None, info=True):
        """One file's text (device bytes, changed in place): the sequence and quality lines of the written member perm[head
        place] of every cluster of two or more members of (perm, head) (group_owners') become the cluster's column-wise
        consensus.  start, size, seq_off, seq_len: scan_records' arrays of the file.  flags: 0 or _lib.CONSENSUS_SMALL_TIERS.
        changed (n bytes by record, or None): set for every written record with a changed base; reads_changed counts only
        those it was not set for before, so a pair is counted once over the two files' calls.  Returns the call's
        fqd_consensus_info (_lib.ConsensusInfo); info=None hands the library a null pointer, which it refuses."""
        got = _lib.ConsensusInfo() if info else None
        self._check(self._L.fqd_consensus(self._h, self._p(perm), self._p(head), n, self._p(text), self._p(start), self._p(size), self._p(seq_off),
                                          self._p(seq_len), flags, self._p(changed), C.byref(got) if info else None))
        return got

    # -- FQD_FAST_CENTROID=abundant (csrc/fqd_centroid.hip) ----------------------------------------------------
    def subcluster_sizes(self, perm, head, label, n: int, abundance, weight=None, info: bool = True):
        """abundance[r] (n uint32, device, by record) = the summed weight (weight: n uint32 by record, None: 1 each) of the
        members of r's run of (perm, head) (group_owners') that share label[r], the exact owner; saturating at 2^32 - 1.
        seq_pick_best over it puts every run's centroid at its head's place.  Returns the call's fqd_centroid_info
        (_lib.CentroidInfo); info=False hands the library a null pointer and returns None."""
        got = _lib.CentroidInfo() if info else None
        self._check(self._L.fqd_subcluster_sizes(self._h, self._p(perm), self._p(head), self._p(label), self._p(weight), n, self._p(abundance),
                                                 C.byref(got) if info else None))
        return got

    def subcluster_scores(self, perm, head, label, score, n: int, masked):
        """Behind the centroid's pick: masked[r] (n uint32, device, by record) = min(score[r], 2^32 - 2) + 1 where label[r] is
        the label of the record at the head place of r's run, 0 elsewhere.  A second seq_pick_best over it keeps the best
        copy of the most abundant sequence."""
        self._check(self._L.fqd_subcluster_scores(self._h, self._p(perm), self._p(head), self._p(label), self._p(score), n, self._p(masked)))

    # -- FQD_FAST_SIZEOUT / FQD_FAST_LEVELS (csrc/fqd_size.hip) --------------------------------------------
    def cluster_sizes(self, perm, head, n: int, size, levels: bool = True):
        """size[perm[k]] (n uint32, device) = the length of the run of (perm, head) that starts at place k where head[k], 0 at
        every other place.  Returns the call's fqd_size_levels (_lib.SizeLevels): runs and records per duplication level and
        the longest run; levels=False hands the library a null pointer and returns None."""
        got = _lib.SizeLevels() if levels else None
        self._check(self._L.fqd_cluster_sizes(self._h, self._p(perm), self._p(head), n, self._p(size), C.byref(got) if levels else None))
        return got

    def size_labels(self, text, start, id_len, rec_size, keep, size, n: int, label_at, out_size):
        """Per record of one file: label_at = the length of '@' and the first word of its ID line (where `;size=N` goes),
        out_size = its size with the label where keep is set: output_plan's `sizes`."""
        self._check(self._L.fqd_size_labels(self._h, self._p(text), self._p(start), self._p(id_len), self._p(rec_size), self._p(keep),
                                            self._p(size), n, self._p(label_at), self._p(out_size)))

    def copy_labelled(self, src, src_off, lens, label_at, size, n: int, dst, dst_off):
        """copy_spans with `;size=<size[i]>` put in at label_at[i]; lens are the grown lengths of output_plan.  dst may be an
        address (int): a window's buffer moved back by the window's first offset."""
        self._check(self._L.fqd_copy_labelled(self._h, self._p(src), self._p(src_off), self._p(lens), self._p(label_at), self._p(size), n,
                                              self._p(dst), self._p(dst_off)))

    # -- FQD_FAST_SORT / FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE (csrc/fqd_size_order.hip) ----------------------
    def size_filter(self, size, n: int, min_size: int, max_size: int, keep):
        """Clears keep[r] of every kept record whose cluster size lies outside min_size .. max_size (max_size 0: no upper
        bound).  Returns (clusters taken out, their records)."""
        clusters, records = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.fqd_size_filter(self._h, self._p(size), n, min_size, max_size, self._p(keep), C.byref(clusters), C.byref(records)))
        return int(clusters.value), int(records.value)

    def size_order(self, perm, head, size, keep, n: int, order) -> int:
        """order[k] (uint32, device) = the record written k-th: the kept head places of (perm, head) sorted stably by cluster
        size descending.  Returns W, the number of entries written; order[W:] is not touched."""
        written = C.c_uint64(0)
        self._check(self._L.fqd_size_order(self._h, self._p(perm), self._p(head), self._p(size), self._p(keep), n, self._p(order), C.byref(written)))
        return int(written.value)

    def size_order_info(self, perm, head, size, keep, n: int, order):
        """size_order through fqd_size_order_ex: returns (W, the call's fqd_size_order_info (_lib.SizeOrderInfo): W, the
        clusters above 255 members that tier 2 sorted apart, the largest size and tier 2's passes)."""
        written, info = C.c_uint64(0), _lib.SizeOrderInfo()
        self._check(self._L.fqd_size_order_ex(self._h, self._p(perm), self._p(head), self._p(size), self._p(keep), n, self._p(order),
                                              C.byref(written), C.byref(info)))
        return int(written.value), info

    def take_u32(self, values, idx, n: int, out):
        """out[k] = values[idx[k]] for k < n (uint32, device)."""
        self._check(self._L.fqd_take_u32(self._h, self._p(values), self._p(idx), n, self._p(out)))

    # -- FQD_FAST_SIZEIN (csrc/fqd_sizein.hip) ------------------------------------------------------------
    def size_annotations(self, text, start, id_len, n: int, expect, weight, label_at, cut, info=True):
        """Per record of one file (device memory; weight, label_at and cut may each be None): weight = what the `;size=N`
        annotation in the first word of its ID line says, 1 where there is none; label_at = the annotation's start, or the
        first word's end; cut = the annotation's length, 0 for none.  expect: file 1's weights for a call over file 2, else
        None.  Returns the call's fqd_sizein_info (_lib.SizeinInfo): the lowest refused record with its reason, the records
        with an annotation and the total weight.  info=None hands the library a null pointer, which it refuses."""
        got = _lib.SizeinInfo() if info else None
        self._check(self._L.fqd_size_annotations(self._h, self._p(text), self._p(start), self._p(id_len), n, self._p(expect), self._p(weight),
                                                 self._p(label_at), self._p(cut), C.byref(got) if info else None))
        return got

    def cluster_weights(self, perm, head, weight, n: int, size, levels: bool = True, info=True):
        """cluster_sizes with a weight per record: size[perm[k]] = the sum of weight over the run that starts at place k where
        head[k], 0 at every other place.  Returns (the call's fqd_size_levels or None, its fqd_weights_info
        (_lib.WeightsInfo): the lowest record at the head of a run above 2^31-1 and that run's sum)."""
        got = _lib.SizeLevels() if levels else None
        over = _lib.WeightsInfo() if info else None
        self._check(self._L.fqd_cluster_weights(self._h, self._p(perm), self._p(head), self._p(weight), n, self._p(size),
                                                C.byref(got) if levels else None, C.byref(over) if info else None))
        return got, over

    def size_relabel(self, rec_size, keep, size, cut, n: int, out_size):
        """out_size = the record's size without its annotation's cut bytes and with the label of size where keep is set:
        output_plan's `sizes`."""
        self._check(self._L.fqd_size_relabel(self._h, self._p(rec_size), self._p(keep), self._p(size), self._p(cut), n, self._p(out_size)))

    def copy_relabelled(self, src, src_off, lens, label_at, cut, size, n: int, dst, dst_off):
        """copy_labelled that leaves the cut[i] bytes behind label_at[i] out.  dst may be an address (int)."""
        self._check(self._L.fqd_copy_relabelled(self._h, self._p(src), self._p(src_off), self._p(lens), self._p(label_at), self._p(cut), self._p(size), n,
                                                self._p(dst), self._p(dst_off)))

    def extract_tags(self, text, id_start, id_len, n: int, tag_off, tag_len):
        self._check(self._L.fqd_extract_tags(self._h, self._p(text), self._p(id_start), self._p(id_len), n, self._p(tag_off), self._p(tag_len)))

    def join_tags(self, a, b, perm_a, perm_b, match_a, match_b, pair_a, pair_b) -> int:
        """a, b = (bytes, offsets, lengths, n); returns the number of pairs (the call drains the stream)."""
        ta, tb = self._tags(*a), self._tags(*b)
        n_pairs = C.c_uint64(0)
        out = _lib.JoinDesc(perm_a=self._p(perm_a), perm_b=self._p(perm_b), match_a=self._p(match_a), match_b=self._p(match_b),
                            pair_a=self._p(pair_a), pair_b=self._p(pair_b), n_pairs=C.pointer(n_pairs))
        self._check(self._L.fqd_join_tags(self._h, C.byref(ta), C.byref(tb), C.byref(out)))
        return int(n_pairs.value)

    def gather_seqs(self, idx, n: int, off_table, len_table, off_out, len_out):
        self._check(self._L.fqd_gather_seqs(self._h, self._p(idx), n, self._p(off_table), self._p(len_table), self._p(off_out), self._p(len_out)))

    def copy_spans(self, src, src_off, lens, n: int, dst, dst_off):
        self._check(self._L.fqd_copy_spans(self._h, self._p(src), self._p(src_off), self._p(lens), n, self._p(dst), self._p(dst_off)))

    def bgzf_bound(self, n: int) -> int:
        return int(self._L.fqd_bgzf_bound(n))

    BGZF_EFFORT = {"fast": 0, "high": 1}                 # FQD_BGZF_FAST, FQD_BGZF_SEARCH

    def bgzf_deflate(self, src, n: int, dst, lines_per_record: int = 4, effort="fast") -> int:
        """BGZF members for the n bytes at src (device) written to dst (device, >= bgzf_bound(n) bytes);
        returns their total size.  The end-of-file marker is the caller's to append.  effort: "fast" (no match
        search, zlib 1-2 class) or "high" (LZ77 search over every member: smaller than zlib 3); a number is handed
        to the library as it is, which refuses what it does not know."""
        total = C.c_uint64(0)
        level = self.BGZF_EFFORT[effort] if isinstance(effort, str) else int(effort)
        self._check(self._L.fqd_bgzf_deflate_ex(self._h, self._p(src), n, lines_per_record, level, self._p(dst), dst.numel(), C.byref(total)))
        return int(total.value)

    def bgzf_inflate(self, comp, comp_off, comp_len, out_off, out_len, crc, n_members: int, text) -> int:
        """Members (device arrays describing them) of the BGZF bytes at comp inflated into text; returns the number
        of members that failed (damaged stream, wrong size or CRC)."""
        bad = C.c_uint64(0)
        self._check(self._L.fqd_bgzf_inflate(self._h, self._p(comp), self._p(comp_off), self._p(comp_len), self._p(out_off), self._p(out_len),
                                             self._p(crc), n_members, self._p(text), C.byref(bad)))
        return int(bad.value)

    def gunzip(self, deflate, avail: int, text, arrived=None):
        """An ordinary gzip member's deflate stream (device bytes from its first byte on) inflated into text (device); returns
        (ok, text_bytes, deflate_bytes, crc32).  arrived: a ctypes.c_uint64 another thread raises while it copies the file into
        `deflate` (fqd_gunzip_arriving: the call works on what is there and waits for the rest)."""
        tb, db, crc, ok = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_int32(0)
        if arrived is None:
            self._check(self._L.fqd_gunzip(self._h, self._p(deflate), avail, self._p(text), text.numel(), C.byref(tb), C.byref(db), C.byref(crc), C.byref(ok)))
        else:
            self._check(self._L.fqd_gunzip_arriving(self._h, self._p(deflate), avail, C.byref(arrived), self._p(text), text.numel(),
                                                    C.byref(tb), C.byref(db), C.byref(crc), C.byref(ok)))
        return bool(ok.value), int(tb.value), int(db.value), int(crc.value)

    def count_lines(self, text, n: int) -> int:
        lines = C.c_uint64(0)
        self._check(self._L.fqd_count_lines(self._h, self._p(text), n, C.byref(lines)))
        return int(lines.value)

    def scan_records(self, text, n: int, lines_per_record: int, n_records: int, start, seq_off, id_len, seq_len, size) -> bool:
        ok = C.c_int(0)
        self._check(self._L.fqd_scan_records(self._h, self._p(text), n, lines_per_record, n_records, self._p(start), self._p(seq_off),
                                             self._p(id_len), self._p(seq_len), self._p(size), C.byref(ok)))
        return bool(ok.value)

    def count_tags_le(self, t, other, other_index: int) -> int:
        """Records of t = (bytes, offsets, lengths, n) whose tag is <= the tag of record other_index of `other`."""
        tt, to = self._tags(*t), self._tags(*other)
        count = C.c_uint64(0)
        self._check(self._L.fqd_count_tags_le(self._h, C.byref(tt), C.byref(to), other_index, C.byref(count)))
        return int(count.value)

    # -- `--unordered` over several GPUs: records dealt by tag range (splitters) ------------------
    def sample_tags(self, t, n_samples: int, stride: int, out_bytes, out_len):
        """Sample k = the tag of record k * n / n_samples of t = (bytes, offsets, lengths, n), cut to `stride` bytes, at
        out_bytes + k * stride; out_len[k] (uint32) = its length.  Only launches."""
        tt = self._tags(*t)
        self._check(self._L.fqd_sample_tags(self._h, C.byref(tt), n_samples, stride, self._p(out_bytes), self._p(out_len)))

    def classify_tags(self, t, split_bytes, split_stride: int, split_len, n_split: int, range_out):
        """range_out[i] (uint32) = number of the n_split ascending splitters (split_bytes + k * split_stride, split_len[k])
        that are < tag i of t = (bytes, offsets, lengths, n).  Only launches."""
        tt = self._tags(*t)
        self._check(self._L.fqd_classify_tags(self._h, C.byref(tt), self._p(split_bytes), split_stride, self._p(split_len), n_split,
                                              self._p(range_out)))

    def range_keep(self, range_, n: int, which: int, keep) -> int:
        """keep[i] = (range_[i] == which) as 0 / 1 bytes; returns how many are set (the call drains the stream)."""
        count = C.c_uint64(0)
        self._check(self._L.fqd_range_keep(self._h, self._p(range_), n, which, self._p(keep), C.byref(count)))
        return int(count.value)

    def max_u32(self, values, n: int) -> int:
        """The largest of n uint32 values, 0 for none (the call drains the stream)."""
        m = C.c_uint32(0)
        self._check(self._L.fqd_max_u32(self._h, self._p(values), n, C.byref(m)))
        return int(m.value)

    def output_offsets(self, keep, idx, n: int, sizes, dest) -> int:
        total = C.c_uint64(0)
        self._check(self._L.fqd_output_offsets(self._h, self._p(keep), self._p(idx), n, self._p(sizes), self._p(dest), C.byref(total)))
        return int(total.value)

    def output_plan(self, keep, idx, n: int, starts, sizes, src_off, lens, dst_off) -> int:
        total = C.c_uint64(0)
        self._check(self._L.fqd_output_plan(self._h, self._p(keep), self._p(idx), n, self._p(starts), self._p(sizes),
                                            self._p(src_off), self._p(lens), self._p(dst_off), C.byref(total)))
        return int(total.value)

    def scatter_flags(self, flags, origin, n: int, keep_out):
        self._check(self._L.fqd_scatter_flags(self._h, self._p(flags), self._p(origin), n, self._p(keep_out)))

    def synth_reads(self, seed: int, first: int, n: int, length: int, dup_permille: int, mate: int, bases, expect_keep=None):
        self._check(self._L.fqd_synth_reads(self._h, seed, first, n, length, dup_permille, mate,
                                            self._p(bases), self._p(expect_keep)))
