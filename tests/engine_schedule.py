"""Schedules against one fqd_engine, the set model they are held against, and the runner.  A module, not a test.

A schedule is a list of steps — Submit, InsertKeys, Widen, Reset, Refused — against ONE engine, chosen so that the engine
crosses from one state to another between (or inside) steps: uniform -> ragged layout, table growth, fresh -> filled
bulk launch, a reset that leaves a stale table, keys widened in mid-run.

  * Source: records (one or two mates, any mix of lengths) over the reads of bulk_placement.Pool; cut() makes shorter
    reads out of longer ones (equal prefix, another length = another key), join() puts sources side by side.  Distinct
    by bulk_placement.first_occurrence_of_reads; .hash is the placement hash of key_layout, so bulk_placement.Picker
    places a Source's records by bucket like a Pool's.
  * Model: a dict from (mate-1 bytes, mate-2 bytes) — for insert_keys the key's words — to the engine index of the first
    record, emptied by a reset.  It never sees a hash.  Beside it, restated from submit_impl / insert_keys_impl /
    fqd_widen_keys of csrc/fqd_engine.hip: the layout (none / uniform / ragged / opaque) and with it stats()["key_bytes"],
    the table's size (bulk_placement.TableSize) and the insert path of every step (predict_path).
  * Runner: drives Engine(profile=True) through the steps and asserts after every one, exactly: the flags, all four
    fields of stats(), the rise of (partition, dedup, insert, encode) launches, links, the keep buffer's tail; at the end
    of every run owners() and group_owners().
  * the scripted schedules (groups L, G, R, W) and the random ones (group S), built here so that
    tests/test_engine_schedule.py checks on the CPU what tests/test_gpu_engine_transitions.py runs.
"""
from dataclasses import dataclass, field
from typing import Any, Optional

import numpy as np

import bulk_placement as bp
import key_layout as kl

FILL = 7                       # what a keep buffer holds before the call
UNWRITTEN = 0xFFFFFFFF         # what a link buffer holds before the call
TAIL = 64                      # bytes (entries) every keep / link buffer is longer than n
MAX_RECORDS = 150_000          # no schedule submits more
CHUNK = 1000                   # FQD_CHUNK_READS of every schedule
FINAL_TEXT = "fqd_submit_final"

SHAPES = {"se32": [(32,)], "se150": [(150,)], "pe150": [(150, 150)], "se75": [(75,)], "ragged149_151": [(149,), (150,), (151,)]}


# ---- records ----------------------------------------------------------------------------------------------------------------
class Source:
    """n distinct records.  mates[m]: (n, width[m]) uint8, zero behind a read's end; lens[m]: (n,) uint32."""
    weak = False

    def __init__(self, mates, lens):
        self.S, self.n = len(mates), len(mates[0])
        self.mates = [np.ascontiguousarray(m, dtype=np.uint8) for m in mates]
        self.lens = [np.ascontiguousarray(l, dtype=np.uint32) for l in lens]
        self.width = [m.shape[1] for m in self.mates]
        for rows, ln in zip(self.mates, self.lens):
            assert np.array_equal(rows != 0, np.arange(rows.shape[1])[None, :] < ln[:, None]), "bases up to the length, zeros behind it"
        # bases are never 0, so the zero-padded rows say the lengths too: equal rows = equal reads of equal lengths
        assert bp.first_occurrence_of_reads(self.mates[0], self.mates[1] if self.S == 2 else None).duplicates == 0, "records are not distinct"
        self._keys = self._hash = self._words = None

    @classmethod
    def of_pool(cls, pool, idx=None):
        idx = np.arange(pool.n) if idx is None else idx
        return cls([m[idx] for m in pool.mates], [l[idx] for l in pool.lens])

    @classmethod
    def join(cls, *parts):
        S = parts[0].S
        width = [max(p.width[m] for p in parts) for m in range(S)]
        mates = [np.concatenate([np.pad(p.mates[m], ((0, 0), (0, width[m] - p.width[m]))) for p in parts]) for m in range(S)]
        return cls(mates, [np.concatenate([p.lens[m] for p in parts]) for m in range(S)])

    def cut(self, idx, lens):
        """The records idx with mate m cut to lens[m] bases (a number, or one per record)."""
        mates, out_lens = [], []
        for m in range(self.S):
            L = np.broadcast_to(np.asarray(lens[m], np.uint32), (len(idx),)).copy()
            assert np.all(L <= self.lens[m][idx])
            rows = self.mates[m][idx].copy()
            rows[np.arange(rows.shape[1])[None, :] >= L[:, None]] = 0
            mates.append(rows); out_lens.append(L)
        return Source(mates, out_lens)

    def shape_of(self, idx):
        """(len0, len1) when all records idx have one shape, else None."""
        l0 = self.lens[0][idx]
        l1 = self.lens[1][idx] if self.S == 2 else np.zeros(len(idx), np.uint32)
        return (int(l0[0]), int(l1[0])) if np.all(l0 == l0[0]) and np.all(l1 == l1[0]) else None

    @property
    def keys(self):
        """What the model sees of a submitted record: (mate-1 bytes, mate-2 bytes or None)."""
        if self._keys is None:
            per = [[rows[i, :ln[i]].tobytes() for i in range(self.n)] for rows, ln in zip(self.mates, self.lens)]
            self._keys = list(zip(per[0], per[1])) if self.S == 2 else [(a, None) for a in per[0]]
        return self._keys

    def _by_shape(self):
        l1 = self.lens[1] if self.S == 2 else np.zeros(self.n, np.uint32)
        code = self.lens[0].astype(np.uint64) << np.uint64(32) | l1.astype(np.uint64)
        for c in np.unique(code):
            sel = np.flatnonzero(code == c)
            t = (int(c >> np.uint64(32)), int(c & np.uint64(kl.M32)))
            yield sel, t, [kl.words_of_rows(np.ascontiguousarray(self.mates[m][sel, :t[m]])) for m in range(self.S)]

    @property
    def hash(self):
        """The placement hash of every record (key_layout.hashes_of_rows), as bulk_placement.Pool has it."""
        if self._hash is None:
            h = np.zeros(self.n, np.uint64)
            for sel, t, w in self._by_shape():
                h[sel] = kl.hashes_of_rows(t[0], w[0]) if self.S == 1 else kl.hashes_of_rows(t[0], w[0], t[1], w[1])
            self._hash = h
        return self._hash

    @property
    def word_keys(self):
        """What the model sees of a key handed to insert_keys: the words of key_layout.expected_padded at the record's own
        lengths (header, mate 1's words, mate 2's: no padding), as bytes.  From words_of_rows, which tests/test_key_layout.py
        holds against expected_words."""
        if self._words is None:
            out = [None] * self.n
            for sel, t, w in self._by_shape():
                header = np.full((len(sel), 1), t[0] | (t[1] << 32), np.uint64)
                rows = np.ascontiguousarray(np.concatenate([header] + w, axis=1))
                for k, i in enumerate(sel):
                    out[int(i)] = rows[k].tobytes()
            self._words = out
        return self._words

    def oracle_arrays(self, idx):
        """Per mate (flat bases, offsets, lengths) of the records idx, for oracle.dedup_single / dedup_paired."""
        out = []
        for m in range(self.S):
            flat = np.concatenate([self.mates[m][idx].reshape(-1), np.zeros(16, np.uint8)])
            out.append((flat, np.arange(len(idx), dtype=np.uint64) * np.uint64(self.width[m]), np.ascontiguousarray(self.lens[m][idx])))
        return out


def describe(source, idx, descriptor):
    """Per mate (bases, offsets, lengths, uniform_len, uniform_stride) as host arrays.  uniform: the reads back to back."""
    out = []
    for m in range(source.S):
        if descriptor == "uniform":
            L = source.lens[m][idx]
            assert np.all(L == L[0]) and L[0] > 0, "a uniform descriptor needs reads of one length"
            L = int(L[0])
            flat = np.concatenate([source.mates[m][idx, :L].reshape(-1), np.zeros(TAIL, np.uint8)])
            out.append((flat, None, None, L, L))
        else:
            w = source.width[m]
            flat = np.concatenate([source.mates[m][idx].reshape(-1), np.zeros(TAIL, np.uint8)])
            out.append((flat, np.arange(len(idx), dtype=np.uint64) * np.uint64(w), np.ascontiguousarray(source.lens[m][idx]), 0, 0))
    return out


_POOLS = {}


def pool_of(shape, n=60_000):
    if (shape, n) not in _POOLS:
        _POOLS[(shape, n)] = bp.Pool(sum(shape.encode()) * 1000 + n % 997, n, SHAPES[shape])
    return _POOLS[(shape, n)]


# ---- steps -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class How:
    descriptor: str = "uniform"            # uniform / ragged
    memory: str = "host"                   # host / device
    linked: bool = False                   # device only
    final: bool = False

    def __str__(self):
        return f"{self.descriptor}/{self.memory}{'/linked' if self.linked else ''}{'/final' if self.final else ''}"


@dataclass
class Submit:
    idx: Any
    how: How = How()

    def __str__(self):
        return f"submit({len(self.idx)}, {self.how})"


@dataclass
class InsertKeys:
    idx: Any
    shape: tuple                           # ("exact", len0, len1) -> encode_uniform; ("padded", max0, max1) -> encode_padded

    def __str__(self):
        return f"insert_keys({len(self.idx)}, {self.shape})"


@dataclass
class Widen:
    new_words: int

    def __str__(self):
        return f"widen({self.new_words})"


@dataclass
class Reset:
    def __str__(self):
        return "reset()"


@dataclass
class BadBase:
    """fqd_bad_base: only ever as the call of a Refused step."""
    def __str__(self):
        return "bad_base()"


@dataclass
class Refused:
    call: Any
    code: int
    text: str

    def __str__(self):
        return f"refused({self.call}, {self.code}, {self.text!r})"


@dataclass
class Schedule:
    name: str
    source: Source
    steps: list
    bulk_min: int = 0                      # FQD_BULK_MIN: 0 or -1
    capacity: int = 0                      # capacity_reads
    seg_bits: Optional[int] = None         # FQD_SEG_BITS when the engine is created (None: unset)
    seg_bits_at: dict = field(default_factory=dict)    # {step number: FQD_SEG_BITS from that step on} (read when a table is made)
    expect: dict = field(default_factory=dict)         # the shape the schedule is named for, see check_shape

    @property
    def env(self):
        return {"FQD_BULK_MIN": str(self.bulk_min), "FQD_CHUNK_READS": str(CHUNK)}

    def told(self, upto=None):
        steps = self.steps if upto is None else self.steps[:upto + 1]
        return f"{self.name} (FQD_BULK_MIN={self.bulk_min}, capacity_reads={self.capacity}): " + "; ".join(f"[{k}] {s}" for k, s in enumerate(steps))


# ---- the paths, restated from submit_impl and insert_keys_impl -------------------------------------------------------------
def predict_path(n, records_before, slots, bulk_min, chunk=CHUNK, encodes=True):
    """(name, (partition, dedup, insert, encode) launches) of one batch; slots: the table AFTER ensure_table.
    encodes: a submit (its encoder is timed); insert_keys hashes keys that are there and is never overlapped."""
    if bulk_min == 0 and bp.bulk_applies(n, records_before, slots):
        return ("bulk_fresh" if records_before == 0 else "bulk_filled"), (1, 1, 0, 1 if encodes else 0)
    if encodes and n >= 2 * chunk:
        launches = -(-n // chunk)
        return "overlapped", (0, 0, launches, launches)
    return "atomic", (0, 0, 1, 1 if encodes else 0)


# ---- the model ---------------------------------------------------------------------------------------------------------------
@dataclass
class Outcome:
    step: Any
    run: int                               # number of resets before it
    first_index: int = 0                   # engine index of the batch's first record
    flags: Any = None
    owners: Any = None                     # engine index of the first record of every record's key
    path: Optional[str] = None
    launches: tuple = (0, 0, 0, 0)
    layout: Optional[str] = None           # after the step
    switched: bool = False                 # the step took a uniform key store to the ragged layout
    relaid: int = 0                        # records that switch laid out again
    grew: tuple = ()                       # (slots before, slots after) where the step made a larger table out of a filled one
    stats: dict = None


class Model:
    def __init__(self, source, capacity=0, bulk_min=0, chunk=CHUNK):
        self.source, self.bulk_min, self.chunk = source, bulk_min, chunk
        self.size = bp.TableSize(capacity)
        self.run = 0
        self._clear()

    def _clear(self):
        self.first = {}                    # key -> engine index of its first record
        self.owner = []                    # per record of this run
        self.records = self.duplicates = 0
        self.layout, self.L, self.W0 = None, None, 0
        self.ragged_words = 0              # sum over the run's records of 1 + seg_words(len0) + seg_words(len1)
        self.kind = None                   # "reads" / "words": what this run's dict is keyed by
        self.finalised = False

    def stats(self):
        key_words = self.ragged_words if self.layout == "ragged" else self.records * self.W0
        return {"records": self.records, "duplicates": self.duplicates, "table_slots": self.size.slots, "key_bytes": 8 * key_words}

    def legal_links(self, i):
        """Every earlier record of record i's key since the last reset."""
        return {j for j in range(i) if self.owner[j] == self.owner[i]}

    def _insert(self, out, keys, idx, encodes):
        n, before, slots_before = len(idx), self.records, self.size.slots
        slots = self.size.after(before + n)
        if slots != slots_before and slots_before and before:
            out.grew = (slots_before, slots)
        out.path, out.launches = predict_path(n, before, slots, self.bulk_min, self.chunk, encodes)
        out.first_index = before
        out.flags, out.owners = np.ones(n, np.uint8), np.empty(n, np.int64)
        for j, i in enumerate(idx):
            f = self.first.setdefault(keys[int(i)], before + j)
            out.owners[j] = f
            if f != before + j:
                out.flags[j] = 0
        self.owner.extend(out.owners.tolist())
        self.records += n
        self.duplicates += int(n - out.flags.sum())

    def apply(self, step):
        out = Outcome(step, self.run)
        src = self.source
        if isinstance(step, Submit):
            assert not self.finalised and self.layout != "opaque" and self.kind in (None, "reads") and len(step.idx)
            self.kind = "reads"
            idx = np.asarray(step.idx)
            uniform = step.how.descriptor == "uniform"
            shape = src.shape_of(idx)
            assert shape is not None or not uniform
            if src.S == 1 and shape is not None:
                shape = (shape[0], 0)
            if self.layout is None and uniform:
                self.layout, self.L, self.W0 = "uniform", shape, kl.seg_words(shape[0]) + kl.seg_words(shape[1])
            elif self.layout != "ragged" and (not uniform or shape != self.L):
                out.switched, out.relaid = self.layout == "uniform", self.records if self.layout == "uniform" else 0
                self.layout = "ragged"
            l1 = src.lens[1][idx] if src.S == 2 else np.zeros(len(idx), np.uint32)
            self.ragged_words += sum(1 + kl.seg_words(int(a)) + kl.seg_words(int(b)) for a, b in zip(src.lens[0][idx], l1))
            self._insert(out, src.keys, idx, True)
            self.finalised = step.how.final
        elif isinstance(step, InsertKeys):
            assert not self.finalised and self.layout != "ragged" and self.kind in (None, "words") and len(step.idx)
            self.kind = "words"
            how, a, b = step.shape
            if how == "exact":
                shape, W = ("uniform", (a, b)), kl.seg_words(a) + kl.seg_words(b)
                assert src.shape_of(np.asarray(step.idx)) == (a, b)
            else:
                W = kl.padded_key_words(a, b)
                shape = ("opaque", W)
                assert np.all(src.lens[0][step.idx] <= a) and (src.S == 1 or np.all(src.lens[1][step.idx] <= b))
            if self.layout is None:
                self.layout, self.L, self.W0 = shape[0], shape[1], W
            assert (self.layout, self.L, self.W0) == (shape[0], shape[1], W), "the engine holds keys of another shape"
            self._insert(out, src.word_keys, np.asarray(step.idx), False)
        elif isinstance(step, Widen):
            assert not self.finalised and self.layout != "ragged"
            if self.layout is not None and self.records:
                assert step.new_words >= self.W0 + (0 if self.layout == "opaque" else 1)
            self.layout, self.L, self.W0 = "opaque", step.new_words, step.new_words
        elif isinstance(step, Reset):
            self.run += 1
            self._clear()
        else:
            assert isinstance(step, Refused)             # changes nothing
        out.layout, out.stats = self.layout, self.stats()
        return out


def trace(schedule):
    """What the model says of every step, before anything is submitted."""
    m = Model(schedule.source, schedule.capacity, schedule.bulk_min)
    return [m.apply(s) for s in schedule.steps]


def runs_of(schedule):
    """Per reset-delimited run: (the pool indices of all its records in order, the model's flags)."""
    runs, idx, flags = [], [], []
    for o in trace(schedule):
        if isinstance(o.step, Reset):
            runs.append((idx, flags)); idx, flags = [], []
        elif o.flags is not None:
            idx.append(np.asarray(o.step.idx)); flags.append(o.flags)
    runs.append((idx, flags))
    return [(np.concatenate(i), np.concatenate(f)) for i, f in runs if i]


def check_shape(schedule):
    """Asserts schedule.expect from the restated predicates:
      slots          the table sizes the schedule passes through, in order
      switch_at      the step that takes the key store to the ragged layout, and relaid, the records it lays out again
      paths          {step number: path}
      includes       paths taken at least once
      dups_across    step numbers T: a record at or after step T is a copy of one before step T, in the same run
      grows_at       step numbers that make a larger table out of a filled one; grows_to: what the last of them makes
      kept_again     after every reset, keys of the run before are present and are kept
      prefixes_kept  (step, records): reads cut out of earlier reads are in that step and are kept
      tag_masks      the slot tag masks of the tables before and after a growth: they differ
    and that no schedule goes beyond MAX_RECORDS."""
    tr, ex, src = trace(schedule), schedule.expect, schedule.source
    assert sum(len(o.step.idx) for o in tr if o.flags is not None) <= MAX_RECORDS
    sizes = []
    for o in tr:
        if o.stats["table_slots"] and (not sizes or sizes[-1] != o.stats["table_slots"]):
            sizes.append(o.stats["table_slots"])
    if "slots" in ex:
        assert sizes == ex["slots"], f"{schedule.name}: the table goes through {sizes}"
    if "switch_at" in ex:
        assert [k for k, o in enumerate(tr) if o.switched] == [ex["switch_at"]], f"{schedule.name}: the layout switch"
        assert tr[ex["switch_at"]].relaid == ex["relaid"]
    elif "slots" in ex:
        assert not any(o.switched for o in tr), f"{schedule.name}: a layout switch nobody named"
    if "prefixes_kept" in ex:                             # an equal prefix at another length is another key
        k, shorter = ex["prefixes_kept"]
        idx = np.asarray(tr[k].step.idx)
        first_place = np.unique(idx, return_index=True)[1]
        mine = first_place[np.isin(idx[first_place], shorter)]
        assert len(mine) and np.all(tr[k].flags[mine] == 1), f"{schedule.name}: the cut reads of step {k}"
    if "tag_masks" in ex:
        assert len(set(ex["tag_masks"])) == len(ex["tag_masks"]), f"{schedule.name}: the tags keep their width"
    for k, path in ex.get("paths", {}).items():
        assert tr[k].path == path, f"{schedule.name}: step {k} takes the {tr[k].path} path, not {path}"
    taken = {o.path for o in tr if o.path}
    assert set(ex.get("includes", ())) <= taken, f"{schedule.name}: takes only {taken}"
    if "grows_at" in ex:
        assert [k for k, o in enumerate(tr) if o.grew] == list(ex["grows_at"]), f"{schedule.name}: growth"
    for T in ex.get("dups_across", ()):
        run, start = tr[T].run, tr[T].first_index if tr[T].flags is not None else None
        if start is None:                                 # a widening: the records held so far
            start = tr[T].stats["records"]
        later = [o for o in tr[T:] if o.run == run and o.flags is not None]
        assert any(np.any((o.flags == 0) & (o.owners < start)) for o in later), f"{schedule.name}: no copy across step {T}"
    if ex.get("kept_again"):
        before, now, kept = set(), set(), {}
        for o in tr:
            if isinstance(o.step, Reset):
                before, now = now, set()
            elif o.flags is not None:
                keys = src.keys if isinstance(o.step, Submit) else src.word_keys
                mine = [keys[int(i)] for i in o.step.idx]
                kept[o.run] = kept.get(o.run, 0) + sum(1 for k, f in zip(mine, o.flags) if f and k in before)
                now.update(mine)
        for run in range(1, tr[-1].run + 1):
            assert kept.get(run, 0) > 0, f"{schedule.name}: run {run} keeps no key of the run before"
    return tr


# ---- the runner (GPU) -----------------------------------------------------------------------------------------------------------
LAUNCHES = ("partition_launches", "dedup_launches", "insert_launches", "encode_launches")


class _Words:
    """Raw device memory as something torch can alias (__cuda_array_interface__)."""
    def __init__(self, ptr, n_words):
        self.__cuda_array_interface__ = {"shape": (n_words,), "typestr": "<i8", "data": (ptr, False), "version": 3, "strides": None}


class Runner:
    """with Runner(schedule, monkeypatch.setenv) as r: r.run() — or r.step(s) one at a time; r.e is the engine."""
    def __init__(self, schedule, setenv, delenv):
        from fastq_dupaway_amd import Engine
        self.sch, self.setenv = schedule, setenv
        for name in ("FQD_SEG_BITS", "FQD_HEAVY_ABOVE", "FQD_DEDUP_THREADS", "FQD_PART_BLOCKS_PER_CU", "FQD_DEDUP_VL"):
            delenv(name, raising=False)
        for name, value in schedule.env.items():             # read when an engine is created
            setenv(name, value)
        if schedule.seg_bits is not None:
            setenv("FQD_SEG_BITS", str(schedule.seg_bits))   # read when a table is made
        self.model = Model(schedule.source, schedule.capacity, schedule.bulk_min)
        self.e = Engine(segments=schedule.source.S, capacity_reads=schedule.capacity, profile=True)
        self.encoder = None                                  # the source side of insert_keys: another engine, as in a sharded run
        self.done = -1
        self.run_keep, self.run_link, self.run_linked = [], [], False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.close()
        if self.encoder is not None:
            self.encoder.close()

    def check(self, ok, what):
        if not ok:
            raise AssertionError(f"{what() if callable(what) else what}\n  after step {self.done + 1} of {self.sch.told(self.done + 1)}")

    # -- descriptors
    def reads(self, idx, descriptor, device):
        import torch
        from fastq_dupaway_amd import Reads
        out = []
        for flat, offs, lens, ulen, ustride in describe(self.sch.source, np.asarray(idx), descriptor):
            if device:
                flat = torch.from_numpy(flat).cuda()
                offs = None if offs is None else torch.from_numpy(offs.view(np.int64)).cuda()
                lens = None if lens is None else torch.from_numpy(lens.view(np.int32)).cuda()
            out.append(Reads(flat, offs, lens, ulen, ustride))
        return out

    def launches(self):
        p = self.e.profile()
        return tuple(p[f] for f in LAUNCHES)

    # -- the calls
    def call_submit(self, step):
        """Returns (keep with its tail, link with its tail or None), both on the host."""
        import torch
        from fastq_dupaway_amd import _lib
        n, how = len(step.idx), step.how
        if how.linked:
            segs = self.reads(step.idx, how.descriptor, True)
            keep = torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda")
            link = torch.full((n + TAIL,), -1, dtype=torch.int32, device="cuda")
            self.e.submit_linked(segs, n, keep, link, last=how.final, memory=None if how.memory == "device" else _lib.MEM_HOST)
            self.e.sync()
            return keep.cpu().numpy(), link.cpu().numpy().view(np.uint32)
        if how.memory == "device":
            keep = torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda")
            self.e.submit(self.reads(step.idx, how.descriptor, True), n, keep=keep, final=how.final)
            self.e.sync()
            return keep.cpu().numpy(), None
        keep = np.full(n + TAIL, FILL, np.uint8)
        self.e.submit(self.reads(step.idx, how.descriptor, False), n, keep=keep, final=how.final)
        return keep, None

    def wire(self, step):
        """The keys of an insert_keys step as they come off the wire: (device words without the hash word, len0, len1)."""
        import torch
        from fastq_dupaway_amd import Engine
        from fastq_dupaway_amd._lib import OPAQUE_KEYS
        if self.encoder is None:
            self.encoder = Engine(segments=self.sch.source.S)
        enc, n, (how, a, b) = self.encoder, len(step.idx), step.shape
        if how == "exact":
            W = enc.key_words(a, b)
            rec = torch.zeros(n * (W + 1), dtype=torch.int64, device="cuda")
            enc.encode_uniform(self.reads(step.idx, "uniform", True), n, rec)
            shape = (a, b)
        else:
            W = enc.padded_key_words(a, b)
            rec = torch.zeros(n * (W + 1), dtype=torch.int64, device="cuda")
            enc.encode_padded(self.reads(step.idx, "ragged", True), n, a, b, rec)
            shape = (W, OPAQUE_KEYS)
        enc.sync()
        return rec.view(n, W + 1)[:, 1:].contiguous().view(-1), W, shape

    def call_insert_keys(self, step, wire, in_place=True):
        import torch
        words, W, shape = wire
        n = len(step.idx)
        keep = torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda")
        if in_place:                                         # receive at the tail of the key store, as the exchange does
            slot = torch.as_tensor(_Words(self.e.reserve_keys(n, *shape), n * W), device="cuda")
            slot.copy_(words)
            words = slot
        self.e.insert_keys(words, n, *shape, keep)
        self.e.sync()
        return keep.cpu().numpy(), None

    # -- one step
    def step(self, step):
        from fastq_dupaway_amd._lib import FqdError
        k = self.done + 1
        if k in self.sch.seg_bits_at:
            self.setenv("FQD_SEG_BITS", str(self.sch.seg_bits_at[k]))
        if isinstance(step, Refused):
            stats, launches = self.e.stats(), self.launches()
            call = step.call
            wire = self.wire(call) if isinstance(call, InsertKeys) else None
            try:
                if isinstance(call, Submit):
                    self.call_submit(call)
                elif isinstance(call, InsertKeys):
                    self.call_insert_keys(call, wire, in_place=False)      # reserve_keys is a call of its own: this is about insert_keys
                elif isinstance(call, Widen):
                    self.e.widen_keys(call.new_words)
                else:
                    self.e.bad_base()
            except FqdError as err:
                self.check(err.code == step.code and step.text in str(err), f"refused with code {err.code}: {err}")
            else:
                self.check(False, "the call was not refused")
            self.check(self.e.stats() == stats == self.model.stats(), lambda: f"stats after the refusal {self.e.stats()}, before it {stats}, model {self.model.stats()}")
            self.check(self.launches() == launches, "a refused call launched")
            self.done = k
            return None
        if isinstance(step, Reset):
            self.end_run()
            self.e.reset()
            out = self.model.apply(step)
        elif isinstance(step, Widen):
            before = self.launches()
            self.e.widen_keys(step.new_words)
            out = self.model.apply(step)
            self.check(self.launches() == before, "widen_keys ran an insert path")
        else:
            wire = self.wire(step) if isinstance(step, InsertKeys) else None
            before = self.launches()
            keep, link = self.call_submit(step) if isinstance(step, Submit) else self.call_insert_keys(step, wire)
            rose = tuple(a - b for a, b in zip(self.launches(), before))
            out = self.model.apply(step)
            n = len(step.idx)
            self.check(rose == out.launches, f"the {out.path} path: (partition, dedup, insert, encode) launches rose by {rose}, not {out.launches}")
            wrong = np.flatnonzero(keep[:n] != out.flags)
            self.check(len(wrong) == 0, lambda: f"{len(wrong)} flags of the batch differ from the model, first at {wrong[:8].tolist()}: got {keep[wrong[:8]].tolist()}")
            self.check(np.all(keep[n:] == FILL), "the keep buffer's tail was written")
            if link is not None:
                self.check(np.all(link[n:] == UNWRITTEN), "the link buffer's tail was written")
                self.check(np.all(link[:n][out.flags == 1] == UNWRITTEN), "a kept record's link was written")
                dup = np.flatnonzero(out.flags == 0)
                to = link[:n][dup].astype(np.int64)
                owner = np.asarray(self.model.owner)
                # the legal set of record i: every earlier record of its key = every j < i with owner[j] == owner[i]
                ok = (to < out.first_index + dup) & (owner[np.minimum(to, len(owner) - 1)] == out.owners[dup])
                self.check(bool(np.all(ok)), lambda: f"links that name no earlier record of the same key, first at batch position {dup[~ok][:8].tolist()}: {to[~ok][:8].tolist()}")
                for i in dup[:: max(1, len(dup) // 20)]:         # the same, spelled out on a sample
                    self.check(int(link[i]) in self.model.legal_links(out.first_index + int(i)), "a link outside the legal set")
                self.run_linked = True
            else:                                                # no links of its own: the model's owners stand in for them in owners()
                link = np.where(out.flags == 0, out.owners, UNWRITTEN).astype(np.uint32)
            self.run_keep.append(keep[:n]); self.run_link.append(link[:n])
        got = self.e.stats()
        self.check(got == out.stats, lambda: f"stats() {got}, the model {out.stats}")
        self.done = k
        return out

    def end_run(self):
        """owners() over the run's batches — links of the linked ones, the model's first occurrence for the others — and
        group_owners over them."""
        import torch
        if self.run_linked:
            keep, link = np.concatenate(self.run_keep), np.concatenate(self.run_link)
            n = len(keep)
            d_keep = torch.from_numpy(keep).cuda()
            d_link = torch.from_numpy(link.view(np.int32)).cuda()
            owner = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            perm = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            head = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
            self.e.owners(d_keep, d_link, n, owner)
            clusters = self.e.group_owners(owner, n, perm, head)
            got = owner.cpu().numpy().view(np.uint32)
            self.check(np.array_equal(got, np.asarray(self.model.owner, np.uint32)), "owners() differ from the model's first occurrences")
            self.check(clusters == len(self.model.first) == int(head.cpu().numpy().sum()), f"group_owners gives {clusters} clusters, the model {len(self.model.first)}")
        self.run_keep, self.run_link, self.run_linked = [], [], False

    def run(self):
        from fastq_dupaway_amd._lib import FqdError
        try:
            for s in self.sch.steps:
                self.step(s)
            self.end_run()
        except FqdError as err:
            self.check(False, f"FqdError {err.code}: {err}")


def run_schedule(schedule, monkeypatch):
    with Runner(schedule, monkeypatch.setenv, monkeypatch.delenv) as r:
        r.run()


# ---- building batches ------------------------------------------------------------------------------------------------------------
def mixed(rng, n, fresh, *repeat_of):
    """A batch of n, shuffled: about a quarter of it repeats of each of the batches repeat_of, the rest the records
    `fresh` in turn (so more than once each where they are fewer than the rest)."""
    parts, left = [], n
    for earlier in repeat_of:
        take = min(left, max(1, n // 4))
        if take and len(earlier):
            parts.append(np.asarray(earlier)[rng.integers(0, len(earlier), take)]); left -= take
    if left:
        rest = np.asarray(fresh) if len(fresh) else np.concatenate(parts)
        parts.append(rest[np.arange(left) % len(rest)])
    b = np.concatenate(parts)
    rng.shuffle(b)
    return b


class Deck:
    """Hands out the records of a range of a source once each."""
    def __init__(self, lo, hi):
        self.at, self.hi = lo, hi

    def take(self, n):
        assert self.at + n <= self.hi, "the pool is used up"
        self.at += n
        return np.arange(self.at - n, self.at)


PLANS = {"atomic": (-1, 1500), "overlapped": (-1, 2500), "bulk": (0, 6000)}      # FQD_BULK_MIN, batch size (slots / 12 = 5462)
PLAN_PATHS = {"atomic": "atomic", "overlapped": "overlapped", "bulk": "bulk_filled"}


def _l_expect(plan, first, n_batches, switch_at, relaid):
    paths = {k: PLAN_PATHS[plan] for k in range(1, n_batches)}
    paths[0] = predict_path(first, 0, bp.MIN_SLOTS, PLANS[plan][0])[0]
    return {"slots": [bp.MIN_SLOTS], "switch_at": switch_at, "relaid": relaid, "paths": paths, "dups_across": [switch_at]}


_SOURCES = {}


def se_source():
    """0..59999: 150 bases; 60000..119999: 149 / 150 / 151 bases; 120000..139999: the first 75 bases of records 0..19999;
    140000..159999: 75 bases of their own."""
    if "se" not in _SOURCES:
        a = Source.of_pool(pool_of("se150"))
        _SOURCES["se"] = Source.join(a, Source.of_pool(pool_of("ragged149_151")), a.cut(np.arange(20_000), (75,)),
                                     Source.of_pool(pool_of("se75"), np.arange(20_000)))
    return _SOURCES["se"]


SE_150, SE_RAGGED, SE_PREFIX75, SE_75 = 0, 60_000, 120_000, 140_000


def pe_source():
    """0..59999: (150, 150); 60000..79999: records 0..19999 with mate 2 cut to 100; 80000..99999: records 0..19999 cut to
    (149, 150) / (150, 149) / (120, 150) in turn; 100000..119999: records 20000..39999 cut to (100, 100)."""
    if "pe" not in _SOURCES:
        a = Source.of_pool(pool_of("pe150"))
        k = np.arange(20_000)
        _SOURCES["pe"] = Source.join(a, a.cut(k, (150, 100)), a.cut(k, (np.array([149, 150, 120])[k % 3], np.array([150, 149, 150])[k % 3])),
                                     a.cut(20_000 + k, (100, 100)))
    return _SOURCES["pe"]


PE_150, PE_150_100, PE_RAGGED, PE_100 = 0, 60_000, 80_000, 100_000


def how(descriptor, memory, linked=False, final=False):
    return How(descriptor, memory, linked, final)


def lh(descriptor, memory):
    """Device batches go through submit_linked, host batches through submit."""
    return How(descriptor, memory, linked=memory == "device")


# ---- group L: the layout switch ------------------------------------------------------------------------------------------------
def L1(plan, memory, first=None):
    """Uniform 150, ragged 149..151 (with 150-base reads of batch 1 described raggedly), uniform 150 again: repeats of
    batch 1, of the 150-base reads batch 2 stored under the ragged layout, and fresh ones."""
    bulk_min, size = PLANS[plan]
    first = size if first is None else first
    src, rng = se_source(), np.random.default_rng(11)
    d150, drag = Deck(SE_150, SE_150 + 60_000), Deck(SE_RAGGED, SE_RAGGED + 60_000)
    b1 = mixed(rng, first, d150.take(max(1, first * 3 // 4)))
    b2 = mixed(rng, size, drag.take(size // 2), b1)
    in2 = b2[src.lens[0][b2] == 150]
    b3 = mixed(rng, size, d150.take(size // 4), b1, in2)
    steps = [Submit(b1, lh("uniform", memory)), Submit(b2, lh("ragged", memory)), Submit(b3, lh("uniform", memory))]
    return Schedule(f"L1-{plan}-{memory}-first{first}", src, steps, bulk_min, expect=_l_expect(plan, first, 3, 1, first))


def L2(plan, memory):
    """Uniform 150, then uniform 75 — a second uniform length alone forces the switch — among them the first 75 bases of
    reads of batch 1, which are other keys and are kept; then uniform 150 with repeats of batch 1."""
    bulk_min, size = PLANS[plan]
    src, rng = se_source(), np.random.default_rng(12)
    b1 = Deck(SE_150, SE_150 + 20_000).take(size)
    prefixes = SE_PREFIX75 + b1[: size // 2]                 # record 120000 + i = the first 75 bases of record i
    own75 = Deck(SE_75, SE_75 + 20_000).take(size // 4)
    b2 = mixed(rng, size, np.concatenate([prefixes, own75]))
    b3 = mixed(rng, size, Deck(SE_150 + 20_000, SE_150 + 60_000).take(size // 2), b1)
    steps = [Submit(b1, lh("uniform", memory)), Submit(b2, lh("uniform", memory)), Submit(b3, lh("uniform", memory))]
    s = Schedule(f"L2-{plan}-{memory}", src, steps, bulk_min, expect=_l_expect(plan, size, 3, 1, size))
    s.expect["prefixes_kept"] = (1, prefixes)
    return s


def L3(plan, memory, first=None):
    """Pairs: uniform (150, 150); uniform (150, 100) — only mate 2's length changes — with mate 1 equal to batch 1's and
    mate 2 its prefix; ragged; uniform (150, 150) with repeats of batch 1."""
    bulk_min, size = PLANS[plan]
    first = size if first is None else first
    src, rng = pe_source(), np.random.default_rng(13)
    b1 = mixed(rng, first, Deck(PE_150, PE_150 + 20_000).take(max(1, first * 3 // 4)))
    cut2 = PE_150_100 + b1[: max(1, first // 2)]             # the same pairs, mate 2 cut to 100
    more = PE_150_100 + np.arange(10_000, 10_000 + size)
    b2 = mixed(rng, size, np.unique(np.concatenate([cut2, more])))
    b3 = mixed(rng, size, PE_RAGGED + np.arange(size // 2), b1, b2)
    b4 = mixed(rng, size, Deck(PE_150 + 20_000, PE_150 + 60_000).take(size // 4), b1, b3[_same_shape(src, b3, b1[0])])
    steps = [Submit(b1, lh("uniform", memory)), Submit(b2, lh("uniform", memory)), Submit(b3, lh("ragged", memory)), Submit(b4, lh("uniform", memory))]
    s = Schedule(f"L3-{plan}-{memory}-first{first}", src, steps, bulk_min, expect=_l_expect(plan, first, 4, 1, first))
    s.expect["prefixes_kept"] = (1, cut2)
    s.expect["dups_across"] = [1, 3]                         # repeats of batch 1 arrive in batch 4
    return s


def L4(plan, memory, paired):
    """The first batch is ragged: the engine was never uniform and nothing is laid out again.  Then uniform batches of two
    lengths, with repeats."""
    bulk_min, size = PLANS[plan]
    rng = np.random.default_rng(14)
    if paired:
        src = pe_source()
        b1 = mixed(rng, size, np.concatenate([PE_RAGGED + np.arange(size // 2), PE_150 + np.arange(size // 4)]))
        u1, u2 = PE_150 + np.arange(size // 2), PE_150_100 + np.arange(size // 2)
    else:
        src = se_source()
        b1 = mixed(rng, size, np.concatenate([SE_RAGGED + np.arange(size // 2), SE_150 + np.arange(size // 4)]))
        u1 = np.concatenate([SE_150 + np.arange(size // 2), b1[src.lens[0][b1] == 150]])
        u2 = SE_75 + np.arange(size // 2)
    b2 = mixed(rng, size, u1)
    b3 = mixed(rng, size, u2)
    b4 = mixed(rng, size, u1[::-1], b2)
    steps = [Submit(b1, lh("ragged", memory))] + [Submit(b, lh("uniform", memory)) for b in (b2, b3, b4)]
    ex = _l_expect(plan, size, 4, 0, 0)
    del ex["switch_at"], ex["relaid"]
    ex["dups_across"] = [1]
    return Schedule(f"L4-{plan}-{memory}-{'pe' if paired else 'se'}", src, steps, bulk_min, expect=ex)


# ---- group G: growth ---------------------------------------------------------------------------------------------------------------
G_SHAPES = ("se150", "pe150", "se75", "ragged149_151")


def _uniform_or_ragged(shape):
    return "ragged" if shape.startswith("ragged") else "uniform"


def _growing(name, src, fresh, sizes, descriptor, bulk_min=0, capacity=0, **more):
    """Batches of the given sizes over the records `fresh` (a Deck); every batch after the first repeats keys of every
    earlier batch; host and device memory in turn."""
    rng = np.random.default_rng(len(name) + sum(sizes))
    batches = []
    for k, n in enumerate(sizes):
        reps = n // (2 * max(1, len(batches))) if batches else 0
        parts = [np.asarray(b)[rng.integers(0, len(b), max(1, reps))] for b in batches]
        left = n - sum(len(p) for p in parts)
        parts.append(fresh.take(left))
        b = np.concatenate(parts)
        rng.shuffle(b)
        batches.append(b)
    steps = [Submit(b, lh(descriptor, "host" if k % 2 else "device")) for k, b in enumerate(batches)]
    return Schedule(name, src, steps, bulk_min, capacity, **more)


G1_SIZES = (16_000, 1000, 4000, 6000, 1000, 5000, 22_000, 1000, 2500, 88_000)
G1_PATHS = ("bulk_fresh", "atomic", "overlapped", "bulk_filled", "atomic", "overlapped", "bulk_filled", "atomic", "overlapped", "bulk_filled")


def G1(shape, seg_bits=None):
    """2^16 -> 2^18 (inside an overlapped batch) -> 2^20 (inside a bulk batch against the filled table), all three paths
    on every table.  seg_bits = (a, b):
    FQD_SEG_BITS is a for the first table and b for the tables made from step 5 on, so that the slot tags change their
    width with the growth (at 13 bits they are 19 bits wide in all three tables)."""
    src = Source.of_pool(pool_of(shape, 100_000))
    s = _growing(f"G1-{shape}" + (f"-segbits{seg_bits[0]}to{seg_bits[1]}" if seg_bits else ""), src, Deck(0, src.n), G1_SIZES, _uniform_or_ragged(shape))
    s.expect = {"slots": [1 << 16, 1 << 18, 1 << 20], "grows_at": [5, 9], "paths": dict(enumerate(G1_PATHS)), "dups_across": [5, 9]}
    if seg_bits:
        s.seg_bits, s.seg_bits_at = seg_bits[0], {5: seg_bits[1]}
        s.expect["tag_masks"] = [bp.tag_mask_for(1 << 16, bp.seg_bits_for(1 << 16, seg_bits[0])), bp.tag_mask_for(1 << 18, bp.seg_bits_for(1 << 18, seg_bits[1]))]
    return s


def G2(path, paired):
    """One submit both switches the layout and grows the table: convert_to_ragged runs first, then ensure_table rehashes
    the keys just laid out again.  That submit on the bulk path or on the atomic one; then repeats on both."""
    n2 = 22_000 if path == "bulk" else 1500
    rng = np.random.default_rng(21 + paired)
    if paired:
        src = pe_source()
        b0, b1 = mixed(rng, 16_000, PE_150 + np.arange(12_000)), mixed(rng, 16_000, PE_150 + np.arange(12_000, 24_000))
        b2 = mixed(rng, n2, PE_150_100 + np.arange(n2 * 3 // 4))           # uniform (150, 100): the second length alone
        fresh3 = PE_150 + np.arange(24_000, 40_000)
        d2 = "uniform"
    else:
        src = se_source()
        b0, b1 = mixed(rng, 16_000, SE_150 + np.arange(12_000)), mixed(rng, 16_000, SE_150 + np.arange(12_000, 24_000))
        b2 = mixed(rng, n2, SE_RAGGED + np.arange(n2), b0, b1)
        fresh3 = SE_150 + np.arange(24_000, 40_000)
        d2 = "ragged"
    like1 = b2[_same_shape(src, b2, b1[0])]                  # what batch 2 holds of batch 1's shape (pairs: nothing)
    b3 = mixed(rng, 1500, fresh3[:400], b0, b1, like1)
    b4 = mixed(rng, 22_000, fresh3[400:], b0, b1, like1)
    b5 = b2[rng.integers(0, len(b2), 1500)]                  # keys stored by the submit that switched and grew
    steps = [Submit(b0, lh("uniform", "host")), Submit(b1, lh("uniform", "device")), Submit(b2, lh(d2, "host")), Submit(b3, lh("uniform", "device")), Submit(b4, lh("uniform", "host")),
             Submit(b5, lh(d2, "device"))]
    ex = {"slots": [1 << 16, 1 << 18], "switch_at": 2, "relaid": 32_000, "grows_at": [2], "dups_across": [2],
          "paths": {0: "bulk_fresh", 1: "bulk_filled", 2: "bulk_filled" if path == "bulk" else "atomic", 3: "atomic", 4: "bulk_filled", 5: "atomic"}}
    return Schedule(f"G2-{path}-{'pe' if paired else 'se'}", src, steps, 0, expect=ex)


def _same_shape(src, idx, like):
    """Mask of the records idx that have record `like`'s lengths."""
    ok = src.lens[0][idx] == src.lens[0][like]
    return ok & (src.lens[1][idx] == src.lens[1][like]) if src.S == 2 else ok


def G3():
    """A table made from capacity_reads = 40 000 (2^17 slots, a size an engine without the hint never has), filled past the
    hint and then past the table: it grows to 2^19, and keys stored under the hint are found again on both paths."""
    src = Source.of_pool(pool_of("se150", 100_000))
    s = _growing("G3-hint40000", src, Deck(0, src.n), (30_000, 1500, 12_000, 3000, 22_000, 1500, 44_000), "uniform", capacity=40_000)
    s.expect = {"slots": [1 << 17, 1 << 19], "grows_at": [4], "dups_across": [4],
                "paths": dict(enumerate(("bulk_fresh", "atomic", "bulk_filled", "overlapped", "overlapped", "atomic", "bulk_filled")))}
    return s


def G4(plan):
    """One submit takes the table from 2^16 straight to 2^20."""
    src = Source.of_pool(pool_of("se150", 100_000))
    s = _growing(f"G4-{plan}", src, Deck(0, src.n), (1000, 132_000, 1500), "uniform", bulk_min=0 if plan == "bulk" else -1)
    first = "bulk_fresh" if plan == "bulk" else "atomic"
    s.expect = {"slots": [1 << 16, 1 << 20], "grows_at": [1], "dups_across": [1],
                "paths": {0: first, 1: "bulk_filled" if plan == "bulk" else "overlapped", 2: "atomic"}}
    return s


# ---- group R: reset ------------------------------------------------------------------------------------------------------------------
EMPTY_BUCKETS = (2, 5)                     # of the 8 buckets of 2^16 slots in 2^13-slot segments


def _run_b(src, rng, run_a_keys, n1, n2):
    """Run B of R1 / R2: a ragged batch that leaves EMPTY_BUCKETS without a record and holds keys of run A, then 75-base
    reads aimed at exactly those buckets: fresh keys, every one twice."""
    geom = bp.geometry(bp.MIN_SLOTS, 13)
    assert geom.n_buckets == 8
    pick = bp.Picker(src, geom)
    ragged = np.zeros(src.n, bool)
    ragged[SE_RAGGED:SE_RAGGED + 60_000] = True
    ragged[run_a_keys] = True                                # 150-base reads of run A, described raggedly
    pick.free &= ragged
    again = run_a_keys[~np.isin(pick.at.bucket[run_a_keys], EMPTY_BUCKETS)][: n1 // 4]
    pick.free[again] = False
    b1 = np.concatenate([again, pick.take_outside(set(EMPTY_BUCKETS), n1 - len(again))])
    rng.shuffle(b1)
    assert not np.any(np.isin(pick.at.bucket[b1], EMPTY_BUCKETS)), "batch 1 must leave these buckets without a record"
    short = bp.Picker(src, geom)
    short.free[:] = False
    short.free[SE_75:SE_75 + 20_000] = True
    fresh = np.concatenate([short.take(b, n2 // 4) for b in EMPTY_BUCKETS])
    b2 = np.concatenate([fresh, fresh])
    rng.shuffle(b2)
    assert set(np.unique(short.at.bucket[b2]).tolist()) == set(EMPTY_BUCKETS)
    return b1, b2


def R1():
    """Run A, uniform 150, ends in a bulk final batch (its segments stay in LDS: the table is garbage).  Everything that
    adds is refused until the reset.  Run B, another shape: a fresh bulk launch that leaves two buckets without a record —
    their segments must be cleared all the same — then an atomic insert into exactly those."""
    src, rng = se_source(), np.random.default_rng(31)
    a1 = mixed(rng, 16_000, SE_150 + np.arange(12_000))
    a2 = mixed(rng, 1000, SE_150 + np.arange(15_000, 15_500), a1)
    a3 = mixed(rng, 6000, SE_150 + np.arange(15_500, 18_500), a1, a2)
    some = SE_150 + np.arange(18_500, 18_600)
    b1, b2 = _run_b(src, rng, np.unique(a1), 8000, 1600)
    final = [Refused(Submit(some, how("uniform", "host")), 1, FINAL_TEXT), Refused(Submit(some, how("uniform", "device", linked=True)), 1, FINAL_TEXT),
             Refused(InsertKeys(some, ("exact", 150, 0)), 1, FINAL_TEXT), Refused(Widen(9), 1, FINAL_TEXT)]
    steps = [Submit(a1, how("uniform", "device")), Submit(a2, how("uniform", "host")), Submit(a3, how("uniform", "device", final=True))] + final + \
            [Reset(), Submit(b1, how("ragged", "device")), Submit(b2, how("uniform", "host"))]
    ex = {"slots": [1 << 16], "kept_again": True, "paths": {0: "bulk_fresh", 1: "atomic", 2: "bulk_filled", 8: "bulk_fresh", 9: "atomic"}}
    return Schedule("R1-final-then-another-shape", src, steps, 0, expect=ex)


def R2():
    """R1 with run A ending on the atomic path, not declared final: the table is live and the reset makes it stale.  Run
    B's first batch is atomic too (FQD_BULK_MIN=-1)."""
    src, rng = se_source(), np.random.default_rng(32)
    a1 = mixed(rng, 16_000, SE_150 + np.arange(12_000))
    a2 = mixed(rng, 1000, SE_150 + np.arange(15_000, 15_500), a1)
    b1, b2 = _run_b(src, rng, np.unique(a1), 1800, 1600)
    steps = [Submit(a1, how("uniform", "device")), Submit(a2, how("uniform", "host")), Reset(), Submit(b1, how("ragged", "device")), Submit(b2, how("uniform", "host"))]
    ex = {"slots": [1 << 16], "kept_again": True, "paths": {0: "overlapped", 1: "atomic", 3: "atomic", 4: "atomic"}}
    return Schedule("R2-live-table-then-another-shape", src, steps, -1, expect=ex)


def R3_full_run(paired):
    """What follows the reported base of R3: Reset, bad_base() refused, a full run."""
    rng = np.random.default_rng(33 + paired)
    src = pe_source() if paired else se_source()
    base = PE_150 if paired else SE_150
    b1 = mixed(rng, 2500, base + np.arange(2000))
    b2 = mixed(rng, 1500, base + np.arange(2000, 3000), b1)
    steps = [Reset(), Refused(BadBase(), 1, ""), Submit(b1, how("uniform", "host")), Submit(b2, how("uniform", "device"))]
    return Schedule(f"R3-{'pe' if paired else 'se'}", src, steps, -1, expect={"slots": [1 << 16], "paths": {2: "overlapped", 3: "atomic"}})


def R4():
    """A paired engine through submit_linked, owners() per run: (150, 150), reset, (100, 100), reset, ragged."""
    src, rng = pe_source(), np.random.default_rng(34)
    steps = []
    for k, (base, descriptor) in enumerate(((PE_150, "uniform"), (PE_100, "uniform"), (PE_RAGGED, "ragged"))):
        if k:
            steps.append(Reset())
        b1 = mixed(rng, 6000, base + np.arange(4000))
        b2 = mixed(rng, 500, base + np.arange(4000, 4200), b1)
        b3 = mixed(rng, 2500, base + np.arange(4200, 5000), b1, b2)
        if k == 2:                                            # the ragged run holds pairs of the first run, described raggedly
            b1 = np.concatenate([b1, PE_150 + np.arange(500)])
        steps += [Submit(b, how(descriptor, "device", linked=True, final=(j == 2 and k == 1))) for j, b in enumerate((b1, b2, b3))]
    ex = {"slots": [1 << 16], "includes": ["bulk_fresh", "atomic", "overlapped"]}
    return Schedule("R4-linked-three-runs", src, steps, 0, expect=ex)


# ---- group W: widening -----------------------------------------------------------------------------------------------------------------
def w_source(paired):
    """0..19999: 60 bases (pairs: (60, 60)); 20000..39999: 77 (77, 96); 40000..59999: 96 (96, 60)."""
    key = "w_pe" if paired else "w_se"
    if key not in _SOURCES:
        a = Source.of_pool(pool_of("pe150" if paired else "se150"))
        k = np.arange(20_000)
        cuts = [(60, 60), (77, 96), (96, 60)] if paired else [(60,), (77,), (96,)]
        _SOURCES[key] = Source.join(*[a.cut(20_000 * j + k, c) for j, c in enumerate(cuts)])
    return _SOURCES[key]


def W1(bulk_min, paired):
    """Owner side: exact 60-base keys up to the first growth (a rehash over exact keys), widen_keys to the padded width of
    96, more keys — copies of the first stage among them — up to the second growth: a rehash over opaque keys."""
    src, rng = w_source(paired), np.random.default_rng(41 + paired)
    exact = ("exact", 60, 60 if paired else 0)
    padded = ("padded", 96, 96 if paired else 0)
    a0 = mixed(rng, 16_000, np.arange(12_000))
    a1 = mixed(rng, 15_000, np.arange(12_000, 18_000), a0)
    a2 = mixed(rng, 3000, np.arange(18_000, 20_000), a0, a1)
    later = np.arange(20_000, 60_000)
    b1 = mixed(rng, 50_000, later[:25_000], a0, a2)
    b2 = mixed(rng, 50_000, later[25_000:], a0, b1)
    W = kl.padded_key_words(*padded[1:])
    steps = [InsertKeys(a0, exact), InsertKeys(a1, exact), InsertKeys(a2, exact), Widen(W), InsertKeys(b1, padded), InsertKeys(b2, padded)]
    bulk = bulk_min == 0
    ex = {"slots": [1 << 16, 1 << 18, 1 << 20], "grows_at": [2, 5], "dups_across": [2, 3, 5],
          "paths": {0: "bulk_fresh" if bulk else "atomic", 1: "bulk_filled" if bulk else "atomic", 2: "atomic", 4: "bulk_filled" if bulk else "atomic", 5: "atomic"}}
    return Schedule(f"W1-bulkmin{bulk_min}-{'pe' if paired else 'se'}", src, steps, bulk_min, expect=ex)


def W2_after_reset():
    """widen_keys on an engine that has been reset only sets the opaque shape; insert_keys of that shape then works."""
    src, rng = w_source(False), np.random.default_rng(42)
    a = mixed(rng, 1500, np.arange(1000))
    b = mixed(rng, 1500, np.concatenate([np.arange(500), np.arange(20_000, 20_500)]))
    W = kl.padded_key_words(96)
    steps = [InsertKeys(a, ("exact", 60, 0)), Reset(), Widen(W), InsertKeys(b, ("padded", 96, 0)), InsertKeys(b[::-1].copy(), ("padded", 96, 0))]
    return Schedule("W2-widen-after-reset", src, steps, 0, expect={"slots": [1 << 16], "kept_again": True})


def W2_widths():
    """widen_keys to exactly W0 + 1 (the header word and nothing else); to the engine's own width (nothing happens); to a
    wider width: earlier keys are still found."""
    src, rng = w_source(False), np.random.default_rng(43)
    W0 = kl.seg_words(60)
    assert kl.padded_key_words(60) == W0 + 1
    a = mixed(rng, 1500, np.arange(1000))
    b = mixed(rng, 1500, np.arange(1000, 1500), a)
    c = mixed(rng, 1500, np.arange(1500, 2000), a, b)
    d = mixed(rng, 1500, np.arange(20_000, 21_000), a, c)
    steps = [InsertKeys(a, ("exact", 60, 0)), Widen(W0 + 1), InsertKeys(b, ("padded", 60, 0)), Widen(W0 + 1), InsertKeys(c, ("padded", 60, 0)),
             Widen(kl.padded_key_words(96)), InsertKeys(d, ("padded", 96, 0))]
    return Schedule("W2-widths", src, steps, 0, expect={"slots": [1 << 16], "dups_across": [1, 3, 5]})


def W3_opaque():
    """Refusals on the owner side: narrower than the keys held; insert_keys of another shape; submit on opaque keys."""
    src, rng = w_source(False), np.random.default_rng(44)
    a = mixed(rng, 1500, np.arange(1000))
    b = mixed(rng, 1500, np.arange(1000, 1500), a)
    other = np.arange(20_000, 20_100)                         # 77 bases
    W0 = kl.seg_words(60)
    steps = [InsertKeys(a, ("exact", 60, 0)),
             Refused(Widen(W0), 1, "narrower"), Refused(InsertKeys(other, ("exact", 77, 0)), 1, "another shape"),
             InsertKeys(b, ("exact", 60, 0)), Widen(W0 + 1),
             Refused(Submit(a[:100], how("uniform", "host")), 1, "opaque keys"), Refused(Submit(a[:100], how("uniform", "device")), 1, "opaque keys"),
             Refused(Widen(W0), 1, "narrower"), Refused(InsertKeys(a[:100], ("exact", 60, 0)), 1, "another shape"),
             InsertKeys(mixed(rng, 1500, np.arange(1500, 2000), a, b), ("padded", 60, 0))]
    return Schedule("W3-owner-side", src, steps, 0, expect={"slots": [1 << 16], "dups_across": [3, 9]})


def W3_ragged():
    """Refusals on an engine that submits: submit_linked with host memory; widen_keys on a ragged engine."""
    src, rng = se_source(), np.random.default_rng(45)
    a = mixed(rng, 1500, SE_150 + np.arange(1000))
    b = mixed(rng, 1500, SE_RAGGED + np.arange(1000), a)
    c = mixed(rng, 1500, SE_150 + np.arange(1000, 1500), a, b[src.lens[0][b] == 150])
    steps = [Submit(a, how("uniform", "device")), Refused(Submit(a[:100], how("uniform", "host", linked=True)), 1, "fqd_submit_linked"),
             Submit(b, how("ragged", "host")), Refused(Widen(16), 1, "ragged layout"), Refused(Submit(a[:100], how("ragged", "host", linked=True)), 1, "fqd_submit_linked"),
             Submit(c, how("uniform", "device", linked=True))]
    return Schedule("W3-submit-side", src, steps, 0, expect={"slots": [1 << 16], "switch_at": 2, "relaid": 1500, "dups_across": [2]})


# ---- group S: random schedules -----------------------------------------------------------------------------------------------------------
SEEDS = tuple(range(8))


def random_schedule(seed):
    """Ten to fourteen steps drawn from: submit (uniform / ragged x host / device, linked or not on the device; 1..300,
    2000..5000 or slots / 12 .. slots / 6 records), reset, and a final batch followed by a reset.  FQD_BULK_MIN=0.  Odd
    seeds are paired.  Every batch mixes records not yet used with repeats of this run and of the runs before."""
    rng = np.random.default_rng(1000 + seed)
    paired = bool(seed % 2)
    src = pe_source() if paired else se_source()
    if paired:
        groups = {"a": Deck(PE_150, PE_150 + 60_000), "b": Deck(PE_150_100, PE_150_100 + 20_000), "r": Deck(PE_RAGGED, PE_RAGGED + 20_000)}
    else:
        groups = {"a": Deck(SE_150, SE_150 + 60_000), "b": Deck(SE_75, SE_75 + 20_000), "r": Deck(SE_RAGGED, SE_RAGGED + 60_000)}
    model = Model(src, 0, 0)
    steps, seen, total = [], {g: [] for g in groups}, 0
    n_steps = int(rng.integers(10, 15))
    while len(steps) < n_steps:
        room = n_steps - len(steps)
        roll = rng.random()
        if model.records and roll < 0.12:
            steps.append(Reset()); model.apply(steps[-1])
            continue
        final = model.records > 0 and roll < 0.22 and room >= 2
        descriptor = "ragged" if rng.random() < 0.4 else "uniform"
        memory = "device" if rng.random() < 0.6 else "host"
        linked = memory == "device" and rng.random() < 0.6
        slots = model.size.slots or bp.MIN_SLOTS
        lo, hi = [(1, 300), (2000, 5000), (-(-slots // 12), slots // 6)][int(rng.integers(0, 3))]
        n = int(rng.integers(lo, hi + 1))
        if total + n > MAX_RECORDS - 6000:                   # what is left goes to small batches
            n = int(rng.integers(1, 301))
        if descriptor == "uniform":
            g = "a" if rng.random() < 0.7 else "b"
            old = seen[g]
            take = min(max(1, n // 2), groups[g].hi - groups[g].at)
            fresh = groups[g].take(take)
        else:
            old = [b for g in groups for b in seen[g]]
            take = min(max(1, n // 2), groups["r"].hi - groups["r"].at)
            fresh, g = groups["r"].take(take), "r"
        b = mixed(rng, n, fresh, *[old[int(k)] for k in rng.permutation(len(old))[:2]])
        seen[g].append(b)
        steps.append(Submit(b, How(descriptor, memory, linked, final)))
        model.apply(steps[-1])
        total += n
        if final:
            steps.append(Reset()); model.apply(steps[-1])
    return Schedule(f"S-seed{seed}", src, steps, 0)


# ---- the registry ---------------------------------------------------------------------------------------------------------------------------
def scripted():
    """{name: builder} of every scripted schedule; tests/test_engine_schedule.py walks all of them on the CPU."""
    out = {}

    def add(builder, *args):
        out["-".join([builder.__name__] + [str(a) for a in args])] = lambda: builder(*args)
    for plan in PLANS:
        for memory in ("host", "device"):
            add(L1, plan, memory); add(L2, plan, memory); add(L3, plan, memory)
            add(L4, plan, memory, False)
        add(L4, plan, "device", True)
    for first in (1, 257, 6000):
        add(L1, "atomic", "device", first); add(L3, "atomic", "device", first)
    for shape in G_SHAPES:
        add(G1, shape)
    add(G1, "se150", (12, 14))
    for path in ("bulk", "atomic"):
        for paired in (False, True):
            add(G2, path, paired)
    add(G3)
    add(G4, "bulk"); add(G4, "overlapped")
    add(R1); add(R2); add(R3_full_run, False); add(R3_full_run, True); add(R4)
    for bulk_min in (0, -1):
        for paired in (False, True):
            add(W1, bulk_min, paired)
    add(W2_after_reset); add(W2_widths); add(W3_opaque); add(W3_ragged)
    return out
