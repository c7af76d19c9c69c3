"""fqd_prefix_merge in the cases of tests/test_gpu_buffer_extents.py: every buffer of the call in a guarded arena, at addresses
aligned to the element size and to nothing more, the arena filled with 0xFF and with '\\n', the reads' text also across byte 2^32
of an allocation of more than 4 GiB; the results equal to those of a plain run — which are the sequential statement's
(tests/prefix_reference.py) — and every byte outside the outputs as it was.

The rows live here, in the file of the feature that brought the entry, and are ADDED TO THAT MODULE'S TABLE when this file is
imported, as tests/test_gpu_centroid_extents.py adds its own: the test that every exported entry with a device buffer runs in a
case reads the table when it runs, behind the collection of all three files.  (Run alone, without this file, that test names the
entry as missing: the suite is run whole.)  The cases use that module's helpers as they are."""
import random

import numpy as np
import pytest

from fastq_dupaway_amd import Engine, Reads, _lib
import prefix_reference as ref
import test_gpu_buffer_extents as ext
from prefix_cases import chain, pair_directions, random_records, scattered, star, two_maximal
from test_gpu_buffer_extents import far_holder                 # noqa: F401  (the fixture: an arena of more than 4 GiB, made when a far run asks)

pytestmark = pytest.mark.gpu
u8, u32, u64 = np.uint8, np.uint32, np.uint64
L = 20


def reads_of(paired):
    """Chains, a star, two maximal reads over a short one, random cuts with copies; for pairs the direction cases as well."""
    def make():
        rng = random.Random(31 + paired)
        if paired:
            nodes = pair_directions(rng, L)[0] + chain(rng, L, 5, paired=True)
            return scattered(rng, nodes) + random_records(rng, L, nodes=150, templates=12, paired=True)
        nodes = chain(rng, L, 9) + star(rng, L)[0] + two_maximal(rng, L)
        return scattered(rng, nodes) + random_records(rng, L, nodes=200, templates=15)
    return ext.cached(("prefix_reads", paired), make)


def case_prefix_merge(A, paired, flags):
    records = reads_of(paired)
    n = len(records)
    segs = []
    for m in range(2 if paired else 1):
        mates = [r[m] for r in records]
        lens = np.array([len(x) for x in mates], u32)
        offs = np.zeros(n, u64)
        offs[1:] = np.cumsum(lens[:-1] + u32(1))                # a '\n' behind every read, the last one too
        T = A.text(f"text{m}", np.frombuffer(b"".join(x + b"\n" for x in mates), u8))
        segs.append(Reads(T.base, offsets=A.inp(f"seq_off{m}", offs + u64(T.bias)), lengths=A.inp(f"seq_len{m}", lens)))
    owner_h = ref.exact_owners(records)
    want, counts = ref.merged_owners(records, L)
    owner, owner_out, span_out = A.inp("owner", owner_h), A.out("owner_out", u32, n), A.out("span_out", u32, n)
    A.ready()
    with Engine(segments=len(segs)) as e:
        got = e.prefix_merge(segs, owner, n, L, owner_out, span_out, flags)
    said = [got.nodes, got.eligible, got.merged, got.groups, got.pairs, got.related, got.children, got.largest_group, got.deepest, got.jumps, got.over_limit_first,
            got.over_limit_nodes]
    return dict(owner_out=owner_out, span_out=span_out, info=said,
                _nontrivial=lambda o: (o["info"][6] > 20 and o["info"][8] >= 3 and np.array_equal(o["owner_out"].view(u32), want) and
                                       not np.array_equal(want, owner_h) and np.array_equal(o["span_out"].view(u32), ref.spans(records)) and
                                       (o["info"][0], o["info"][2], o["info"][6], o["info"][8]) == (counts["nodes"], counts["merged"], counts["children"], counts["deepest"])))


ROWS = [ext.Case("fqd_prefix_merge", f"{'pe' if paired else 'se'}-{name}", lambda A, paired=paired, flags=flags: case_prefix_merge(A, paired, flags), far=True)
        for paired in (False, True) for flags, name in ((0, "seeds"), (_lib.PREFIX_WEAK_SEEDS, "weak_seeds"))]
ext.TABLE.extend(row for row in ROWS if row.id not in {c.id for c in ext.TABLE})


@pytest.mark.parametrize("case", ROWS, ids=[c.id for c in ROWS])
def test_buffers_are_respected_wherever_they_lie(case, monkeypatch, far_holder):      # noqa: F811
    """That module's test over these rows: plain, 0xFF, '\\n' and the far run."""
    ext.test_buffers_are_respected_wherever_they_lie(case, monkeypatch, far_holder)


def test_the_rows_are_in_the_table():
    covered = {name for c in ext.TABLE for name in c.entries}
    assert "fqd_prefix_merge" in covered and "fqd_prefix_merge" not in ext.NOT_IN_THE_TABLE
