"""fqd_subcluster_sizes and fqd_subcluster_scores in the cases of tests/test_gpu_buffer_extents.py: every buffer of the call in
a guarded arena, at addresses aligned to the element size and to nothing more, the arena filled with 0xFF and with '\\n', the
results equal to those of a plain run and every byte outside the outputs as it was.

The rows live here, in the file of the feature that brought the two entries, and are ADDED TO THAT MODULE'S TABLE when this
file is imported: its test that every exported entry with a device buffer runs in a case reads the table when it runs, behind
the collection of both files.  (Run alone, without this file, that test names the two entries as missing: the suite is run
whole.)  The cases use that module's helpers as they are."""
import numpy as np
import pytest

from fastq_dupaway_amd import Engine
import test_gpu_buffer_extents as ext

pytestmark = pytest.mark.gpu
u32 = np.uint32


def case_subcluster_sizes(A, weighted):
    """The clusters by sequence, the labels by UMI and sequence: a cluster holds several sub-clusters."""
    R = ext.resident_run()
    n = R["n"]
    perm, head, label, abundance = A.inp("perm", R["perm"]), A.inp("head", R["head"]), A.inp("label", R["owner_exact"]), A.out("abundance", u32, n)
    weight = A.inp("weight", (1 + np.arange(n) % 5).astype(u32)) if weighted else None
    A.ready()
    with Engine(segments=1) as e:
        got = e.subcluster_sizes(perm, head, label, n, abundance, weight)
    return dict(abundance=abundance, info=[got.clusters, got.mixed, got.subclusters, got.largest] + list(got.tier_clusters),
                _nontrivial=lambda o: o["info"][1] > 5 and o["info"][2] > o["info"][0] and o["info"][3] == 65 and len(np.unique(o["abundance"])) >= 3)


def case_subcluster_scores(A):
    R = ext.resident_run()
    n = R["n"]
    rng = np.random.default_rng(5)
    ins = [A.inp("perm", R["perm"]), A.inp("head", R["head"]), A.inp("label", R["owner_exact"]), A.inp("score", rng.integers(0, 50, n).astype(u32))]
    masked = A.out("masked", u32, n)
    A.ready()
    with Engine(segments=1) as e:
        e.subcluster_scores(*ins, n, masked)
    return dict(masked=masked, _nontrivial=lambda o: 50 < int((o["masked"].view(u32) == 0).sum()) < n - 50 and int(o["masked"].view(u32).max()) == 50)


ROWS = [ext.Case("fqd_subcluster_sizes", "", lambda A: case_subcluster_sizes(A, False)), ext.Case("fqd_subcluster_sizes", "weighted", lambda A: case_subcluster_sizes(A, True)),
        ext.Case("fqd_subcluster_scores", "", case_subcluster_scores)]
ext.TABLE.extend(row for row in ROWS if row.id not in {c.id for c in ext.TABLE})


@pytest.mark.parametrize("case", ROWS, ids=[c.id for c in ROWS])
def test_buffers_are_respected(case):
    """ext.test_buffers_are_respected_wherever_they_lie over these rows (none of them takes offsets into a text: no far run)."""
    assert not case.far and not case.env
    results = {}
    for mode in ("plain", "ff", "nl"):
        try:
            results[mode], nontrivial = ext.run_case(case.fn, mode, None)
        except Exception as ex:                                        # after a GPU FAULT nothing more is started on the card
            if any(word in str(ex).lower() for word in ext.GPU_FAULT_WORDS):
                pytest.exit(f"{case.id}, {mode} run: {ex}", returncode=3)
            raise
    plain = results["plain"]
    assert nontrivial(plain), f"{case.id}: the plain run's outputs are trivial or not what the inputs were built to give"
    for mode in ("ff", "nl"):
        got = results[mode]
        assert got.keys() == plain.keys()
        for k in plain:
            assert ext.same(plain[k], got[k]), f"{case.id}: '{k}' of the {mode} run differs from the plain run's: {ext.first_difference(plain[k], got[k])}"


def test_the_rows_are_in_the_table():
    covered = {name for c in ext.TABLE for name in c.entries}
    assert {"fqd_subcluster_sizes", "fqd_subcluster_scores"} <= covered
    assert not {"fqd_subcluster_sizes", "fqd_subcluster_scores"} & ext.NOT_IN_THE_TABLE
