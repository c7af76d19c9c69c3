"""One fqd_engine across its transitions: key layout (none / uniform / ragged / opaque) x table (none, stale, live, grown,
sized from a hint) x insert path (atomic, overlapped, bulk fresh and against a filled table), with fqd_submit_final,
fqd_engine_reset and fqd_widen_keys in between.  The schedules, the set model they are held against and the runner
that asserts after every step are tests/engine_schedule.py; tests/test_engine_schedule.py checks on the CPU that the
model equals the oracle and that every schedule crosses the transitions it is named for.

  L  the layout switch (relayout_ragged_kernel, single-end and paired), on each path, host and device descriptors
  G  growth between and inside the other transitions (rehash_kernel over relaid, hinted and opaque key stores)
  R  reset and the tables it leaves (a final batch's garbage, a live table gone stale)
  W  widen_keys with the rest, and what is refused
  S  random schedules, seeds 0..7

Nothing is compared with a tolerance.  FQD_CHUNK_READS=1000 throughout; FQD_BULK_MIN is the schedule's.
"""
import numpy as np
import pytest

from fastq_dupaway_amd._lib import FqdError
import engine_schedule as es

pytestmark = pytest.mark.gpu

SCRIPTED = es.scripted()


def names(prefix):
    return [n for n in SCRIPTED if n.startswith(prefix)]


def run(name, monkeypatch):
    es.run_schedule(SCRIPTED[name](), monkeypatch)


@pytest.mark.parametrize("name", names("L1") + names("L2") + names("L3") + names("L4"))
def test_layout_switch(monkeypatch, name):
    """L1: uniform 150 / ragged 149..151 / uniform 150.  L2: a second uniform length alone.  L3: pairs, only mate 2's
    length changes, then ragged, then repeats of batch 1 — the header L0 | L1 << 32 and the stride W0 + 1.  L4: ragged from
    the first batch on.  first1 / first257 / first6000: the relayout's grid over one record, a block and a record, and
    several blocks."""
    run(name, monkeypatch)


@pytest.mark.parametrize("name", names("G1"))
def test_growth_twice_on_alternating_paths(monkeypatch, name):
    """2^16 -> 2^18 -> 2^20 with bulk / atomic / overlapped batches on every table; segbits12to14: the second and third
    table have 2^14-slot segments after a first of 2^12, so the slot tags change their width with the first growth."""
    run(name, monkeypatch)


@pytest.mark.parametrize("name", names("G2"))
def test_one_submit_switches_the_layout_and_grows_the_table(monkeypatch, name):
    run(name, monkeypatch)


@pytest.mark.parametrize("name", names("G3") + names("G4"))
def test_growth_from_a_hinted_table_and_by_two_sizes_at_once(monkeypatch, name):
    run(name, monkeypatch)


@pytest.mark.parametrize("name", ["R1", "R2", "R4"])
def test_reset_and_the_table_it_leaves(monkeypatch, name):
    run(name, monkeypatch)


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_reset_after_a_reported_base(monkeypatch, paired):
    """R3: an unknown base is reported (code 3); after reset() bad_base() is refused, all counters are zero, and a full
    run gives the model's flags."""
    s = SCRIPTED[f"R3_full_run-{paired}"]()
    src, n = s.source, 2001
    idx = np.arange(n)                                       # (150) / (150, 150) records
    with es.Runner(s, monkeypatch.setenv, monkeypatch.delenv) as r:
        segs = r.reads(idx, "uniform", False)
        at = (678, src.S - 1, 29)
        segs[at[1]].bases[at[0] * 150 + at[2]] = ord("n")
        with pytest.raises(FqdError) as err:
            r.e.submit(segs, n)
        assert err.value.code == 3 and r.e.bad_base() == (at[0], at[1], at[2], ord("n"))
        assert r.e.stats()["records"] == n
        r.model.size.after(n)                                # the table that submit made stays
        r.run()
        st = r.e.stats()
        assert st["records"] == 4000 and st["table_slots"] == 1 << 16


@pytest.mark.parametrize("name", names("W1"))
def test_owner_widens_between_two_growths(monkeypatch, name):
    run(name, monkeypatch)


@pytest.mark.parametrize("name", names("W2") + names("W3"))
def test_widen_keys_edges_and_refusals(monkeypatch, name):
    run(name, monkeypatch)


@pytest.mark.parametrize("seed", es.SEEDS)
def test_random_schedule(monkeypatch, seed):
    es.run_schedule(es.random_schedule(seed), monkeypatch)
