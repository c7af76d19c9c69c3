"""CPU checks of tests/engine_schedule.py: the model against the oracle, every scripted schedule against the shape it is
named for (table sizes, layout switch, paths — from the restated predicates, before anything is submitted), and the
random generator's coverage.  tests/test_gpu_engine_transitions.py runs the same schedules against real engines."""
import numpy as np
import pytest

import bulk_placement as bp
import engine_schedule as es

SCRIPTED = es.scripted()
_BUILT = {}


def built(name):
    if name not in _BUILT:
        _BUILT[name] = SCRIPTED[name]() if name in SCRIPTED else es.random_schedule(int(name[len("S-seed"):]))
    return _BUILT[name]


EVERY = list(SCRIPTED) + [f"S-seed{seed}" for seed in es.SEEDS]


@pytest.mark.parametrize("name", EVERY)
def test_model_flags_equal_the_oracle(oracle, name):
    """Every reset-delimited run, its batches concatenated: the dict's flags are dedup_single's / dedup_paired's.  Keys
    handed to insert_keys are words in the model and reads in the oracle."""
    s = built(name)
    runs = es.runs_of(s)
    assert runs
    for idx, flags in runs:
        arrays = s.source.oracle_arrays(idx)
        exp = oracle.dedup_paired(*arrays[0], *arrays[1]) if s.source.S == 2 else oracle.dedup_single(*arrays[0])
        assert np.array_equal(flags, exp), f"{s.name}: {int((flags != exp).sum())} of {len(idx)} flags differ from the oracle"
        assert 0 < int((exp == 0).sum()) < len(idx)


@pytest.mark.parametrize("name", list(SCRIPTED))
def test_schedule_has_the_shape_it_is_named_for(name):
    s = built(name)
    assert s.expect, "a scripted schedule says what it is there for"
    es.check_shape(s)


def test_placement_hash_of_a_source_is_the_pools():
    """Source.hash is what bulk_placement.Pool computes for the same records, also behind join()."""
    for shape in ("se150", "ragged149_151"):
        pool = es.pool_of(shape)
        assert np.array_equal(es.Source.of_pool(pool).hash, pool.hash)
    src = es.se_source()
    assert np.array_equal(src.hash[es.SE_RAGGED:es.SE_RAGGED + 60_000], es.pool_of("ragged149_151").hash)
    assert src.shape_of(np.arange(es.SE_PREFIX75, es.SE_PREFIX75 + 5)) == (75, 0)
    assert np.array_equal(src.mates[0][es.SE_PREFIX75 + 3, :75], src.mates[0][3, :75]) and src.keys[es.SE_PREFIX75 + 3][0] == src.keys[3][0][:75]


def test_paths_are_the_restated_predicates():
    slots = bp.MIN_SLOTS
    assert es.predict_path(1, 0, slots, 0) == ("bulk_fresh", (1, 1, 0, 1))
    assert es.predict_path(5461, 10, slots, 0) == ("overlapped", (0, 0, 6, 6))
    assert es.predict_path(5462, 10, slots, 0) == ("bulk_filled", (1, 1, 0, 1))
    assert es.predict_path(5462, 10, slots, 0, encodes=False) == ("bulk_filled", (1, 1, 0, 0))
    assert es.predict_path(60_000, 0, slots, -1) == ("overlapped", (0, 0, 60, 60))
    assert es.predict_path(60_000, 0, slots, -1, encodes=False) == ("atomic", (0, 0, 1, 0))
    assert es.predict_path(1999, 0, slots, -1) == ("atomic", (0, 0, 1, 1))
    assert es.predict_path(2000, 0, slots, -1) == ("overlapped", (0, 0, 2, 2)) and es.predict_path(2001, 5, slots, -1)[1] == (0, 0, 3, 3)


def test_key_bytes_follow_the_layout():
    """8 * n * W0 while uniform; from the switch on 8 * the sum of 1 + seg_words(len0) + seg_words(len1) over ALL records held."""
    tr = es.trace(built("L2-atomic-host"))
    n = 1500
    assert [o.stats["key_bytes"] for o in tr] == [8 * n * 8, 8 * (n * 9 + n * 6), 8 * (n * 9 + n * 6 + n * 9)]
    tr = es.trace(built("W2_widths"))
    assert [o.stats["key_bytes"] // (8 * 1500) for o in tr] == [3, 4, 8, 8, 12, 18, 24]


def test_random_schedules_cover_what_they_are_for():
    seen, linked_on = set(), set()
    for seed in es.SEEDS:
        s = built(f"S-seed{seed}")
        assert s.bulk_min == 0 and 10 <= len(s.steps) <= 14
        tr = es.trace(s)
        assert sum(len(o.step.idx) for o in tr if o.flags is not None) <= es.MAX_RECORDS
        for o in tr:
            if o.path:
                seen.add(o.path)
                if o.step.how.linked:
                    linked_on.add(o.path.split("_")[0])
            if o.switched:
                seen.add("switch")
            if o.grew:
                seen.add("growth")
            if isinstance(o.step, es.Reset):
                seen.add("reset")
    assert seen >= {"atomic", "overlapped", "bulk_fresh", "bulk_filled", "switch", "growth", "reset"}
    assert linked_on == {"atomic", "overlapped", "bulk"}
