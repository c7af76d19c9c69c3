"""hamming_walk_kernel (fqd_seq_heads in tail-hamming mode, csrc/fqd_seq.hip) on lists whose clusters end on chosen lanes
of the wave's 64 places and whose members lie at exactly d, d + 1, 2d and 2d + 1 substitutions, placed on the edges of
the 8-byte words and of the tail of fqdseq::mismatches (reads of 37 and of 5 bytes).  The lists are those of
tests/hamming_walk_cases.py, built in sorted order with their heads and held to that on the host by
tests/test_edge_inputs.py.  Here the device sort must give tests/seq_reference.py's order, and the heads and their
count must equal seq_reference.heads: exact equality throughout."""
import numpy as np
import pytest
import torch

import hamming_walk_cases as hw
import seq_reference as ref
from fastq_dupaway_amd import Engine
from fastq_dupaway_amd._lib import SEQ_HAMMING

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    with Engine(segments=1) as e:
        yield e


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def spans(seqs):
    """One byte array holding seq + '\\n' per record; (data, offsets, lengths without the '\\n') on the device."""
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    offs = np.zeros(len(seqs), np.uint64)
    offs[1:] = np.cumsum(lens[:-1].astype(np.uint64) + 1)
    data = np.frombuffer(b"".join(s + b"\n" for s in seqs) + b"\0" * 16, dtype=np.uint8).copy()
    return dev(data), dev(offs), dev(lens)


def device_order(e, mates):
    """The mates' descriptors and the device's sorted order of the records (tuples of 1 or 2 mates)."""
    n = len(mates)
    t = [(*spans([m[k] for m in mates]), n) for k in range(len(mates[0]))]
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    e.sort_seqs(t[0], perm, t[1] if len(t) > 1 else None)
    return t, perm


def host_u32(t, n):
    return t.cpu().numpy().view(np.uint32)[:n]


def walk(e, layout, d, what):
    mates = hw.shuffled(layout)
    n = len(mates)
    t, perm = device_order(e, mates)
    p = host_u32(perm, n)
    assert list(p) == ref.sorted_order(mates), what
    head = torch.empty(n, dtype=torch.uint8, device="cuda")
    got = e.seq_heads(t[0], perm, SEQ_HAMMING, d, head, t[1] if len(t) > 1 else None)
    exp = ref.heads(ref.HAMMING, d, [mates[i] for i in p])
    assert exp == hw.flags(layout), what                     # the layout's own claim, as on the host
    flags = head.cpu().numpy().tolist()
    if flags != exp:
        at = next(k for k in range(n) if flags[k] != exp[k])
        print(f"{what}: first difference at sorted place {at} (lane {at % 64}): got {flags[at]}, want {exp[at]}")
    assert flags == exp, what
    assert got == sum(exp), what


@pytest.mark.parametrize("d", hw.DISTANCES)
def test_clusters_on_every_lane_edge(eng, d):
    """Cluster sizes 1, 2, 63, 64, 65, 127, 128, 129 and 200 in twelve orders, behind 0, 1, 62 and 63 single records, with
    n = 0, 1 and 63 (mod 64); in every cluster members at d, heads at d + 1, neighbours at 2d and at 2d + 1, and a head
    that is within d of the first head but not of the one it is measured from."""
    for name, layout in hw.main_lists(d):
        walk(eng, layout, d, (d, name))


@pytest.mark.parametrize("d", (0, 1))
def test_reads_shorter_than_a_word(eng, d):
    for n_mod in hw.N_MODS:
        walk(eng, hw.short_list(d, n_mod, seed=40 + n_mod), d, (d, "short", n_mod))


@pytest.mark.parametrize("d", (1, 2, 5))
def test_drift_is_measured_from_the_head(eng, d):
    walk(eng, hw.drift_list(d), d, (d, "drift"))


@pytest.mark.parametrize("d", hw.DISTANCES)
def test_a_change_of_length_is_a_head(eng, d):
    walk(eng, hw.mixed_length_list(d), d, (d, "mixed_lengths"))


@pytest.mark.parametrize("d", hw.DISTANCES)
def test_pairs_are_held_mate_by_mate(eng, d):
    walk(eng, hw.pair_list(d), d, (d, "pairs"))


@pytest.mark.parametrize("d", hw.LARGE_DISTANCES)
def test_distances_no_read_can_exceed(eng, d):
    """2 * d must saturate, not wrap: with d = 2^31 a wrapped 2d is 0 and every neighbour that differs becomes a cut."""
    for name, layout in hw.large_distance_lists(d):
        walk(eng, layout, d, (d, name))
