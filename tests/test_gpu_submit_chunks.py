"""The two-stream sub-batch pipeline of submit_impl (csrc/fqd_engine.hip): on the atomic path a batch of at least
2 * FQD_CHUNK_READS reads is encoded on a second stream in sub-batches while the sub-batch before is inserted.  With the
default of 8 Mi reads no other test reaches it; here FQD_CHUNK_READS=1000 and FQD_BULK_MIN=-1 (no bulk path), both read
when the engine is created.  Reference: first occurrence over the read bytes (tests/bulk_placement.py)."""
import numpy as np
import pytest
import torch

from fastq_dupaway_amd import Engine, Reads
from fastq_dupaway_amd._lib import FqdError
import bulk_placement as bp

pytestmark = pytest.mark.gpu
CHUNK = 1000
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(autouse=True)
def small_sub_batches(monkeypatch):
    monkeypatch.setenv("FQD_CHUNK_READS", str(CHUNK))
    monkeypatch.setenv("FQD_BULK_MIN", "-1")


def make_reads(rng, n, S, ragged, distinct):
    """n records over `distinct` keys, (n, 36) byte rows per mate; ragged: lengths 30..36 (a key's own), else 36."""
    W = 36
    src = [ACGT[rng.integers(0, 4, size=(distinct, W))] for _ in range(S)]
    src_len = [rng.integers(30, W + 1, distinct).astype(np.uint32) if ragged else np.full(distinct, W, np.uint32) for _ in range(S)]
    for m in range(S):
        src[m][np.arange(W)[None, :] >= src_len[m][:, None]] = 0
    pick = rng.integers(0, distinct, n)
    return [src[m][pick] for m in range(S)], [src_len[m][pick] for m in range(S)]


def key_rows(mates, lens):
    cols = []
    for rows, ln in zip(mates, lens):
        cols += [rows, ln.astype("<u4").view(np.uint8).reshape(-1, 4)]
    return np.concatenate(cols, axis=1)


def descriptors(mates, lens, a, b, ragged, device):
    out, W = [], mates[0].shape[1]
    for rows, ln in zip(mates, lens):
        flat = np.concatenate([rows[a:b].reshape(-1), np.zeros(64, np.uint8)])
        offs = np.arange(b - a, dtype=np.uint64) * np.uint64(W) if ragged else None
        l = np.ascontiguousarray(ln[a:b]) if ragged else None
        if device:
            flat = torch.from_numpy(flat).cuda()
            offs = None if offs is None else torch.from_numpy(offs.view(np.int64)).cuda()
            l = None if l is None else torch.from_numpy(l.view(np.int32)).cuda()
        out.append(Reads(flat, offs, l, 0 if ragged else W, 0 if ragged else W))
    return out


def submit(e, segs, n, device):
    if not device:
        return e.submit(segs, n)
    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    e.submit(segs, n, keep=keep)
    e.sync()
    return keep.cpu().numpy()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("S", [1, 2], ids=["se", "pe"])
@pytest.mark.parametrize("n", [1999, 2000, 2001, 5500])
def test_sub_batches(n, S, ragged, device):
    """1999 reads: one encode and one insert launch.  From 2000 on: ceil(n / 1000) of each, the last sub-batch short (2001:
    one read).  A second submit to the same engine reuses the event list and finds the first submit's keys."""
    rng = np.random.default_rng(n * 8 + S * 4 + ragged * 2 + device)
    n2 = 2500
    mates, lens = make_reads(rng, n + n2, S, ragged, distinct=(n + n2) // 2)
    ref = bp.FirstOccurrence(key_rows(mates, lens))
    dup = np.flatnonzero(ref.keep == 0)
    if n >= 2 * CHUNK:          # copies whose first occurrence lies in an earlier sub-batch of the same submit
        assert np.any((dup < n) & (ref.first[dup] // CHUNK < dup // CHUNK))
    assert np.any((dup >= n) & (ref.first[dup] < n)) and np.any((dup >= n) & (ref.first[dup] >= n))
    got = []
    with Engine(segments=S, profile=True) as e:
        for a, b in ((0, n), (n, n + n2)):
            before = e.profile()
            got.append(submit(e, descriptors(mates, lens, a, b, ragged, device), b - a, device))
            after = e.profile()
            launches = 1 if b - a < 2 * CHUNK else -(-(b - a) // CHUNK)
            assert after["insert_launches"] - before["insert_launches"] == launches
            assert after["encode_launches"] - before["encode_launches"] == launches
            assert after["insert_reads"] - before["insert_reads"] == b - a == after["encode_reads"] - before["encode_reads"]
            assert after["partition_launches"] == 0 and after["dedup_launches"] == 0
        e.sync()
        assert e.stats()["duplicates"] == ref.duplicates and e.stats()["records"] == n + n2
    keep = np.concatenate(got)
    wrong = np.flatnonzero(keep != ref.keep)
    assert len(wrong) == 0, f"{len(wrong)} flags differ from first occurrence, first at {wrong[:8].tolist()}"


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("S", [1, 2], ids=["se", "pe"])
@pytest.mark.parametrize("n", [2001, 5500])
def test_first_unknown_base_in_input_order(n, S, ragged, device):
    """An unknown base in sub-batch 3 and one in sub-batch 1, whose encoders run one after the other on the second stream:
    the one reported is the first in input order."""
    rng = np.random.default_rng(n + S)
    mates, lens = make_reads(rng, n, S, ragged, distinct=n)
    late, early = (2000, 0, 3) if n == 2001 else (2345, S - 1, 17), (678, S - 1, 29)
    mates[late[1]][late[0], late[2]] = ord("x")
    mates[early[1]][early[0], early[2]] = ord("n")
    assert late[0] // CHUNK == 2 and early[0] // CHUNK == 0 and late[2] < 30
    with Engine(segments=S) as e:
        with pytest.raises(FqdError) as err:
            submit(e, descriptors(mates, lens, 0, n, ragged, device), n, device)
        assert err.value.code == 3
        assert e.bad_base() == (early[0], early[1], early[2], ord("n"))
