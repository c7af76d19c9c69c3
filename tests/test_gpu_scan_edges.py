"""fqd_count_lines / fqd_scan_records (csrc/fqd_inflate.hip) with newlines on the edges of the kernels' units: a lane's 32
bytes, a workgroup's 8 KiB tile, the parts of 1024 tiles that the tile counts are scanned in, and a text base that is not
16-byte aligned (every lane then reads byte by byte).  The texts are those of tests/scan_edge_cases.py, which
tests/test_edge_inputs.py holds to their claims on the host; the reference is tests/record_reference.py: the positions
of '\\n', K at a time.  Every comparison is exact.

Not reached: above 2^20 tiles (8 GiB of text) launch_tile_offsets gives a part more than 1024 tiles.  A text of that
size is out of reach of a test of seconds, and a smaller one would not take that path, so nothing here stands in for it."""
from functools import lru_cache

import numpy as np
import pytest

import scan_edge_cases as sc
from record_reference import numpy_records

pytestmark = pytest.mark.gpu

DTYPES = ("int64", "int64", "int32", "int32", "int32")


@pytest.fixture(scope="module")
def eng():
    from fastq_dupaway_amd import Engine
    with Engine(segments=1, device=0) as e:
        yield e


@lru_cache(maxsize=None)
def reference(name, k):
    return tuple(a.astype(np.int64) for a in numpy_records(sc.text_of(name, k), k))


def upload(data: bytes, pad: int = 0):
    """The text on the device behind `pad` bytes of something else: pad = 0 is torch's aligned base."""
    import torch
    buf = torch.frombuffer(bytearray(b"\n" * pad + data), dtype=torch.uint8).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return buf[pad:]


def device_records(eng, text, n, k):
    """(line count, well formed, the five arrays on the host) of the n bytes at text."""
    import torch
    lines = eng.count_lines(text, n)
    n_rec = lines // k
    out = [torch.empty(max(n_rec, 1), dtype=getattr(torch, d), device=text.device) for d in DTYPES]
    ok = eng.scan_records(text, n, k, n_rec, *out)
    return lines, ok, [o[:n_rec].cpu().numpy().astype(np.int64) for o in out]


def check(eng, name, k, pad):
    data = sc.text_of(name, k)
    lines, ok, got = device_records(eng, upload(data, pad), len(data), k)
    assert lines == data.count(b"\n"), (name, k, pad)
    assert ok, (name, k, pad)
    for which, (g, want) in enumerate(zip(got, reference(name, k))):
        assert np.array_equal(g, want), (name, k, pad, which)


@pytest.mark.parametrize("name,k", sc.ids(sc.SMALL))
def test_small_texts_aligned(eng, name, k):
    check(eng, name, k, 0)


@pytest.mark.parametrize("name,k", sc.ids(sc.SMALL))
def test_small_texts_behind_1_7_and_15_bytes(eng, name, k):
    """The pad bytes are newlines: a lane that read from the buffer's base instead of the text's would count them."""
    for pad in (1, 7, 15):
        check(eng, name, k, pad)


@pytest.mark.parametrize("name,k", sc.ids(sc.PARTS))
def test_texts_of_1024_1025_and_2049_tiles(eng, name, k):
    check(eng, name, k, 0)


@pytest.mark.parametrize("name,k", sc.ids(sc.PARTS))
def test_texts_of_1024_1025_and_2049_tiles_behind_7_bytes(eng, name, k):
    check(eng, name, k, 7)


@pytest.mark.parametrize("name,data", list(sc.line_count_cases()), ids=[c[0] for c in sc.line_count_cases()])
def test_line_counts_of_text_that_is_not_records(eng, name, data):
    for pad in (0, 1):
        assert eng.count_lines(upload(data, pad), len(data)) == data.count(b"\n"), (name, pad)


@pytest.mark.parametrize("kind", sc.DAMAGE)
def test_damage_in_a_text_of_two_parts_is_reported(eng, kind):
    data = sc.damaged(kind)
    lines, ok, _ = device_records(eng, upload(data), len(data), 4)
    assert lines == data.count(b"\n")
    assert not ok
