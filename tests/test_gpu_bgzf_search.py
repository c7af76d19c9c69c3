"""fqd_bgzf_deflate_ex(FQD_BGZF_SEARCH) on the GPU: the kernels must write, byte for byte, what the same functions write
when tests/native/bgzf_search_check.cpp runs them thread by thread on the CPU (tests/test_bgzf_search_core.py checks that
to be BGZF which inflates member by member to the input) — whatever the order in which the threads reach the table."""
import gzip
import struct
import time

import numpy as np
import pytest

from bgzf_cases import fastq_text
from bgzf_search_cases import FAST, HIGH, all_cases, harness_bgzf
from test_bgzf_core import EOF_MARK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from fastq_dupaway_amd import Engine
    with Engine(segments=1, device=0) as e:
        yield e


def device_bgzf(eng, data: bytes, k: int, effort) -> bytes:
    import torch
    dev = torch.device("cuda", 0)
    src = torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).to(dev)
    dst = torch.empty(max(1, eng.bgzf_bound(len(data))), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    size = eng.bgzf_deflate(src, len(data), dst, k, effort=effort)
    return dst[:size].cpu().numpy().tobytes()


@pytest.mark.parametrize("name,data,k", list(all_cases()), ids=[c[0] for c in all_cases()])
def test_kernels_write_what_the_cpu_run_of_the_same_logic_writes(eng, tmp_path, name, data, k):
    got = device_bgzf(eng, data, k, "high")
    want = harness_bgzf(data, k, HIGH, tmp_path)
    assert want.endswith(EOF_MARK)
    assert got == want[:-len(EOF_MARK)]
    assert gzip.decompress(got + EOF_MARK) == data


def test_unaligned_source_and_reuse_of_the_engine_across_modes(eng, tmp_path):
    import torch
    data = fastq_text(1500, 21)
    dev = torch.device("cuda", 0)
    buf = torch.frombuffer(bytearray(b"xyz" + data), dtype=torch.uint8).to(dev)
    dst = torch.empty(eng.bgzf_bound(len(data)), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    want = {"fast": harness_bgzf(data, 4, FAST, tmp_path)[:-len(EOF_MARK)], "high": harness_bgzf(data, 4, HIGH, tmp_path)[:-len(EOF_MARK)]}
    assert len(want["high"]) < len(want["fast"])
    for effort in ("high", "fast", "fast", "high", "high"):       # one scratch, laid out differently by the two modes
        size = eng.bgzf_deflate(buf[3:], len(data), dst, 4, effort=effort)
        assert dst[:size].cpu().numpy().tobytes() == want[effort], effort


def test_unknown_effort_is_refused(eng):
    import torch
    dev = torch.device("cuda", 0)
    src = torch.zeros(1000, dtype=torch.uint8, device=dev)
    dst = torch.zeros(2000, dtype=torch.uint8, device=dev)
    with pytest.raises(Exception, match="effort"):
        eng.bgzf_deflate(src, 1000, dst, 4, effort=7)
    with pytest.raises(Exception, match="dst_capacity"):
        eng.bgzf_deflate(src, 1000, dst[:100], 4, effort="high")


def walk(raw):
    rows, at, out = [], 0, 0
    while at < len(raw):
        total = struct.unpack_from("<H", raw, at + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", raw, at + total - 8)
        rows.append((at + 18, total - 26, out, isize, crc)); out += isize
        at += total
    a = np.array(rows, dtype=np.uint64).reshape(-1, 5)
    return [a[:, 0].copy(), a[:, 1].astype(np.uint32), a[:, 2].copy(), a[:, 3].astype(np.uint32), a[:, 4].astype(np.uint32)], out


def test_600_mb_of_fastq_in_high_mode_inflates_to_the_input_here_and_in_gzip(eng):
    """The text of test_gpu_bgzf.test_600_mb_of_fastq_inflates_to_the_input, through the search mode, then back through
    gzip and through the device inflater (one wave per member, 12 288 tokens of scratch per window: many more matches now)."""
    import torch
    dev = torch.device("cuda", 0)
    n, L = 1_900_000, 150
    g = torch.Generator(device=dev); g.manual_seed(5)
    rec = torch.empty((n, 18 + L + 3 + L + 1), dtype=torch.uint8, device=dev)
    ids = torch.arange(n, device=dev, dtype=torch.int64)
    rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
    x = ids.clone()
    for p in range(9):
        rec[:, 10 - p] = (48 + x % 10).to(torch.uint8); x //= 10
    rec[:, 11:18] = torch.tensor(list(b" 1:N:0\n"), dtype=torch.uint8, device=dev)
    rec[:, 18:18 + L] = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (n, L), device=dev, generator=g)]
    rec[:, 18 + L] = 10; rec[:, 19 + L] = ord("+"); rec[:, 20 + L] = 10
    rec[:, 21 + L:21 + 2 * L] = torch.tensor(list(b"FFFFFFFF:,#"), dtype=torch.uint8, device=dev)[torch.randint(0, 11, (n, L), device=dev, generator=g)]
    rec[:, 21 + 2 * L] = 10
    src = rec.reshape(-1)
    nbytes = src.numel()
    dst = torch.empty(eng.bgzf_bound(nbytes), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    fast = eng.bgzf_deflate(src, nbytes, dst, 4)
    eng.bgzf_deflate(src, nbytes, dst, 4, effort="high")           # warm-up (scratch allocation)
    t0 = time.perf_counter()
    size = eng.bgzf_deflate(src, nbytes, dst, 4, effort="high")
    dt = time.perf_counter() - t0
    print(f"\n[bgzf search] {nbytes / 1e6:.0f} MB -> {size / 1e6:.0f} MB ({nbytes / size:.2f}x; fast mode {fast / 1e6:.0f} MB) in {dt * 1e3:.1f} ms = {nbytes / dt / 1e9:.1f} GB/s")
    assert size < fast
    got = dst[:size].cpu().numpy().tobytes()
    want = src.cpu().numpy().tobytes()
    assert gzip.decompress(got + EOF_MARK) == want
    arrs, total = walk(got)
    assert total == nbytes
    t = lambda v: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32)).to(dev)
    text = torch.zeros(total, dtype=torch.uint8, device=dev)
    bad = eng.bgzf_inflate(dst, *[t(v) for v in arrs], len(arrs[0]), text)
    assert bad == 0
    assert torch.equal(text[:total], src)
