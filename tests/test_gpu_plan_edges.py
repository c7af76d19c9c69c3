"""fqd_output_offsets / fqd_output_plan / fqd_copy_spans (csrc/fqd_join.hip) at the edges of their units and with 64-bit
sums: entry counts around a lane's 8 entries, a tile of 2048, the 64 tiles of the tile scan's first wave (131 072
entries) and the 1024 tiles of its first round (2 097 152 entries); sizes over the whole uint32 range, so that every
partial sum must be held in 64 bits; and a copy whose destination offsets lie above 2^33.  Inputs and the numpy
reference (cumsum in uint64) are tests/plan_edge_cases.py; every comparison is exact."""
import numpy as np
import pytest
import torch

import plan_edge_cases as pc
from fastq_dupaway_amd import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    with Engine(segments=1, device=0) as e:
        yield e


def to_dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(x, want):
    """A bare assert on two arrays of two million entries makes pytest format them: compare first, show the first place."""
    got = x.cpu().numpy().view(want.dtype)
    if np.array_equal(got, want):
        return True
    at = int(np.flatnonzero(got != want)[0])
    print(f"first difference at {at}: got {got[at]}, want {want[at]}")
    return False


@pytest.mark.parametrize("size_kind", pc.SIZES)
@pytest.mark.parametrize("n", pc.NS)
def test_plan_and_offsets_equal_numpy_cumsum(eng, n, size_kind):
    i64 = dict(dtype=torch.int64, device="cuda")
    for keep_kind in pc.keeps_for(n):
        case = pc.make(n, keep_kind, size_kind)
        what = (n, size_kind, keep_kind)
        d_keep, d_idx, d_starts, d_sizes = (to_dev(case[k]) for k in ("keep", "idx", "starts", "sizes"))
        for use_idx in (True, False):
            src, ln, dst = torch.full((n,), -7, **i64), torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n,), -7, **i64)
            torch.cuda.synchronize()
            total = eng.output_plan(d_keep, d_idx if use_idx else None, n, d_starts, d_sizes, src, ln, dst)
            w_src, w_len, w_dst, w_total = pc.plan_reference(case, use_idx)
            assert total == w_total, (what, use_idx)
            assert same(src, w_src), (what, use_idx, "src_off")
            assert same(ln, w_len), (what, use_idx, "len")
            assert same(dst, w_dst), (what, use_idx, "dst_off")
        dest = torch.full((case["n_rec"],), -1, **i64)
        torch.cuda.synchronize()
        total = eng.output_offsets(d_keep, d_idx, n, d_sizes, dest)
        w_dest, w_total = pc.offsets_reference(case)
        assert total == w_total, what
        assert same(dest, w_dest), (what, "dest")


def test_copy_spans_to_destinations_above_2_to_the_33(eng):
    """The writer's biased window: every dst_off carries 2^33 and the destination base is 2^33 below the window."""
    case = pc.span_case()
    n = case["n"]
    d_keep, d_idx, d_starts, d_sizes, d_text = (to_dev(case[k]) for k in ("keep", "idx", "starts", "sizes", "text"))
    src, dst = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
    ln = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    total = eng.output_plan(d_keep, d_idx, n, d_starts, d_sizes, src, ln, dst)
    want = pc.span_window(case)
    assert total == len(want)
    assert bool((src % 16 != 0).any()) and bool((src % 2 != 0).any())
    dst += pc.SPAN_BIAS
    window = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.copy_spans(d_text, src, ln, n, window.data_ptr() - pc.SPAN_BIAS, dst)
    eng.sync()
    got = window.cpu().numpy()
    assert np.array_equal(got[:total], want)
    assert not got[total:].any()
