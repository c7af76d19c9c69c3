"""The guarded arena (tests/guarded_arena.py) on the CPU: a torch-made "kernel" that writes one byte behind an output, one
before it, alters an input, or writes far from any buffer is flagged, with the right buffer named; one that writes only
its outputs passes.  Placement: every view at its element's alignment and no more, 4096 pattern bytes between views."""
import numpy as np
import pytest
import torch

from guarded_arena import GUARD, WINDOW, Arena, to_torch_bits


def make(fill=0xFF):
    a = Arena("cpu", 1 << 16, fill)
    src = a.take("src", np.uint8, 100, "in")
    idx = a.take("idx", np.uint32, 33, "in")
    out = a.take("out", np.uint64, 33, "out")
    acc = a.take("acc", np.uint32, 7, "inout")
    src.copy_(torch.arange(100, dtype=torch.uint8))
    idx.copy_(to_torch_bits(np.arange(33, dtype=np.uint32) * 3))
    acc.zero_()
    a.seal()
    return a, src, idx, out, acc


def good_kernel(src, idx, out, acc):
    out.copy_(src[idx.long()].to(torch.int64) * 1000)
    acc += 5


def test_views_are_aligned_to_their_element_and_no_more():
    a, src, idx, out, acc = make()
    assert src.data_ptr() % 16 == 1 and idx.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 8 and acc.data_ptr() % 16 == 4
    views = sorted(a.views, key=lambda v: v.off)
    assert views[0].off >= GUARD and views[-1].end + GUARD <= a.nbytes
    for u, v in zip(views[:-1], views[1:]):
        assert v.off - u.end >= GUARD
    assert (src.dtype, idx.dtype, out.dtype) == (torch.uint8, torch.int32, torch.int64)
    assert out.numel() == 33 and a.view_of(out).nbytes == 264


@pytest.mark.parametrize("fill", [0xFF, b"\n"])
def test_a_call_that_writes_only_its_outputs_passes(fill):
    a, src, idx, out, acc = make(fill)
    assert int(a.mem[0]) == (0xFF if fill == 0xFF else 10)
    good_kernel(src, idx, out, acc)
    a.check()
    assert out[32].item() == 96000 and acc[6].item() == 5


def flagged(a):
    with pytest.raises(AssertionError) as ei:
        a.check()
    return str(ei.value)


def test_one_byte_behind_an_output_is_flagged():
    a, src, idx, out, acc = make()
    good_kernel(src, idx, out, acc)
    a.mem[a.view_of(out).end] = 0
    msg = flagged(a)
    assert "0 byte(s) BEHIND the end of out buffer 'out'" in msg and "from 0xff to 0x00" in msg and "1 byte(s) changed" in msg


def test_one_byte_before_an_output_is_flagged():
    a, src, idx, out, acc = make()
    good_kernel(src, idx, out, acc)
    a.mem[a.view_of(acc).off - 1] = 7
    msg = flagged(a)
    assert "1 byte(s) BEFORE inout buffer 'acc'" in msg and "to 0x07" in msg


def test_an_altered_input_is_flagged():
    a, src, idx, out, acc = make()
    good_kernel(src, idx, out, acc)
    idx[5] += 1
    msg = flagged(a)
    assert "INSIDE in buffer 'idx' at byte 20 (element 5)" in msg and "from 0x0f to 0x10" in msg


def test_a_write_far_from_any_buffer_is_flagged():
    a, src, idx, out, acc = make()
    good_kernel(src, idx, out, acc)
    last = max(a.views, key=lambda v: v.off)
    far = last.end + 3 * GUARD + 17
    assert far < a.nbytes
    a.mem[far] = 1
    msg = flagged(a)
    assert f"arena byte {far} changed" in msg and f"{3 * GUARD + 17} byte(s) BEHIND the end of {last.role} buffer '{last.name}'" in msg


def test_a_byte_rewritten_with_its_own_value_is_no_damage_and_the_fill_is_the_callers():
    a, src, idx, out, acc = make(b"\n")
    a.mem[a.view_of(out).end] = 10
    a.check()
    a.mem[a.view_of(out).end] = 0xFF
    assert "from 0x0a to 0xff" in flagged(a)


def test_windowed_arena_checks_around_its_buffers_and_resets():
    a = Arena("cpu", 1 << 20, 0xFF, windowed=True)
    at = (1 << 19) - 50 + 1                                  # straddles the middle, odd address
    t = a.take("text", np.uint8, 100, "in", at=at)
    o = a.take("sizes", np.uint32, 10, "out", at=at + 100 + GUARD + 3 - (at + 100 + GUARD + 3) % 4)
    t.fill_(65)
    a.seal()
    assert sum(b - lo for lo, b, _ in a.snap) <= 2 * WINDOW + 2 * GUARD + 200
    o.fill_(3)
    a.check()
    a.mem[at + 100] = 0
    assert "0 byte(s) BEHIND the end of in buffer 'text'" in flagged(a)
    a.mem[at - WINDOW // 2] = 0
    assert f"{WINDOW // 2} byte(s) BEFORE in buffer 'text'" in flagged(a)
    a.reset(b"\n")
    assert not a.views and int(a.mem[at]) == 10 and int(a.mem[at - WINDOW // 2]) == 10 and int(a.mem[0]) == 0xFF
    with pytest.raises(AssertionError):
        a.take("x", np.uint8, 10, "in", at=5)               # no room for the guard in front
