"""One block of memory that holds every buffer of a call, so that what the call does AROUND its buffers is seen.

An Arena owns one uint8 tensor pre-filled with a pattern.  take() hands out views of it, back to back, each at an address
aligned to its element size and to nothing more (uint8 at 1 mod 16, uint32 at 4 mod 16, uint64 at 8 mod 16) with at least
GUARD bytes of the pattern before and after.  seal() copies the arena once the inputs are written; check(), after the call
and a synchronise, holds every byte that is not part of an `out` / `inout` view against that copy: guards, the bytes far from
any buffer, and the `in` views, since a const input comes back bit for bit.  The guards only space the buffers: a store
anywhere in the arena is found.

A windowed arena (the 4.5 GiB one whose buffers straddle or lie beyond byte 2^32) copies and checks WINDOW bytes either side
of every buffer instead of all of it; its buffers are placed by the caller (take(..., at=offset)) and reset() makes it ready
for the next case.  Works on device="cpu" as well (tests/test_guarded_arena.py)."""
import numpy as np
import torch

GUARD = 4096
WINDOW = 65536
ROLES = ("in", "out", "inout")
TORCH_OF = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16, np.dtype(np.uint32): torch.int32,
            np.dtype(np.uint64): torch.int64, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}


def to_torch_bits(a):
    """A numpy array as a torch tensor of the same bits (torch has no arithmetic on unsigned 32 / 64 bit)."""
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a)


class View:
    def __init__(self, name, dtype, count, role, off, tensor):
        self.name, self.dtype, self.count, self.role, self.off, self.t = name, np.dtype(dtype), count, role, off, tensor
        self.nbytes = count * self.dtype.itemsize

    @property
    def end(self):
        return self.off + self.nbytes


class Arena:
    def __init__(self, device, nbytes, fill, windowed=False):
        self.fill = fill[0] if isinstance(fill, (bytes, bytearray)) else int(fill)
        self.mem = torch.full((nbytes,), self.fill, dtype=torch.uint8, device=device)
        self.base = self.mem.data_ptr()
        assert self.base % 16 == 0, "the allocator's own block is expected to be 16-byte aligned"
        self.nbytes, self.windowed = nbytes, windowed
        self.views, self.cursor, self.snap = [], 0, None

    # ---- placement ---------------------------------------------------------------------------------------------------------------
    def take(self, name, dtype, count, role, at=None):
        """A view of `count` elements of `dtype` (numpy) as a torch tensor of the same width.  at: the byte offset to place it
        at (windowed arenas; it must keep GUARD bytes to every other view and the element's alignment)."""
        assert role in ROLES, role
        assert self.snap is None, "take() after seal()"
        dt = np.dtype(dtype)
        size = dt.itemsize
        if at is None:
            off = self.cursor + GUARD
            want = size % 16                       # the residue mod 16 that is a multiple of `size` and of nothing larger
            off += (want - (self.base + off)) % 16
        else:
            off = at
            assert (self.base + off) % size == 0, (name, off)
            for v in self.views:
                assert off >= v.end + GUARD or off + count * size + GUARD <= v.off, (name, "too close to", v.name)
        assert off >= GUARD and off + count * size + GUARD <= self.nbytes, f"arena of {self.nbytes} bytes is too small for {name}"
        t = self.mem[off:off + count * size].view(TORCH_OF[dt])
        assert t.data_ptr() == self.base + off
        assert at is not None or size >= 16 or t.data_ptr() % 16 == size, (name, t.data_ptr() % 16)
        v = View(name, dt, count, role, off, t)
        self.views.append(v)
        self.cursor = max(self.cursor, v.end)
        return t

    def view_of(self, tensor):
        return next(v for v in self.views if v.t is tensor)

    # ---- snapshot and check ------------------------------------------------------------------------------------------------------
    def regions(self):
        if not self.windowed:
            return [(0, self.nbytes)]
        spans = sorted((max(0, v.off - WINDOW), min(self.nbytes, v.end + WINDOW)) for v in self.views)
        merged = []
        for a, b in spans:
            if merged and a <= merged[-1][1]:
                merged[-1] = (merged[-1][0], max(merged[-1][1], b))
            else:
                merged.append((a, b))
        return merged

    def seal(self):
        self.snap = [(a, b, self.mem[a:b].clone()) for a, b in self.regions()]

    def check(self):
        """Every byte outside the out / inout views equals the snapshot; raises AssertionError naming the nearest buffer, the
        side, the first damaged offset and the value found."""
        assert self.snap is not None, "check() before seal()"
        for a, b, snap in self.snap:
            bad = self.mem[a:b] != snap
            for v in self.views:
                if v.role != "in" and v.nbytes and v.off < b and v.end > a:
                    bad[max(v.off, a) - a:min(v.end, b) - a] = False
            if not bool(bad.any()):
                continue
            at = a + int(torch.nonzero(bad)[0])
            raise AssertionError(self.describe(at, int(self.mem[at]), int(snap[at - a]), int(bad.sum())))

    def describe(self, at, got, was, n_bad):
        def gap(v):
            return v.off - at if at < v.off else at - (v.end - 1) if at >= v.end else 0
        if not self.views:
            return f"arena byte {at} changed from 0x{was:02x} to 0x{got:02x} ({n_bad} bytes changed in all); no buffer was taken"
        v = min(self.views, key=gap)
        if at < v.off:
            where = f"{v.off - at} byte(s) BEFORE {v.role} buffer '{v.name}'"
        elif at >= v.end:
            where = f"{at - v.end} byte(s) BEHIND the end of {v.role} buffer '{v.name}' ({v.count} x {v.dtype})"
        else:
            where = f"INSIDE {v.role} buffer '{v.name}' at byte {at - v.off} (element {(at - v.off) // v.dtype.itemsize})"
        return f"arena byte {at} changed from 0x{was:02x} to 0x{got:02x}: {where}; {n_bad} byte(s) changed in all"

    def reset(self, fill=None):
        """Forget the views; their windows (or all of a small arena) get the pattern again."""
        if fill is not None:
            self.fill = fill[0] if isinstance(fill, (bytes, bytearray)) else int(fill)
        for a, b in self.regions():
            self.mem[a:b] = self.fill
        self.views, self.cursor, self.snap = [], 0, None
