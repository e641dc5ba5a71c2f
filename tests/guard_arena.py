"""Guarded buffers for the tests of caller-owned workspaces, packed weights and windowed outputs.

torch.empty rounds every allocation up (512 B at least, 2 MiB blocks for large ones) and mostly returns zeroed memory, so a kernel
that writes a little past its workspace, reads a pad row nobody wrote, or depends on what the last call left behind stays green on
buffers that come from it.  A GuardArena is one flat byte tensor `guard | payload | guard`:

  * the payload has exactly the requested number of elements, starts at an address the caller chooses (`align`, `phase`: address %
    align == phase; 256-byte aligned by default) and is pre-filled with a 32-bit word pattern the caller chooses;
  * each guard is at least 1 MiB and at least as large as the payload, filled with GUARD_WORD (a NaN with a payload as float32 and
    as float64, -3824671 as int32: nothing a kernel computes);
  * view(shape) aliases the payload (pass it as workspace=, out=, dx_nhwc= ... or through dptr);
  * check(what) synchronises and asserts that both guards still hold their fill bit for bit; a failure names the first and the last
    touched 32-bit word relative to the payload (negative: before it; >= the payload's words: behind it).

ChannelWindow is the same for an output with a channel window (out_cstride / out_coff): the whole wide tensor is sentinel, and
check() also asserts that every channel outside [coff, coff + C) still holds the sentinel bit for bit.

A plain module (no fixtures, no hooks): works on CPU tensors as well, which is how tests/test_guard_arena_host.py checks it.
"""
import numpy as np
import torch

GUARD_WORD = 0xFFC5A3E1      # guards
SENTINEL_WORD = 0xFFD2B4A7   # outputs before the call: a NaN, so an unwritten or accumulated-into output element is not finite
NAN_WORD = 0xFFFFFFFF
INF_WORD = 0x7F800000
ZERO_WORD = 0x00000000
MIN_GUARD_BYTES = 1 << 20


def _pattern_bytes(word, nbytes, device):
    """nbytes bytes of the little-endian 32-bit `word`, repeated from byte 0"""
    four = torch.tensor([(int(word) >> (8 * i)) & 0xFF for i in range(4)], dtype=torch.uint8)
    return four.repeat((nbytes + 3) // 4)[:nbytes].to(device)


class GuardArena(object):
    def __init__(self, numel, dtype=torch.float32, device="cuda:0", fill=NAN_WORD, align=256, phase=0, guard_bytes=MIN_GUARD_BYTES):
        esize = torch.empty((), dtype=dtype).element_size()
        if numel < 0 or align < 1 or not 0 <= phase < align or phase % esize:
            raise ValueError("GuardArena: numel >= 0, 0 <= phase < align, phase a multiple of the element size; got {} {} {} {}".format(
                numel, dtype, align, phase))
        self.dtype, self.numel, self.nbytes = dtype, int(numel), int(numel) * esize
        self.guard_bytes = max(int(guard_bytes), MIN_GUARD_BYTES, self.nbytes)
        self.flat = torch.empty((2 * self.guard_bytes + self.nbytes + 2 * align + esize,), dtype=torch.uint8, device=device)
        base = self.flat.data_ptr()
        start = base + self.guard_bytes
        start += (phase - start) % align
        self.begin = start - base                       # byte offset of the payload inside flat
        self.end = self.begin + self.nbytes
        self.flat[:self.begin] = _pattern_bytes(GUARD_WORD, self.begin, device)
        self.flat[self.end:] = _pattern_bytes(GUARD_WORD, self.flat.numel() - self.end, device)
        self._front, self._back = self.flat[:self.begin].clone(), self.flat[self.end:].clone()
        self.fill(fill)

    # ---- payload
    def payload_bytes(self):
        return self.flat[self.begin:self.end]

    def fill(self, word):
        """payload <- the 32-bit `word` repeated"""
        self.payload_bytes().copy_(_pattern_bytes(word, self.nbytes, self.flat.device))
        return self

    def fill_from(self, other):
        """payload <- the bytes of tensor `other` (e.g. the workspace another call left behind), repeated / cut to this size"""
        src = other.contiguous().reshape(-1).view(torch.uint8)
        if self.nbytes and src.numel():
            self.payload_bytes().copy_(src.repeat((self.nbytes + src.numel() - 1) // src.numel())[:self.nbytes])
        return self

    def view(self, shape=None):
        """a tensor of the arena's dtype aliasing the payload (flat when no shape is given)"""
        t = self.payload_bytes().view(self.dtype)
        assert t.numel() == self.numel and (self.numel == 0 or t.data_ptr() == self.flat.data_ptr() + self.begin)
        return t if shape is None else t.view(shape)

    def address(self):
        return self.flat.data_ptr() + self.begin

    # ---- guards
    def _touched(self, now, ref, origin):
        """first and last changed 32-bit word of one guard, relative to the payload's first word (`origin`: the guard's byte offset
        relative to the payload)"""
        idx = torch.nonzero(now != ref).reshape(-1)
        if idx.numel() == 0:
            return None
        lo, hi = int(idx[0]) + origin, int(idx[-1]) + origin
        return lo // 4, hi // 4, int(idx.numel())

    def check(self, what=""):
        if self.flat.is_cuda:
            torch.cuda.synchronize(self.flat.device)
        front = self._touched(self.flat[:self.begin], self._front, -self.begin)
        back = self._touched(self.flat[self.end:], self._back, self.nbytes)
        msgs = []
        if front:
            msgs.append("before the payload: words {} .. {} ({} bytes changed)".format(*front))
        if back:
            msgs.append("behind the payload: words {} .. {} ({} bytes changed; the payload has {} words)".format(
                back[0], back[1], back[2], (self.nbytes + 3) // 4))
        assert not msgs, "{}: guard of a {}-byte buffer touched {}".format(what, self.nbytes, "; ".join(msgs))


def workspace(nbytes, min_align, device="cuda:0", fill=NAN_WORD):
    """a feature-kernel workspace of exactly `nbytes` bytes at its documented minimum alignment and no better: the address is min_align
    modulo 2 min_align (8 mod 16 for an 8-byte aligned one).  float64 elements when min_align allows, else int32; NaN bits by default,
    since these workspaces need no initialisation.  -> the GuardArena: pass .view() as workspace=, call .check() after the run"""
    dtype = torch.float64 if min_align % 8 == 0 and nbytes % 8 == 0 else torch.int32
    esize = 8 if dtype == torch.float64 else 4
    if nbytes < 0 or nbytes % esize or min_align % 4:
        raise ValueError("workspace: {} bytes at alignment {} cannot be a whole number of {}-byte elements".format(nbytes, min_align, esize))
    arena = GuardArena(nbytes // esize, dtype=dtype, device=device, fill=fill, align=2 * min_align, phase=min_align)
    assert arena.address() % min_align == 0 and arena.address() % (2 * min_align) != 0
    return arena


class ChannelWindow(object):
    """an output (..., cstride) in a GuardArena, all SENTINEL_WORD, of which a call may write channels [coff, coff + C) only"""

    def __init__(self, shape, coff, C, device="cuda:0", dtype=torch.float32, sentinel=SENTINEL_WORD, **arena_args):
        shape = tuple(int(s) for s in shape)
        if not (0 <= coff and C >= 0 and coff + C <= shape[-1]):
            raise ValueError("ChannelWindow: window [{}, {}) outside {} channels".format(coff, coff + C, shape[-1]))
        self.shape, self.coff, self.C, self.sentinel = shape, int(coff), int(C), sentinel
        self.arena = GuardArena(int(np.prod(shape)), dtype=dtype, device=device, fill=sentinel, **arena_args)
        self.tensor = self.arena.view(shape)

    def inside(self):
        """a copy of the window on the host"""
        return self.tensor[..., self.coff:self.coff + self.C].cpu().numpy().copy()

    def check(self, what=""):
        self.arena.check(what)
        esize = self.tensor.element_size()
        rows = self.arena.payload_bytes().view(-1, self.shape[-1] * esize)
        want = _pattern_bytes(self.sentinel, self.arena.nbytes, rows.device).view(rows.shape)
        bad = rows != want
        bad[:, self.coff * esize:(self.coff + self.C) * esize] = False
        if bool(bad.any()):
            hit = torch.nonzero(bad)
            r, c = int(hit[0, 0]), int(hit[0, 1]) // esize
            raise AssertionError("{}: channel {} of row {} (window [{}, {}) of {}) lost its sentinel; {} bytes outside the window changed".format(
                what, c, r, self.coff, self.coff + self.C, self.shape[-1], int(bad.sum())))


def dense(shape, device="cuda:0", dtype=torch.float32):
    """a dense output in a guard arena, all sentinel: ChannelWindow with the whole row as its window"""
    return ChannelWindow(shape, 0, shape[-1], device=device, dtype=dtype)
