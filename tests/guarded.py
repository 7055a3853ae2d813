"""Poisoned, guarded buffers for the tests that hand raw pointers to the library (imported like kernel_paths; works on
CPU tensors too, which is how tests/test_guarded_cpu.py checks the helper itself).

An Arena hands out views inside larger uint8 allocations:

    [ >= G guard bytes | view: exactly the bytes asked for, 256-byte aligned | >= G guard bytes ]

Every byte of the allocation, the view included, starts as 0xFF.  0xFF.. is a NaN in fp32 and in bf16 and -1 in int64: a
legitimate result is never that NaN, and no test here expects an int64 of -1.  So
  * a store that never happens leaves poison in the output            -> assert_written() names the first missing element;
  * a store outside the tensor lands in owned memory and damages a guard -> check() names the buffer and the offset;
  * a stored result that depends on bytes outside an input, or on scratch / workspace contents that were never written,
    turns NaN (0 * NaN is NaN) and fails the test's own comparison with the fp64 reference.
Discarded lanes may read whatever they like; stored ones may not.

G = 196608 bytes (192 KiB), a condition and not a measurement: a multiple of 256, at least 64 KiB, and at least what one
workgroup of the kernels under test can store in one pass, over every store path to guarded memory (outputs AND scratch):
  * weight-gradient slabs (the scratch of unet_conv3x3_bwd / unet_upconv2_bwd): a workgroup of wgrad<3;3;1> (split0,
    split3) and wgradb<3;3;1> owns a 64 x 64 channel tile for ALL taps and writes T x 4096 floats to its slab in one
    contiguous pass (wgrad.hip: slab + (tile * 4 + wave) * T * 1024): 9 x 16 KiB = 147456 B; the Winograd weight gradient
    (wgradw.hip) writes [9 taps][64][64] floats plus 64 bias partials = 147712 B, the largest of all; the 2 x 2 up-conv
    kernels (wgrad<2;2;2>, wgrad_up) write 4 x 16 KiB = 65536 B;
  * output tiles: 256 x 64 and 128 x 128 fp32 elements (igemm<256;64>, igemm<128;128> and their igemmx twins) = 65536 B;
    the same tiles in bf16 (igemmb, igemmb3: 32 KiB), wino32's 64 tiles x 4 outputs x 64 filters (64 KiB) and the
    HBM-bound kernels store no more.
147712 B rounded up with room to spare: a workgroup whose tile, partition or slab index is one too high still lands inside
a guard.  An overrun longer than G bytes (an index off by two slabs, a wild pointer) is out of this helper's reach.

The view's address is 256-byte aligned: the alignment net.hip gives its plan buffers and asks of the workspace.
scratch(n) has exactly n usable bytes (no rounding up, guards also around n == 0), so a *_scratch_bytes export that
returns too little is caught, not covered up.  A zero-size tensor has no data_ptr of its own: pass Arena.ptr(t) to the
library, which is the address inside the guarded allocation for every buffer handed out here."""
import ctypes

import numpy as np
import torch

POISON = 0xFF
ALIGN = 256
G = 196608
CHUNK = 1 << 28


class _Buf:
    __slots__ = ("raw", "start", "nbytes", "label", "shape", "view")


class Arena:
    """One per test.  Keeps every allocation alive until the test ends (raw pointers are in flight)."""

    def __init__(self, device="cuda", guard=G, chunk=CHUNK):
        assert guard % ALIGN == 0 and guard >= G, "the guard is a multiple of 256 bytes and at least G"
        assert chunk > 0
        self.device = torch.device(device)
        self.guard = guard
        self.chunk = chunk          # bytes assert_written looks at in one piece (the result does not depend on it)
        self.bufs = []

    # ---- allocation ----------------------------------------------------------------------------------------------------
    def _alloc(self, shape, dtype, label, kind):
        shape = tuple(int(s) for s in shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
        b = _Buf()
        b.raw = torch.full((self.guard + nbytes + self.guard + ALIGN,), POISON, dtype=torch.uint8, device=self.device)
        b.start = self.guard + (-b.raw.data_ptr()) % ALIGN
        b.nbytes = nbytes
        b.shape = shape
        b.label = label or "%s%d" % (kind, len(self.bufs))
        b.view = b.raw[b.start:b.start + nbytes].view(dtype).view(shape)
        self.bufs.append(b)
        return b

    def out(self, shape, dtype=torch.float32, label=None):
        """A poisoned output tensor of `shape` (contiguous)."""
        if isinstance(shape, int):
            shape = (shape,)
        return self._alloc(shape, dtype, label, "out").view

    def scratch(self, nbytes, label=None):
        """Exactly `nbytes` poisoned bytes (uint8).  For nbytes == 0 hand Arena.ptr(t) to the library."""
        return self._alloc((int(nbytes),), torch.uint8, label, "scratch").view

    def inp(self, tensor, label=None):
        """A guarded copy of `tensor` on the arena's device: what lies next to it is poison."""
        t = tensor.detach().contiguous()
        v = self._alloc(t.shape, t.dtype, label, "inp").view
        v.copy_(t)
        return v

    def _find(self, t):
        for b in self.bufs:
            if b.view is t:
                return b
        raise KeyError("tensor was not handed out by this Arena")

    def address(self, t):
        b = self._find(t)
        return b.raw.data_ptr() + b.start

    def ptr(self, t):
        """void* of a buffer handed out here (None -> NULL); valid for zero-size buffers too."""
        return None if t is None else ctypes.c_void_p(self.address(t))

    # ---- checks --------------------------------------------------------------------------------------------------------
    def check(self):
        """Every guard byte of every buffer handed out is still 0xFF.  One device-side reduction per guard, one host
        read-back for the whole arena; the guards are only copied to the host to word the failure."""
        if not self.bufs:
            return
        ok = None
        for b in self.bufs:
            end = b.start + b.nbytes
            o = (b.raw[:b.start] == POISON).all() & (b.raw[end:] == POISON).all()
            ok = o if ok is None else ok & o
        if bool(ok):
            return
        msgs = []
        for b in self.bufs:
            end = b.start + b.nbytes
            front = (b.raw[:b.start] != POISON).nonzero().flatten().cpu()
            back = (b.raw[end:] != POISON).nonzero().flatten().cpu()
            if len(front):
                msgs.append("guard BEFORE %s %s damaged: %d bytes, first at offset %d (bytes relative to the tensor's start)"
                            % (b.label, b.shape, len(front), int(front[0]) - b.start))
            if len(back):
                msgs.append("guard AFTER %s %s damaged: %d bytes, first at offset %d = %d past its end (%d bytes long)"
                            % (b.label, b.shape, len(back), b.nbytes + int(back[0]), int(back[0]), b.nbytes))
        raise AssertionError("; ".join(msgs))

    def assert_written(self, *tensors):
        """No element of the given buffers (handed out by out()) is still poison.  (Arithmetic on a quiet NaN returns that NaN,
        payload included, so a result computed FROM poison can also show up here rather than in the test's comparison.)"""
        for t in tensors:
            if t is None:
                continue
            b = self._find(t)
            if b.nbytes == 0:
                continue
            es = t.element_size()
            # in pieces of at most self.chunk bytes: the comparison's mask is as large as what it looks at, and a tensor may
            # be gigabytes.  One device-side count per piece, one host read-back for the whole buffer.
            step = max(self.chunk // es, 1) * es

            def left(o):
                return (b.raw[b.start + o:b.start + min(o + step, b.nbytes)].view(-1, es) == POISON).all(dim=1)

            count = torch.zeros((), dtype=torch.int64, device=b.raw.device)
            for o in range(0, b.nbytes, step):
                count += left(o).sum()
            n = int(count)
            if n == 0:
                continue
            first = last = None                       # only to word the failure: element indices of the first and last poison
            for o in range(0, b.nbytes, step):
                idx = left(o).nonzero().flatten()
                if len(idx):
                    first = o // es + int(idx[0]) if first is None else first
                    last = o // es + int(idx[-1])
            first = np.unravel_index(first, b.shape)
            last = np.unravel_index(last, b.shape)
            names = "(n, h, w, c) = " if len(b.shape) == 4 else "index "
            raise AssertionError("%s %s: %d of %d elements still hold poison (never written, or a NaN that kept the payload of poison "
                                 "that was read); first at %s%s, last at %s"
                                 % (b.label, b.shape, n, b.nbytes // es, names, tuple(int(i) for i in first), tuple(int(i) for i in last)))

    def verify(self, *outputs):
        """assert_written on each requested output (None = not requested), then check()."""
        self.assert_written(*outputs)
        self.check()
