"""The per-op kernels on tensors just below 2 GiB, just above 2 GiB and just above 4 GiB, through the C ABI with the default
knobs: size alone moves the dispatch ("the one size rule", csrc/common.hpp), and every case is pinned to the kernel family
it must reach (kernel_paths, with the size-aware staging()).  Data, bounds, samplers and references are tests/large_ref.py's
(proved without a device by tests/test_large_tensors_cpu.py): small integers, so every path computes exactly in every
summation order, and every accepted case is held, bit for bit, to
  * a sampled fp64 reference independent of the library (>= 2^16 pixels, every channel: corners, image boundaries, the pixels
    whose source or destination byte offsets straddle 2^31 and 2^32, random ones; for dw / db the full contraction), and
  * the same call run once per image (tensors far below the limit) for EVERY element; for dw / db the fp64 sum of the
    per-image results.
Every pointer comes from a guarded.Arena: every output element written, every guard intact; refused calls leave outputs and
scratch poison and enqueue nothing.

Size classes (B = 16, NHWC, square; bytes of the larger tensor):
    below 2 GiB   [16,1022,1022,32] <-> [16,1020,1020,32]   2 139 103 232   buffer-descriptor staging, offsets next to INT_MAX
                  [16, 722, 722,64] <-> [16, 720, 720,64]   2 135 327 744   (64 channels: wgradw<1> at its limit)
                  [16,1022,1022,64] <-> [16,1020,1020,64]   2 139 103 232   bf16 tensors (mode 2): convb64, wgradb
    above 2 GiB   [16,1026,1026,32] <-> [16,1024,1024,32]   2 155 880 448   the smaller one is exactly 2^31
    above 4 GiB   [16,1026,1026,64] <-> [16,1024,1024,64]   4 311 760 896   the smaller one is exactly 2^32

The kernels' 32-bit address arithmetic at these shapes, read before the first run (e = element offset, b = byte offset;
"masked" = computed but replaced by LDS_DMA_OOB / the zero page through a select, never dereferenced):

  kernel                 expression                                            extreme at the case's shape            in range because
  igemm<..> buf=1        vo = (a_off + toff + kc) * 4             (b, int)     fwd 1022^2x32: < 2 139 103 232         tensor bytes < 2^31 - 1
    dgrad (pad 2)        same, taps past the last row/column                   dz 1020^2x32: 2 130 739 200 + 261 392  < 2^31 - 1 by 16.4 M; masked anyway
                         same, taps before the first row/column                -(2 x 1020 + 2) x 32 x 4 = -261 376    masked (inb), OOB marker instead
    64 ch, 722 / 720     same                                                  2 135 327 744; dgrad 2 123 366 400 + 369 k   as above
  igemm<..> buf=0,       a_off + toff + kc                        (e, int)     < 1 077 940 224 + 131 200 (1026^2x64)  elements < 2^31 - 1 (launch_igemm checks); the
  igemmx                                                                                                              pointer add is 64-bit; negative ones masked
  igemm epilogue         off = (unsigned)m * DC, + coloff in size_t (e)        16 x 1026^2 x 64 = 1 077 940 224       < 2^32, widened before the pointer add
    scatter (up-conv)    (unsigned)((img DH + 2 oy) DW + 2 ox) * DC            16 x 1026^2 x 32 = 538 970 112         same
  wino32<1>              poff = o * 4                             (b, int)     o < 534 775 808 -> < 2 139 103 232     tensor bytes < 2^31 - 1; o = -1 for every
                                                                                                                      pixel outside (never multiplied)
  wino32<0>              o = imgb + mul24(iy, rowp) + mul24(ix, C) (e, int)    < 1 077 940 224; imgb[1] = one image   elements < 2^31 - 1; rowp = 65 664 < 2^23,
                                                                               more = the whole tensor's count        iy < 2^12 (wino_applicable checks)
  wino32 epilogue        ib = (img0 + wrap) * PH * rowp           (e, int)     <= 16 x 1026^2 x 64 = 1 077 940 224    < 2^31; then unsigned + size_t
  wgrad<3;3;1;split0>,   (size_t)((img XH + xr) XW + xc) * XC     (e)          pixel index < 16 842 816 in int,       widened before the channel multiply: right up
    split3 buf=0, <2;2;2>                                                      x 64 in size_t                         to 2^31 pixels; rows outside -> zero page
  wgrad<..split3> buf=1  ysoff = ((img YH + y) YW) YC * 4         (b, int,     < tensor bytes < 2^31 - 1              scalar offset; the vector part is a column
                         scalar offset), iv = (xc XC + ..) * 4                 iv < one row = 130 816                 offset, range-checked against num_records
  wgrad_up<f32>          xo = ((4 r YW + 2 x) XC) * 4 + x_lane    (b, int)     dy 1022^2x32: < 2 139 103 232          tensor bytes < 2^31 - 1; chunks past the end
                         yo = pix * YC * 4 + y_lane                            x 511^2x64: < 1 069 551 616            are masked (ok)
  wgradw<1>              (base + qy XW XC) * 4                    (b, int)     x 722^2x64: < 2 135 327 744; rows      tensor bytes < 2^31 - 1; masked outside
                                                                               past the last: + 3 x 184 832 masked
  wgradw<0>              base + qy XW XC                          (e, int)     < 1 077 940 224 + 3 x 65 664           elements < 2^31 - 1 (launch_wgradw checks)
  convb64<8;32> (bf16)   q.base + hrel = (((img H + iy0) W + ix0) C) * 2 + ..  (b, int)  x 1022^2x64 bf16: < 2 139 103 232 + 4 halo   tensor bytes < 2^31 - 1 by 8.4 M; pixels
                                                                               rows past the end (523 k)              outside masked per pixel; "negative" bases
                                                                                                                      only on border tiles, exact in int
  wgradb<3;3;1>          off = (((img XH + xr) XW + xc) XC + ..) * 2   (b, int) < 2 139 103 232 + 71 columns (9 k)    tensor bytes < 2^31 - 1; masked outside
  max-pool, bias_grad,   size_t throughout (element, pixel and row offsets; the drop-out     -                                      -
  drop-out, head1x1,     counter is the 64-bit element index / 4); the int values are rows
  head1xk, conv1ch       (B (S - 2) = 16 416), pixels per block and channel groups
No expression that is used leaves its range, so no kernel changed.  What did change is where the refusals happen: the per-op
entry points now apply the size rule before anything is enqueued (they used to pack the filters first), and launch_wgrad's
limit is the rule's 2^31 - 1 elements instead of twice that (the row-walking kernel itself is right up to 2^31 pixels, but
nothing can produce such a tensor: every forward and dgrad refuses it).
Mode 2 (bf16 tensors) at [16,1022,1022,64], the largest class its kernels accept: outputs are kernel_bounds.rne_bf16 of the
exact value, one rounding.

Wall times on the MI355X (each case prints its own as "[large] ... s"; fill, calls, references and comparisons included): the
forwards 0.05 - 0.3 s (1.0 s for the first case of the process), the backwards 0.13 s (below 2 GiB) - 0.9 s (above 2 GiB,
mode 0) - 1.3 s (above 4 GiB), the concat case 0.3 s, the up-convs 0.1 - 0.3 s, the max-pool 1.8 s (its torch reference),
the bias gradient 0.6 - 4 s, drop-out 0.8 s, the heads 0.8 - 1.1 s, conv1ch 0.9 s, the refusals 0.02 s (bf16) and 0.9 s (26 GB
of poison to allocate and look at); the whole module in under half a minute.
"""
import ctypes
import gc
import time

import pytest
import torch

import guarded as gd
import kernel_bounds as kb
import kernel_paths as kp
import large_ref as lg
from gpu_support import hip, math_mode  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

B = 16
GIB = 1 << 30
ADT = {0: torch.float32, 1: torch.float32, 2: torch.bfloat16, 3: torch.float32}
# class -> (input extent H, channels): C = K
CLASSES = {"below2G": (1022, 32), "below2G-64ch": (722, 64), "above2G": (1026, 32), "above4G": (1026, 64),
           "below2G-bf16": (1022, 64)}          # (bf16 tensors, mode 2: 2 139 103 232 bytes, the largest class the bf16 kernels accept)


@pytest.fixture
def mem(hip):
    """The case's arena; its tensors are freed and the allocator's cache emptied before the next case.  Prints the wall time."""
    gc.collect()
    torch.cuda.empty_cache()
    A = gd.Arena()
    t0 = time.time()
    yield A
    torch.cuda.synchronize()
    print("[large] %.1f s" % (time.time() - t0))
    A.bufs.clear()
    gc.collect()
    torch.cuda.empty_cache()


def need(nbytes, what):
    """Fail (not skip) when the device has too little free memory for the case."""
    free, total = torch.cuda.mem_get_info()
    assert free >= nbytes + 2 * GIB, "%s needs %.1f GiB of free device memory (+ 2 GiB for references), %.1f GiB are free of %.1f" % (
        what, nbytes / GIB, free / GIB, total / GIB)


def nbytes(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    return n * torch.empty(0, dtype=dtype).element_size()


def still_poison(t, chunk=1 << 28):
    flat = t.reshape(-1).view(torch.uint8)
    return all(bool((flat[o:o + chunk] == gd.POISON).all()) for o in range(0, flat.numel(), chunk))


def repoison(*ts):
    for t in ts:
        t.view(torch.uint8).fill_(gd.POISON)


def at(mem, t, b, per_image):
    """void* of image b of an arena tensor."""
    return None if t is None else ctypes.c_void_p(mem.address(t) + b * per_image * t.element_size())


def small(mem, shape, amax, seed, label):
    return mem.inp(lg.ints(torch.empty(shape), amax, lg.gen("cpu", seed)), label)


def refused(hip, L, rc, rec_rows, mem, *outs):
    """The call returned an error that names the limit, enqueued nothing and wrote nothing."""
    msg = L.unet_last_error().decode()
    assert rc != 0 and ("2^31 - 1" in msg and str(kp.LIMIT_31BIT) in msg), (rc, msg)
    torch.cuda.synchronize()
    assert rec_rows == [], rec_rows
    for o in outs:
        assert still_poison(o), "a refused call wrote to %s" % mem._find(o).label
    mem.check()
    return msg


def family_check(rec, specs, what):
    fams = rec.main_families(reduces=False)
    assert fams == [kp.family(s) for s in specs], "%s: expected %r, got %r" % (what, specs, rec.tags)
    for s in specs:
        assert rec.reached(s), "%s: expected %r, got %r" % (what, s, rec.tags)


# ---- 3 x 3 convolution ------------------------------------------------------------------------------------------------------
class Conv:
    """One 3 x 3 layer over x1 [B, H1, H1, C1] (padded by pad to H) and, optionally, x2 [B, H, H, C2] (the virtual concat)."""

    def __init__(self, hip, mem, mode, H, K, C1, H1=None, pad=0, C2=0, seed=0):
        self.hip, self.L, self.mem, self.mode = hip, hip.lib(), mem, mode
        self.H, self.K, self.C1, self.H1, self.pad, self.C2 = H, K, C1, H if H1 is None else H1, pad, C2
        self.Ho = H - 2
        self.adt = ADT[mode]
        self.es = 2 if mode == 2 else 4
        self.C = C1 + C2
        self.g = lg.gen("cuda", 100 + seed)
        self.w = small(mem, (K, self.C, 3, 3), lg.WMAX, 1 + seed, "w")
        self.bias = small(mem, (K,), lg.BMAX, 2 + seed, "bias")
        self.what = "mode %d x1 %s pad %d x2 %s K %d" % (mode, (B, self.H1, self.H1, C1), pad, (B, H, H, C2) if C2 else None, K)

    def big(self, shape, label, amax=None, bits=False):
        t = self.mem.out(shape, self.adt, label)
        if bits:
            lg.bits01(t, self.g)
        elif amax is not None:
            lg.ints(t, amax, self.g)
        return t

    def sources(self):
        self.x1 = self.big((B, self.H1, self.H1, self.C1), "x1", lg.XMAX)
        self.x2 = self.big((B, self.H, self.H, self.C2), "x2", lg.XMAX) if self.C2 else None

    def src_bytes(self):
        return [t.numel() * self.es for t in (self.x1, self.x2) if t is not None]

    # ---- forward ----
    def fwd_call(self, Bn, x1, x2, y, sc):
        L, H, H1 = self.L, self.H, self.H1
        return L.unet_conv3x3_fwd(x1, H1, H1, self.C1, self.pad, x2, self.C2, Bn, H, H, self.mem.ptr(self.w), self.mem.ptr(self.bias), self.K, 1, y, sc, self.hip.stream())

    def forward(self):
        hip, L, mem, Ho, K, es = self.hip, self.L, self.mem, self.Ho, self.K, self.es
        y = self.big((B, Ho, Ho, K), "y")
        sc = mem.scratch(L.unet_conv3x3_scratch_bytes(self.C, K), "conv3x3 scratch")
        with kp.record(L) as rec:
            hip.check(self.fwd_call(B, mem.ptr(self.x1), mem.ptr(self.x2), mem.ptr(y), mem.ptr(sc)), "conv3x3_fwd " + self.what)
        mem.verify(y)
        nchs = [self.C1, self.C2] if self.C2 else [self.C1]
        family_check(rec, [kp.conv_spec(self.mode, 1, Ho, K, nchs, kp.taps_leave(self.H1, Ho, 0, self.pad), self.src_bytes())], "fwd " + self.what)
        dst = (B, Ho, Ho)
        srcs = [((B, self.H1, self.H1), self.C1 * es, self.pad)] + ([((B, self.H, self.H), self.C2 * es, 0)] if self.C2 else [])
        pix = lg.sample_pixels(dst, K * es, srcs, 11)
        assert len(pix) >= lg.N_SAMPLES
        ref, A = lg.conv_fwd_ref([(self.x1, self.pad)] + ([(self.x2, 0)] if self.C2 else []), self.w, self.bias, pix, dst)
        assert float(A.max()) <= lg.direct_bound(self.C) and lg.wino_fwd_bound(self.C) < lg.EXACT
        assert float(ref.max()) > 0 and bool((ref == 0).any()), "both sides of the ReLU"
        lg.assert_sampled(y, pix, ref, "fwd " + self.what, post=kb.rne_bf16 if self.mode == 2 else None)
        del ref, A
        # every element: the same call, one image at a time
        one = gd.Arena()
        y1 = one.out((1, Ho, Ho, K), self.adt, "y of one image")
        sc1 = one.scratch(L.unet_conv3x3_scratch_bytes(self.C, K), "conv3x3 scratch (one image)")
        same = True
        for b in range(B):
            repoison(y1)
            hip.check(self.fwd_call(1, at(mem, self.x1, b, self.H1 * self.H1 * self.C1), at(mem, self.x2, b, self.H * self.H * self.C2),
                                    one.ptr(y1), one.ptr(sc1)), "conv3x3_fwd image %d" % b)
            one.verify(y1)
            same = same and lg.same_bits(y1[0], y[b])
            assert same, "fwd %s: image %d of the batch run differs from its single-image run" % (self.what, b)
        return y

    # ---- backward ----
    def bwd_call(self, Bn, p):
        L, H, H1 = self.L, self.H, self.H1
        return L.unet_conv3x3_bwd(p["x1"], H1, H1, self.C1, self.pad, p.get("x2"), self.C2, Bn, H, H, self.mem.ptr(self.w), self.K, p["dz"],
                                  p.get("dx1"), p.get("mask1"), p.get("add1"), p.get("dx2"), p.get("mask2"), p.get("dw"), p.get("db"), p["sc"], self.hip.stream())

    def backward(self):
        hip, L, mem, H, H1, Ho, K, es, C1, C2 = self.hip, self.L, self.mem, self.H, self.H1, self.Ho, self.K, self.es, self.C1, self.C2
        dz = self.big((B, Ho, Ho, K), "dz", lg.DZMAX)
        dx1 = self.big((B, H1, H1, C1), "dx1")
        mask1 = self.big((B, H1, H1, C1), "mask1", bits=True)
        add1 = self.big((B, H1, H1, C1), "add1", lg.AMAX)
        dx2 = self.big((B, H, H, C2), "dx2") if C2 else None
        mask2 = self.big((B, H, H, C2), "mask2", bits=True) if C2 else None
        dw = mem.out((K, self.C, 3, 3), torch.float32, "dw")
        db = mem.out((K,), torch.float32, "db")
        sc = mem.scratch(L.unet_conv3x3_bwd_scratch_bytes(B, H, H, self.C, K), "conv3x3_bwd scratch")
        P = lambda t: mem.ptr(t)                                                                       # noqa: E731
        base = {"x1": P(self.x1), "x2": P(self.x2), "dz": P(dz), "dx1": P(dx1), "mask1": P(mask1), "add1": P(add1), "dx2": P(dx2), "mask2": P(mask2), "sc": P(sc)}
        dzb = dz.numel() * es
        dgrad = [kp.conv_spec(self.mode, 1, H1, C1, [K], kp.taps_leave(Ho, H1, self.pad, 2), [dzb])] + ([kp.conv_spec(self.mode, 1, H, C2, [K], True, [dzb])] if C2 else [])
        wgrad = [kp.wgrad_spec(self.mode, 1, C, K, [t.numel() * es, dzb]) for C, t in ((C1, self.x1), (C2, self.x2)) if t is not None]
        one = gd.Arena()
        o = {"dx1": one.out((1, H1, H1, C1), self.adt, "dx1 of one image"), "dw": one.out((K, self.C, 3, 3), torch.float32, "dw of one image"),
             "db": one.out((K,), torch.float32, "db of one image")}
        if C2:
            o["dx2"] = one.out((1, H, H, C2), self.adt, "dx2 of one image")
        sc1 = one.scratch(L.unet_conv3x3_bwd_scratch_bytes(1, H, H, self.C, K), "conv3x3_bwd scratch (one image)")

        def check_dx(tag):
            for dx, mask, add, c0, Cn, ext, o0 in ((dx1, mask1, add1, 0, C1, H1, self.pad),) + (((dx2, mask2, None, C1, C2, H, 0),) if C2 else ()):
                dst = (B, ext, ext)
                pix = lg.sample_pixels(dst, Cn * es, [((B, Ho, Ho), K * es, 2 - o0)], 12)
                assert len(pix) >= lg.N_SAMPLES
                ref, A = lg.conv_dgrad_ref(dz, self.w, c0, Cn, pix, dst, o0, mask, add)
                assert float(A.max()) <= lg.direct_bound(K)
                lg.assert_sampled(dx, pix, ref, "%s dx (channels %d..) %s" % (tag, c0, self.what), post=kb.rne_bf16 if self.mode == 2 else None)

        def per_image(tag, want):
            sums = {n: torch.zeros(o[n].shape, dtype=torch.float64, device="cuda") for n in ("dw", "db") if n in want}
            for b in range(B):
                repoison(*[o[n] for n in want])
                p = {"x1": at(mem, self.x1, b, H1 * H1 * C1), "x2": at(mem, self.x2, b, H * H * C2), "dz": at(mem, dz, b, Ho * Ho * K),
                     "mask1": at(mem, mask1, b, H1 * H1 * C1), "add1": at(mem, add1, b, H1 * H1 * C1), "mask2": at(mem, mask2, b, H * H * C2), "sc": one.ptr(sc1)}
                p.update({n: one.ptr(o[n]) for n in want})
                hip.check(self.bwd_call(1, p), "conv3x3_bwd image %d" % b)
                one.verify(*[o[n] for n in want])
                assert lg.same_bits(o["dx1"][0], dx1[b]), "%s %s: dx1 of image %d differs from its single-image run" % (tag, self.what, b)
                assert not C2 or lg.same_bits(o["dx2"][0], dx2[b]), "%s %s: dx2 of image %d differs from its single-image run" % (tag, self.what, b)
                for n in sums:
                    sums[n] += o[n].double()
            return sums

        # pass 1: dense dz, the input gradients alone (+ add, ReLU' mask)
        with kp.record(L) as rec:
            hip.check(self.bwd_call(B, base), "conv3x3_bwd (dx) " + self.what)
        mem.verify(dx1, dx2)
        assert still_poison(dw) and still_poison(db)
        family_check(rec, dgrad, "dgrad " + self.what)
        check_dx("dense dz")
        per_image("dense dz", ["dx1"] + (["dx2"] if C2 else []))

        # pass 2: thinned dz (the weight gradient's sums stay exact), every output
        repoison(dx1, *([dx2] if C2 else []))
        lg.ints(dz, lg.DZMAX, self.g)
        n = Ho * Ho
        forced = [0, n - 1, (B - 1) * n, B * n - 1] + lg.straddlers(B * n, K * es)
        for x, ext, pad in ((self.x1, H1, self.pad),) + (((self.x2, H, 0),) if C2 else ()):
            for q in lg.straddlers(B * ext * ext, x.shape[-1] * es):
                forced += lg.readers(q, (B, ext, ext), (B, Ho, Ho), pad)
        nz = lg.thin(dz, self.g, forced)
        with kp.record(L) as rec:
            hip.check(self.bwd_call(B, dict(base, dw=P(dw), db=P(db))), "conv3x3_bwd " + self.what)
        mem.verify(dx1, dx2, dw, db)
        family_check(rec, dgrad + wgrad, "bwd " + self.what)
        assert "bias_grad" not in rec.families, rec                      # db rides on the weight gradient
        check_dx("thin dz")
        ref_w = torch.empty(K, self.C, 3, 3, dtype=torch.float64, device="cuda")
        dabs = dz.view(-1, K).abs().sum(0, dtype=torch.float64)
        for x, pad, c0, Cn in ((self.x1, self.pad, 0, C1),) + (((self.x2, 0, C1, C2),) if C2 else ()):
            rw, Aw, rb, Ab = lg.wgrad_ref(x, pad, dz, nz)
            assert float(Aw.max()) < lg.EXACT and float(Ab.max()) < lg.EXACT and lg.wgradw_bound(lg.XMAX, dabs) < lg.EXACT, (float(Aw.max()), float(Ab.max()))
            ref_w[:, c0:c0 + Cn] = rw
        assert float(ref_w.abs().max()) > 0 and torch.equal(Ab, dabs)
        assert torch.equal(dw.double(), ref_w), "bwd %s: dw differs from the fp64 contraction over the %d non-zero dz pixels" % (self.what, len(nz))
        assert torch.equal(db.double(), rb), "bwd %s: db differs from the fp64 sum" % self.what
        sums = per_image("thin dz", ["dx1", "dw", "db"] + (["dx2"] if C2 else []))
        assert torch.equal(sums["dw"], dw.double()), "bwd %s: dw is not the sum of the per-image weight gradients" % self.what
        assert torch.equal(sums["db"], db.double()), "bwd %s: db is not the sum of the per-image bias gradients" % self.what


FWD_CASES = [(m, c) for c in ("below2G", "above2G", "above4G") for m in (0, 3)] + [(1, "above2G"), (2, "below2G-bf16")]
BWD_CASES = FWD_CASES + [(0, "below2G-64ch"), (3, "below2G-64ch"), (1, "below2G"), (1, "below2G-64ch")]


@pytest.mark.parametrize("mode,cls", FWD_CASES, ids=["mode%d-%s" % c for c in FWD_CASES])
def test_conv3x3_fwd(hip, math_mode, mem, mode, cls):
    """igemm<..;0> buf=1 / wino32<1> below the limit, buf=0 / wino32<0> above it, igemmx in mode 1 - by size alone."""
    math_mode(mode)
    H, C = CLASSES[cls]
    need(nbytes((B, H, H, C), ADT[mode]) * 2.2, "conv3x3_fwd %s" % cls)
    c = Conv(hip, mem, mode, H, C, C)
    c.sources()
    c.forward()


@pytest.mark.parametrize("mode,cls", BWD_CASES, ids=["mode%d-%s" % c for c in BWD_CASES])
def test_conv3x3_bwd(hip, math_mode, mem, mode, cls):
    """The padded dgrad, wgrad<3;3;1;split0> buf=0 at 32 channels, wgradw<1> / wgradw<0> at 64, in mode 1 wgrad<3;3;1;split3>
    buf=1 below the limit (32 and 64 channels) and buf=0 above it, and the bias gradient riding on them; dx with + add and
    the ReLU' mask."""
    math_mode(mode)
    H, C = CLASSES[cls]
    need(nbytes((B, H, H, C), ADT[mode]) * 5.5, "conv3x3_bwd %s" % cls)
    c = Conv(hip, mem, mode, H, C, C, seed=3)
    c.sources()
    c.backward()


def test_conv3x3_concat_one_large_source(hip, math_mode, mem):
    """The virtual concat in mode 3 with only the second source at 2 GiB or more: igemm_source_bytes moves the whole
    two-source launch off buffer staging (wino32<0>), forward and backward."""
    math_mode(3)
    H, H1, pad, C = 1026, 1018, 4, 32
    need(nbytes((B, H, H, C), torch.float32) * 9, "conv3x3 concat")
    c = Conv(hip, mem, 3, H, C, C, H1=H1, pad=pad, C2=C, seed=5)
    c.sources()
    assert kp.fits_buffer(c.src_bytes()[0]) and not kp.fits_buffer(c.src_bytes()[1])
    y = c.forward()
    mem.bufs[:] = [b for b in mem.bufs if b.view is not y]
    del y
    torch.cuda.empty_cache()
    c.backward()


# ---- 2 x 2 up-conv ----------------------------------------------------------------------------------------------------------
class UpConv:
    """One 2 x 2 stride-2 transposed conv x [B, H, H, Ci] -> y [B, 2H, 2H, Co] in fp32 tensors (modes 0 / 1); x is a ReLU output
    (non-negative) and serves as its own ReLU' mask in the backward."""
    Ci, Co = 64, 32

    def __init__(self, hip, mem, mode, H):
        self.hip, self.L, self.mem, self.mode, self.H = hip, hip.lib(), mem, mode, H
        L, Ci, Co = self.L, self.Ci, self.Co
        self.g = lg.gen("cuda", 200 + H)
        self.what = "upconv2 mode %d x %s" % (mode, (B, H, H, Ci))
        self.x = lg.ints(mem.out((B, H, H, Ci), torch.float32, "x"), lg.XMAX, self.g).abs_()
        self.w = small(mem, (Ci, Co, 2, 2), lg.WMAX, 21, "w")
        self.bias = small(mem, (Co,), lg.BMAX, 22, "bias")
        self.sc = mem.scratch(L.unet_upconv2_scratch_bytes(B, H, H, Ci, Co), "upconv2 scratch")
        self.one = gd.Arena()
        self.sc1 = self.one.scratch(L.unet_upconv2_scratch_bytes(1, H, H, Ci, Co), "upconv2 scratch (one image)")
        self.nx, self.ny = H * H * Ci, 4 * H * H * Co
        self.xb, self.yb = B * self.nx * 4, B * self.ny * 4

    def forward(self):
        hip, L, mem, one, H, Ci, Co, x, w, bias = self.hip, self.L, self.mem, self.one, self.H, self.Ci, self.Co, self.x, self.w, self.bias
        y = mem.out((B, 2 * H, 2 * H, Co), torch.float32, "y")
        with kp.record(L) as rec:
            hip.check(L.unet_upconv2_fwd(mem.ptr(x), B, H, H, Ci, mem.ptr(w), mem.ptr(bias), Co, mem.ptr(y), mem.ptr(self.sc), hip.stream()), "upconv2_fwd")
        mem.verify(y)
        family_check(rec, ["igemmx<128;128;0;split3>" if self.mode == 1 else "igemm<128;128;0> buf=%d" % kp.staging(1, [self.xb])], "fwd " + self.what)
        dst = (B, 2 * H, 2 * H)
        pix = lg.sample_pixels(dst, Co * 4, [], 31)
        # the four outputs of every x pixel whose bytes straddle a limit
        extra = [(b * 2 * H + 2 * yy + a) * 2 * H + 2 * xx + c for q in lg.straddlers(B * H * H, Ci * 4) for b, r in [divmod(q, H * H)]
                 for yy, xx in [divmod(r, H)] for a in (0, 1) for c in (0, 1)]
        pix = torch.unique(torch.cat([pix, torch.tensor(extra, dtype=torch.int64)]))
        ref, A = lg.upconv_fwd_ref(x, w, bias, pix, dst)
        assert float(A.max()) < lg.EXACT
        lg.assert_sampled(y, pix, ref, "fwd " + self.what)
        y1 = one.out((1, 2 * H, 2 * H, Co), torch.float32, "y of one image")
        for b in range(B):
            repoison(y1)
            hip.check(L.unet_upconv2_fwd(at(mem, x, b, self.nx), 1, H, H, Ci, mem.ptr(w), mem.ptr(bias), Co, one.ptr(y1), one.ptr(self.sc1), hip.stream()),
                      "upconv2_fwd image %d" % b)
            one.verify(y1)
            assert lg.same_bits(y1[0], y[b]), "fwd %s: image %d differs from its single-image run" % (self.what, b)
        return y

    def bwd_call(self, Bn, x, dy, dx, dw, db, sc):
        return self.L.unet_upconv2_bwd(x, Bn, self.H, self.H, self.Ci, self.mem.ptr(self.w), self.Co, dy, dx, x, dw, db, sc, self.hip.stream())

    def check_dx(self, tag, dy, dx):
        H = self.H
        dsx = (B, H, H)
        px = lg.sample_pixels(dsx, self.Ci * 4, [((B, 2 * H, 2 * H), self.Co * 4, 0)], 32, taps=2, stride=2)
        assert len(px) >= lg.N_SAMPLES
        r, Ad = lg.upconv_dgrad_ref(dy, self.w, px, dsx, mask=self.x)
        assert float(Ad.max()) < lg.EXACT
        lg.assert_sampled(dx, px, r, "%s dx %s" % (tag, self.what))

    def per_image(self, tag, dy, dx, o, all_outputs):
        """The backward image by image into the single-image buffers o = (dx1, dw1, db1): dx bit for bit, and the fp64 sums
        of the per-image dw and db."""
        mem, one = self.mem, self.one
        dx1, dw1, db1 = o
        sw = torch.zeros(dw1.shape, dtype=torch.float64, device="cuda")
        sb = torch.zeros(db1.shape, dtype=torch.float64, device="cuda")
        for b in range(B):
            repoison(dx1, dw1, db1)
            self.hip.check(self.bwd_call(1, at(mem, self.x, b, self.nx), at(mem, dy, b, self.ny), one.ptr(dx1), one.ptr(dw1) if all_outputs else None,
                                         one.ptr(db1) if all_outputs else None, one.ptr(self.sc1)), "upconv2_bwd image %d" % b)
            one.verify(dx1, *([dw1, db1] if all_outputs else []))
            assert lg.same_bits(dx1[0], dx[b]), "%s %s: dx of image %d differs from its single-image run" % (tag, self.what, b)
            if all_outputs:
                sw += dw1.double()
                sb += db1.double()
        return sw, sb

    def backward(self, dy):
        """dy: a buffer of y's shape (the forward's output is reused)."""
        hip, L, mem, one, H, Ci, Co, x = self.hip, self.L, self.mem, self.one, self.H, self.Ci, self.Co, self.x
        dx = mem.out((B, H, H, Ci), torch.float32, "dx")
        dw = mem.out((Ci, Co, 2, 2), torch.float32, "dw")
        db = mem.out((Co,), torch.float32, "db")
        o = (one.out((1, H, H, Ci), torch.float32, "dx of one image"), one.out((Ci, Co, 2, 2), torch.float32, "dw of one image"),
             one.out((Co,), torch.float32, "db of one image"))
        dgrad = "igemmx<256;64;0;split3>" if self.mode == 1 else "igemm<256;64;0> buf=%d" % kp.staging(1, [self.yb])
        wgrad = kp.upconv_wgrad_spec(self.mode, 1, [self.yb, self.xb])
        assert wgrad == ("wgrad_up<f32>" if H == 511 else "wgrad<2;2;2;split%d> buf=0" % (3 if self.mode == 1 else 0))

        # pass 1: dense dy, the input gradient alone
        lg.ints(dy, lg.DZMAX, self.g)
        with kp.record(L) as rec:
            hip.check(self.bwd_call(B, mem.ptr(x), mem.ptr(dy), mem.ptr(dx), None, None, mem.ptr(self.sc)), "upconv2_bwd (dx)")
        mem.verify(dx)
        assert still_poison(dw) and still_poison(db)
        family_check(rec, [dgrad], "dgrad " + self.what)
        self.check_dx("dense dy", dy, dx)
        self.per_image("dense dy", dy, dx, o, False)

        # pass 2: thinned dy (the weight gradient's sums stay exact), every output
        repoison(dx)
        lg.ints(dy, lg.DZMAX, self.g)
        n = 4 * H * H
        forced = [0, n - 1, (B - 1) * n, B * n - 1] + lg.straddlers(B * n, Co * 4)
        for q in lg.straddlers(B * H * H, Ci * 4):
            b, r = divmod(q, H * H)
            yy, xx = divmod(r, H)
            forced.append((b * 2 * H + 2 * yy) * 2 * H + 2 * xx)
        nzy = lg.thin(dy, self.g, forced)
        b_, r_ = nzy // n, nzy % n
        nzx = torch.unique((b_ * H + (r_ // (2 * H)) // 2) * H + (r_ % (2 * H)) // 2)          # the x pixels whose 2 x 2 block of dy is not all zero
        with kp.record(L) as rec:
            hip.check(self.bwd_call(B, mem.ptr(x), mem.ptr(dy), mem.ptr(dx), mem.ptr(dw), mem.ptr(db), mem.ptr(self.sc)), "upconv2_bwd")
        mem.verify(dx, dw, db)
        family_check(rec, [dgrad, wgrad], "bwd " + self.what)
        assert "bias_grad" not in rec.families, rec
        self.check_dx("thin dy", dy, dx)
        rw, Aw, rb, Ab = lg.upconv_wgrad_ref(x, dy, nzx)
        assert float(Aw.max()) < lg.EXACT and float(Ab.max()) < lg.EXACT and float(rw.abs().max()) > 0
        assert torch.equal(Ab, dy.view(-1, Co).abs().sum(0, dtype=torch.float64)), "the contraction saw every non-zero pixel of dy"
        assert torch.equal(dw.double(), rw), "bwd %s: dw differs from the fp64 contraction" % self.what
        assert torch.equal(db.double(), rb), "bwd %s: db differs from the fp64 sum" % self.what
        sw, sb = self.per_image("thin dy", dy, dx, o, True)
        assert torch.equal(sw, dw.double()) and torch.equal(sb, db.double()), "bwd %s: dw / db are not the sums of the per-image gradients" % self.what


UP_CASES = [(0, 513), (1, 513), (0, 511)]


@pytest.mark.parametrize("mode,H", UP_CASES, ids=["mode%d-x%d" % c for c in UP_CASES])
def test_upconv2(hip, math_mode, mem, mode, H):
    """x [16,H,H,64] -> y [16,2H,2H,32]: at H = 513 only y is above 2 GiB, so the forward still stages x through a buffer
    descriptor and scatters past 2^31 bytes, while the backward (dy is a source) reaches wgrad<2;2;2;split*> buf=0 by size;
    at H = 511 y is just below the limit and the pixel-linear wgrad_up<f32> runs."""
    math_mode(mode)
    need(nbytes((B, 2 * H, 2 * H, UpConv.Co), torch.float32) * 3, "upconv2 H=%d" % H)
    u = UpConv(hip, mem, mode, H)
    y = u.forward()
    u.backward(y)


# ---- HBM-bound kernels on the tensor above 4 GiB ----------------------------------------------------------------------------
def test_maxpool2_above_4GiB(hip, math_mode, mem):
    """unet_maxpool2_fwd / _bwd on [16,1026,1026,64] fp32: a selection, so exact; every element against torch expressions
    (the backward routes dy to the first maximum in row-major window order, masked by max > 0)."""
    math_mode(3)
    L = hip.lib()
    H, C = 1026, 64
    Hp = H // 2
    need(nbytes((B, H, H, C), torch.float32) * 3.5, "maxpool2")
    g = lg.gen("cuda", 300)
    pre = lg.ints(mem.out((B, H, H, C), torch.float32, "pre"), lg.XMAX, g)
    dy = lg.ints(mem.out((B, Hp, Hp, C), torch.float32, "dy"), lg.DZMAX, g)
    y = mem.out((B, Hp, Hp, C), torch.float32, "y")
    dpre = mem.out((B, H, H, C), torch.float32, "dpre")
    with kp.record(L) as rec:
        hip.check(L.unet_maxpool2_fwd(mem.ptr(pre), mem.ptr(y), B, H, H, C, hip.stream()), "maxpool2_fwd")
        hip.check(L.unet_maxpool2_bwd(mem.ptr(pre), mem.ptr(dy), mem.ptr(dpre), B, H, H, C, hip.stream()), "maxpool2_bwd")
    mem.verify(y, dpre)
    assert rec.families == ["maxpool2_fwd", "maxpool2_bwd"], rec
    win = pre.view(B, Hp, 2, Hp, 2, C)
    assert torch.equal(y, win.amax((2, 4))), "maxpool2_fwd"
    v = [win[:, :, a, :, c] for a in (0, 1) for c in (0, 1)]
    m, mi = v[0], torch.zeros_like(y, dtype=torch.int8)
    for i in (1, 2, 3):
        up = v[i] > m
        m = torch.where(up, v[i], m)
        mi = torch.where(up, torch.full_like(mi, i), mi)
    gv = torch.where(m > 0, dy, torch.zeros_like(dy))
    dwin = dpre.view(B, Hp, 2, Hp, 2, C)
    for i in range(4):
        assert torch.equal(dwin[:, :, i // 2, :, i % 2], torch.where(mi == i, gv, torch.zeros_like(gv))), "maxpool2_bwd, window position %d" % i


def test_bias_grad_alone_above_4GiB(hip, math_mode, mem):
    """unet_conv3x3_bwd with only db on dz [16,1024,1024,64] fp32 (exactly 2^32 bytes): the stand-alone bias_grad.  dz in
    {-1, 0, 1}, so that the sum of 16.8 M terms stays below 2^24 (asserted from the data)."""
    math_mode(3)
    L = hip.lib()
    H, C = 1026, 64
    Ho = H - 2
    need(nbytes((B, H, H, C), torch.float32) * 2.2, "bias_grad")
    x = mem.out((B, H, H, C), torch.float32, "x (never read)")
    dz = lg.ints(mem.out((B, Ho, Ho, C), torch.float32, "dz"), 1, lg.gen("cuda", 400))
    assert dz.numel() * 4 == 1 << 32
    w = small(mem, (C, C, 3, 3), lg.WMAX, 41, "w")
    db = mem.out((C,), torch.float32, "db")
    sc = mem.scratch(L.unet_conv3x3_bwd_scratch_bytes(B, H, H, C, C), "conv3x3_bwd scratch")
    with kp.record(L) as rec:
        hip.check(L.unet_conv3x3_bwd(mem.ptr(x), H, H, C, 0, None, 0, B, H, H, mem.ptr(w), C, mem.ptr(dz), None, None, None, None, None, None,
                                     mem.ptr(db), mem.ptr(sc), hip.stream()), "conv3x3_bwd (db alone)")
    mem.verify(db)
    assert rec.families == ["bias_grad"], rec
    flat = dz.view(-1, C)
    assert float(flat.abs().sum(0, dtype=torch.float64).max()) < lg.EXACT
    assert torch.equal(db.double(), flat.sum(0, dtype=torch.float64)), "bias_grad over 2^32 bytes"
    assert still_poison(x)


def test_dropout_above_4GiB(hip, math_mode, mem):
    """unet_dropout_pool_fwd / unet_dropout_bwd on [16,1026,1026,64] fp32 with p = 1/2 (the scale 2 is exact).  The keep flags
    are tests/philox_ref.py's at sampled runs of elements - the first and last of the tensor, the ones on both sides of byte
    2^31 and 2^32, random ones - and there also the library's own unet_dropout_mask, which then stands for every element:
    x = keep ? 2 x0 : 0, pooled = the 2 x 2 maxima of that.  The backward doubles n = numel - 1 elements (its tail path) and
    leaves the last one alone."""
    import numpy as np
    import philox_ref as ph
    math_mode(3)
    L = hip.lib()
    H, C, p, seed, step, site = 1026, 64, 0.5, 0x1234567887654321, (5 << 32) | 7, 0
    Hp = H // 2
    need(nbytes((B, H, H, C), torch.float32) * 6, "dropout")
    x0 = lg.ints(mem.out((B, H, H, C), torch.float32, "x0"), lg.XMAX, lg.gen("cuda", 500))
    x = mem.out((B, H, H, C), torch.float32, "x (in place)")
    x.copy_(x0)
    n = x.numel()
    pooled = mem.out((B, Hp, Hp, C), torch.float32, "pooled")
    keep = mem.out((n,), torch.uint8, "keep flags")
    with kp.record(L) as rec:
        hip.check(L.unet_dropout_pool_fwd(mem.ptr(x), mem.ptr(pooled), B, H, H, C, p, seed, step, site, hip.stream()), "dropout_pool_fwd")
        hip.check(L.unet_dropout_mask(seed, step, site, 0, n, p, mem.ptr(keep), hip.stream()), "dropout_mask")
    mem.verify(pooled, keep)
    assert rec.families == ["dropout_pool_fwd", "dropout_mask"], rec
    run = 64
    firsts = [0, n - run, (1 << 29) - run // 2, (1 << 30) - run // 2] + [int(v) for v in torch.randint(0, n - run, (16,), generator=torch.Generator().manual_seed(6))]
    flat, flat0 = x.view(-1), x0.view(-1)
    for f in firsts:
        want = ph.keep_flags(seed, step, site, f, run, p)
        assert np.array_equal(keep[f:f + run].cpu().numpy(), want), "keep flags of elements %d.. differ from Philox4x32-10" % f
        ref = np.where(want != 0, 2.0 * flat0[f:f + run].cpu().numpy(), 0.0)
        assert np.array_equal(flat[f:f + run].cpu().numpy(), ref), "dropped values of elements %d.. differ" % f
    frac = float(keep.sum(dtype=torch.float64)) / n
    assert abs(frac - 0.5) < 1e-3, frac
    assert torch.equal(x, torch.where(keep.view(x.shape) != 0, x0 * 2, torch.zeros_like(x0))), "dropout_pool_fwd: x"
    assert torch.equal(pooled, x.view(B, Hp, 2, Hp, 2, C).amax((2, 4))), "dropout_pool_fwd: pooled"
    g = mem.out((B, H, H, C), torch.float32, "g (in place)")
    g.copy_(x0)
    with kp.record(L) as rec:
        hip.check(L.unet_dropout_bwd(mem.ptr(g), n - 1, p, hip.stream()), "dropout_bwd")
    assert rec.families == ["dropout_bwd"], rec
    mem.check()
    assert torch.equal(g.view(-1)[:n - 1], flat0[:n - 1] * 2) and torch.equal(g.view(-1)[n - 1:], flat0[n - 1:]), "dropout_bwd"


@pytest.mark.parametrize("K", [2, 3], ids=["head1x1", "head1xk-K3"])
def test_head_above_4GiB(hip, math_mode, mem, K):
    """unet_head1x1_fwd / _bwd (K = 2) and unet_head1xk_fwd / _bwd (K = 3) on x [16,1026,1026,64] fp32.  Integer data: the
    logits and dz equal torch's own fp32 products in every element; dw / db come from a thinned dlogits (their sums over 16.8 M
    pixels stay below 2^24, asserted from the data) and equal the fp64 contraction over its non-zero pixels."""
    math_mode(3)
    L = hip.lib()
    H, C = 1026, 64
    HW = H * H
    need(nbytes((B, H, H, C), torch.float32) * 5, "head")
    g = lg.gen("cuda", 600 + K)
    x = lg.ints(mem.out((B, H, H, C), torch.float32, "x"), lg.XMAX, g)
    w = small(mem, (K, C), lg.WMAX, 61, "w")
    bias = small(mem, (K,), lg.BMAX, 62, "bias")
    logits = mem.out((B, K, H, H), torch.float32, "logits")
    name = "head1x1" if K == 2 else "head1xk"
    kk = () if K == 2 else (K,)
    with kp.record(L) as rec:
        hip.check(getattr(L, "unet_%s_fwd" % name)(mem.ptr(x), B, H, H, C, *kk, mem.ptr(w), mem.ptr(bias), mem.ptr(logits), hip.stream()), name + "_fwd")
    mem.verify(logits)
    assert rec.families == [name + "_fwd"], rec
    xf = x.view(-1, C)
    ref = (xf @ w.t() + bias).view(B, HW, K).permute(0, 2, 1)
    assert float(xf.abs().sum(1).max()) * lg.WMAX + lg.BMAX < lg.EXACT
    assert torch.equal(logits.view(B, K, HW), ref), name + "_fwd: logits"
    # strategic pixels once more in fp64 by 64-bit index (torch's matmul is the every-element reference, this one checks it)
    pix = torch.tensor(sorted(set(lg.corners(B, H, H) + lg.straddlers(B * HW, C * 4))))
    r64 = lg.rows(x, pix) @ w.double().t() + bias.double()
    got = logits.view(B, K, HW).permute(0, 2, 1).reshape(-1, K)[pix.cuda()].double()
    assert torch.equal(got, r64), name + "_fwd: logits at the strategic pixels"
    del ref, got

    dl = lg.ints(mem.out((B, K, H, H), torch.float32, "dlogits"), lg.DZMAX, g)
    dz = mem.out((B, H, H, C), torch.float32, "dz")
    dw = mem.out((K, C), torch.float32, "dw")
    db = mem.out((K,), torch.float32, "db")
    scratch_bytes = L.unet_head1x1_bwd_scratch_bytes(B, H, H, C) if K == 2 else L.unet_head1xk_bwd_scratch_bytes(B, H, H, C, K)
    sc = mem.scratch(scratch_bytes, name + "_bwd scratch")

    def call(want):
        with kp.record(L) as rec:
            hip.check(getattr(L, "unet_%s_bwd" % name)(mem.ptr(x), B, H, H, C, *kk, mem.ptr(w), mem.ptr(dl), mem.ptr(dz), mem.ptr(dw) if want else None,
                                                      mem.ptr(db) if want else None, mem.ptr(sc), hip.stream()), name + "_bwd")
        mem.verify(dz, *([dw, db] if want else []))
        assert rec.families == [name + "_bwd"], rec
        D = dl.view(B, K, HW).permute(0, 2, 1).reshape(-1, K)
        assert torch.equal(dz.view(-1, C), torch.where(xf > 0, D @ w, torch.zeros_like(xf))), name + "_bwd: dz"
        return D

    call(False)                                                    # dense dlogits: dz alone
    assert still_poison(dw) and still_poison(db)
    repoison(dz)
    lg.ints(dl, lg.DZMAX, g)
    forced = [0, HW - 1, (B - 1) * HW, B * HW - 1] + lg.straddlers(B * HW, C * 4)
    keep = torch.rand(B * HW, generator=g, device="cuda") < lg.DENSITY
    keep[torch.tensor(forced).cuda()] = True
    dl.view(B, K, HW).mul_(keep.view(B, 1, HW))
    dl.view(B, K, HW).permute(0, 2, 1)[(keep & (dl.view(B, K, HW) == 0).all(1).view(-1)).view(B, HW)] = 1.0      # a kept pixel is not all zero
    dl.add_(0.0)                                                   # (-0 -> +0)
    D = call(True)
    nz = keep.nonzero().flatten()
    d = D[nz].double()
    xr = lg.rows(x, nz)
    assert torch.equal(d.abs().sum(0), dl.view(B, K, HW).abs().sum((0, 2), dtype=torch.float64)), "the contraction saw every non-zero pixel"
    assert float((d.abs().t() @ xr.abs()).max()) < lg.EXACT and float(d.abs().sum(0).max()) < lg.EXACT
    assert bool((d[torch.searchsorted(nz, torch.tensor(forced).cuda())] != 0).any(1).all())
    assert torch.equal(dw.double(), d.t() @ xr), name + "_bwd: dw"
    assert torch.equal(db.double(), d.sum(0)), name + "_bwd: db"


def test_conv1ch_above_4GiB(hip, math_mode, mem):
    """unet_conv1ch_fwd / _dgrad / _bwd with B = 16, S = 1028, K = 64: y and dz [16,1026,1026,64] are the 4.3 GB tensor.  Integer
    data; the forward and the input gradient equal torch's fp32 expressions image by image in every element, the weight and
    bias gradient (thinned dz) the fp64 contraction over its non-zero pixels."""
    math_mode(3)
    L = hip.lib()
    S, K = 1028, 64
    So = S - 2
    need(nbytes((B, So, So, K), torch.float32) * 2.5, "conv1ch")
    g = lg.gen("cuda", 700)
    x = lg.ints(mem.out((B, S, S), torch.float32, "x"), lg.XMAX, g)
    w = small(mem, (K, 3, 3), lg.WMAX, 71, "w")
    bias = small(mem, (K,), lg.BMAX, 72, "bias")
    y = mem.out((B, So, So, K), torch.float32, "y")
    with kp.record(L) as rec:
        hip.check(L.unet_conv1ch_fwd(mem.ptr(x), B, S, mem.ptr(w), mem.ptr(bias), K, mem.ptr(y), hip.stream()), "conv1ch_fwd")
    mem.verify(y)
    assert rec.families == ["conv1ch_fwd"], rec
    w9 = w.view(K, 9).t().contiguous()                             # [9, K]
    for b in range(B):
        patches = x[b].unfold(0, 3, 1).unfold(1, 3, 1).reshape(So * So, 9)
        assert torch.equal(y[b].view(-1, K), torch.relu(patches @ w9 + bias)), "conv1ch_fwd: image %d" % b
    pix = lg.sample_pixels((B, So, So), K * 4, [], 71, n=1 << 12)
    ref, A = lg.conv_fwd_ref([(x.view(B, S, S, 1), 0)], w.view(K, 1, 3, 3), bias, pix, (B, So, So))
    assert float(A.max()) < lg.EXACT
    lg.assert_sampled(y, pix, ref, "conv1ch_fwd (fp64, 64-bit gather)")

    dz = y                                                          # y's buffer becomes dz
    lg.ints(dz, lg.DZMAX, g)
    dx = mem.out((B, S, S), torch.float32, "dx")
    with kp.record(L) as rec:
        hip.check(L.unet_conv1ch_dgrad(mem.ptr(dz), B, S, K, mem.ptr(w), mem.ptr(dx), hip.stream()), "conv1ch_dgrad")
    mem.verify(dx)
    assert rec.families == ["conv1ch_dgrad"], rec
    for b in range(B):
        t = (dz[b].view(-1, K) @ w.view(K, 9)).view(So, So, 3, 3)
        r = torch.zeros(S, S, device="cuda")
        for ty in range(3):
            for tx in range(3):
                r[ty:ty + So, tx:tx + So] += t[:, :, ty, tx]
        assert torch.equal(dx[b], r), "conv1ch_dgrad: image %d" % b
    px = lg.sample_pixels((B, S, S), 4, [((B, So, So), K * 4, 2)], 72, n=1 << 12)
    ref, A = lg.conv_dgrad_ref(dz, w.view(K, 1, 3, 3), 0, 1, px, (B, S, S), 0)
    assert float(A.max()) < lg.EXACT
    lg.assert_sampled(dx.view(B, S, S, 1), px, ref, "conv1ch_dgrad (fp64, 64-bit gather)")

    lg.ints(dz, lg.DZMAX, g)
    n = So * So
    nz = lg.thin(dz, g, [0, n - 1, (B - 1) * n, B * n - 1] + lg.straddlers(B * n, K * 4))
    dw = mem.out((K, 3, 3), torch.float32, "dw")
    db = mem.out((K,), torch.float32, "db")
    sc = mem.scratch(L.unet_conv1ch_bwd_scratch_bytes(B, S, K), "conv1ch_bwd scratch")
    with kp.record(L) as rec:
        hip.check(L.unet_conv1ch_bwd(mem.ptr(x), B, S, K, mem.ptr(dz), mem.ptr(dw), mem.ptr(db), mem.ptr(sc), hip.stream()), "conv1ch_bwd")
    mem.verify(dw, db)
    assert rec.families == ["conv1ch_wgrad"], rec
    rw, Aw, rb, Ab = lg.wgrad_ref(x.view(B, S, S, 1), 0, dz, nz)
    assert float(Aw.max()) < lg.EXACT and float(Ab.max()) < lg.EXACT and float(rw.abs().max()) > 0
    assert torch.equal(Ab, dz.view(-1, K).abs().sum(0, dtype=torch.float64)), "the contraction saw every non-zero pixel of dz"
    assert torch.equal(dw.double(), rw.view(K, 3, 3)), "conv1ch_bwd: dw"
    assert torch.equal(db.double(), rb), "conv1ch_bwd: db"


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def refusal_buffers(mem, L, H, C, adt):
    Ho = H - 2
    x = mem.out((B, H, H, C), adt, "x")
    y = mem.out((B, Ho, Ho, C), adt, "y / dz")
    dx = mem.out((B, H, H, C), adt, "dx")
    w = small(mem, (C, C, 3, 3), lg.WMAX, 51, "w")
    bias = small(mem, (C,), lg.BMAX, 52, "bias")
    dw = mem.out((C, C, 3, 3), torch.float32, "dw")
    db = mem.out((C,), torch.float32, "db")
    scf = mem.scratch(L.unet_conv3x3_scratch_bytes(C, C), "conv3x3 scratch")
    scb = mem.scratch(L.unet_conv3x3_bwd_scratch_bytes(B, H, H, C, C), "conv3x3_bwd scratch")
    return x, y, dx, w, bias, dw, db, scf, scb


def test_bf16_tensor_above_2GiB_is_refused(hip, math_mode, mem):
    """[16,1026,1026,64] bf16 is 2 155 880 448 bytes: the bf16 kernels stage through buffer descriptors only, so forward and
    backward refuse it - before anything is enqueued (buffers allocated at full size: a missing check could not fault)."""
    math_mode(2)
    L = hip.lib()
    H, C = 1026, 64
    need(nbytes((B, H, H, C), torch.bfloat16) * 3.2, "bf16 refusal")
    x, y, dx, w, bias, dw, db, scf, scb = refusal_buffers(mem, L, H, C, torch.bfloat16)
    assert x.numel() < kp.LIMIT_31BIT and not kp.fits_buffer(x.numel() * 2)
    with kp.record(L) as rec:
        rc = L.unet_conv3x3_fwd(mem.ptr(x), H, H, C, 0, None, 0, B, H, H, mem.ptr(w), mem.ptr(bias), C, 1, mem.ptr(y), mem.ptr(scf), hip.stream())
    msg = refused(hip, L, rc, rec.rows, mem, y, scf)
    assert "conv3x3_fwd" in msg and "bytes" in msg, msg
    for want_dx, want_dw in ((True, True), (True, False), (False, True)):
        with kp.record(L) as rec:
            rc = L.unet_conv3x3_bwd(mem.ptr(x), H, H, C, 0, None, 0, B, H, H, mem.ptr(w), C, mem.ptr(y), mem.ptr(dx) if want_dx else None, None, None, None, None,
                                    mem.ptr(dw) if want_dw else None, mem.ptr(db), mem.ptr(scb), hip.stream())
        msg = refused(hip, L, rc, rec.rows, mem, dx, dw, db, scb)
        assert "conv3x3_bwd" in msg and "bytes" in msg, msg


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_element_limit_is_refused(hip, math_mode, mem, mode):
    """[16,1450,1450,64] fp32 has 2 152 960 000 elements, more than 2^31 - 1: forward, backward with dx, and backward with dw
    alone (the weight gradient's own limit was twice the rule's; it is the rule's now) refuse it before anything is enqueued."""
    math_mode(mode)
    L = hip.lib()
    H, C = 1450, 64
    need(nbytes((B, H, H, C), torch.float32) * 3.2, "element limit")
    x, y, dx, w, bias, dw, db, scf, scb = refusal_buffers(mem, L, H, C, torch.float32)
    assert x.numel() == 2152960000 and x.numel() > kp.LIMIT_31BIT > y.numel()
    with kp.record(L) as rec:
        rc = L.unet_conv3x3_fwd(mem.ptr(x), H, H, C, 0, None, 0, B, H, H, mem.ptr(w), mem.ptr(bias), C, 1, mem.ptr(y), mem.ptr(scf), hip.stream())
    msg = refused(hip, L, rc, rec.rows, mem, y, scf)
    assert "conv3x3_fwd" in msg and "elements" in msg, msg
    for want_dx, want_dw in ((True, True), (True, False), (False, True)):
        with kp.record(L) as rec:
            rc = L.unet_conv3x3_bwd(mem.ptr(x), H, H, C, 0, None, 0, B, H, H, mem.ptr(w), C, mem.ptr(y), mem.ptr(dx) if want_dx else None, None, None, None, None,
                                    mem.ptr(dw) if want_dw else None, mem.ptr(db) if want_dw else None, mem.ptr(scb), hip.stream())
        msg = refused(hip, L, rc, rec.rows, mem, dx, dw, db, scb)
        assert "conv3x3_bwd" in msg and "elements" in msg, msg
