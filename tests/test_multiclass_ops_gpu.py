"""Per-op tests of the K-class kernels of loss.hip (unet_softmax_ce_step, unet_argmaxk, unet_eval_confusion) and multiclass.hip (unet_head1xk_fwd / _bwd) through
the C ABI against the fp64 references of tests/multiclass_ref.py, at the shapes where the kernels change path: pixel counts
either side of a block's quantum, images smaller than a block's stride, more partials than the finisher has threads, more
pixels than a capped grid has threads, every class padding (KP = 4, 8, 16, full and padded), logits at which expf underflows
and the gradient saturates.  Every pointer handed to the library comes from a guarded.Arena (tests/guarded.py): scratch is
exact to the byte, mem.verify(outputs...) after every call = every element written, every guard intact; an output passed as
NULL has a poisoned buffer beside it that must stay poison.  Inputs, shape lists and bounds are multiclass_ref's, proved
well-posed without a device by tests/test_multiclass_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded as gd
import multiclass_ref as ref
from gpu_support import hip, math_mode, put, still_poison, strided

pytestmark = pytest.mark.gpu


# ---- unet_softmax_ce_step ---------------------------------------------------------------------------------------------------
def ce_weight_forms(w):
    """(name, array handed to the library or None, (wsB, wsH, wsW), the weight the reference sees) from a [B,H,W] map: none,
    dense, [H,W], [B,1,W], a view with column stride 2 (NaN in the columns between), a one-element scalar."""
    B, H, W = w.shape
    wide = np.full((B, H, 2 * W), np.nan, np.float32)
    wide[:, :, ::2] = w
    return [("none", None, (0, 0, 0), None),
            ("dense", w, (H * W, W, 1), w),
            ("[H,W]", w[0], (0, W, 1), w[:1]),
            ("[B,1,W]", w[:, :1], (W, 0, 1), w[:, :1]),
            ("column stride 2", wide, (2 * H * W, 2 * W, 2), w),
            ("scalar", w.reshape(-1)[:1], (0, 0, 0), w.reshape(-1)[:1].reshape(1, 1, 1))]


class CeCall:
    """One unet_softmax_ce_step call on Arena buffers; outputs not asked for are still allocated (and must stay poison)."""

    def __init__(self, hip, x, labels, warr, ws, gs, want_dx=True, want_mask=True, want_invalid=True):
        L = hip.lib()
        B, K, H, W = x.shape
        npix = B * H * W
        self.mem = mem = gd.Arena()
        view, (xsB, xsC, xsH) = strided(mem, x)
        lab = put(mem, labels, "labels")
        wd = None if warr is None else put(mem, warr, "weight")
        self.loss = mem.out((1,), torch.float32, "loss")
        self.dx = mem.out((B, K, H, W), torch.float32, "dlogits")
        self.mask = mem.out((B, H, W), torch.int64, "mask")
        self.invalid = mem.out((1,), torch.int64, "invalid")
        nbytes = L.unet_softmax_ce_scratch_bytes(npix)
        sc = mem.scratch(nbytes, "softmax_ce scratch")
        hip.check(L.unet_softmax_ce_step(view, xsB, xsC, xsH, K, mem.ptr(lab), mem.ptr(wd), ws[0], ws[1], ws[2], B, H, W, mem.ptr(self.loss),
                                         mem.ptr(self.dx) if want_dx else None, gs, mem.ptr(self.mask) if want_mask else None,
                                         mem.ptr(self.invalid) if want_invalid else None, mem.ptr(sc), hip.stream()), "unet_softmax_ce_step")
        torch.cuda.synchronize()
        mem.verify(self.loss, self.dx if want_dx else None, self.mask if want_mask else None, self.invalid if want_invalid else None)
        assert nbytes == -(-npix // 2048) * 16                  # a double and a 64-bit count per 2048-pixel block, no more
        assert want_dx or still_poison(self.dx)
        assert want_mask or still_poison(self.mask)
        assert want_invalid or still_poison(self.invalid)


@pytest.mark.parametrize("family", ref.CE_FAMILIES)
@pytest.mark.parametrize("shape,K", ref.CE_CASES, ids=["%dx%dx%d-K%d" % (s + (K,)) for s, K in ref.CE_CASES])
def test_softmax_ce_step_edge_shapes(hip, shape, K, family):
    """Loss within 1e-6 relative of multiclass_ref.softmax_ce (fp64), dlogits element-wise within softmax_ce_grad_bound,
    exactly 0 on every class plane of a saturated pixel (label = the maximum, every other logit <= m - 104: every other exp
    is 0, the sum is 1 and 1 / 1 - 1 is 0) and of a pixel with an invalid label; loss and dlogits finite; the mask bit-equal
    to the first maximum; the invalid count exact, and with invalid_u64 = NULL everything else bit-identical.  Six weight
    forms per case, grad_scale alternating between 1 and 0.25."""
    B, H, W = shape
    npix = B * H * W
    x, labels, w = ref.ce_cases(B, K, H, W, family)
    labels, nbad = ref.plant_invalid(labels, K)
    assert nbad == (5 if npix >= 16 else 0)
    mask_ref = ref.argmax_first(x)
    sat = ref.saturated_pixels(x, labels)
    assert sat.any() or not (family == "extreme" and npix >= 2047)
    bad = ((labels < 0) | (labels >= K))
    worst_l = worst_g = 0.0
    for k, (name, warr, ws, wref) in enumerate(ce_weight_forms(w)):
        gs = (1.0, 0.25)[k % 2]
        loss_ref, d_ref, _, bad_ref = ref.softmax_ce(x, labels, wref, gs)
        assert bad_ref == nbad
        c = CeCall(hip, x, labels, warr, ws, gs)
        loss, g = c.loss.item(), c.dx.cpu().numpy()
        assert np.isfinite(loss) and np.isfinite(g).all(), name
        el = abs(loss - loss_ref) / abs(loss_ref) if loss_ref else abs(loss)
        bound = ref.softmax_ce_grad_bound(x, wref, K, gs)
        eg = float((np.abs(g - d_ref) / bound).max())
        worst_l, worst_g = max(worst_l, el), max(worst_g, eg)
        print("softmax_ce %s K=%d %s, weight %s: loss rel err %.3g, dlogits err / bound %.3g" % (shape, K, family, name, el, eg))
        assert el <= 1e-6, (name, el)
        assert eg <= 1.0, (name, eg)
        gp = g.transpose(0, 2, 3, 1)                                  # [B,H,W,K]
        assert np.all(gp[sat] == 0.0), name
        assert np.all(gp[bad] == 0.0), name
        assert np.array_equal(c.mask.cpu().numpy(), mask_ref), name
        assert c.invalid.item() == nbad, name
        if k == 1:
            c2 = CeCall(hip, x, labels, warr, ws, gs, want_invalid=False)
            assert torch.equal(c2.loss, c.loss) and torch.equal(c2.dx, c.dx) and torch.equal(c2.mask, c.mask)
    print("softmax_ce %s K=%d %s: worst loss rel err %.3g, worst dlogits err / bound %.3g" % (shape, K, family, worst_l, worst_g))


@pytest.mark.parametrize("shape,K", [((3, 1, 683), 5), ((300, 1, 7), 16), ((5, 3, 17), 9)])
def test_softmax_ce_optional_outputs(hip, shape, K):
    """dlogits = NULL and mask = NULL, separately and together: what is requested is bit-identical to the full call, what is
    passed as NULL stays poison (checked in CeCall)."""
    B, H, W = shape
    x, labels, w = ref.ce_cases(B, K, H, W, "extreme")
    labels, nbad = ref.plant_invalid(labels, K)
    ws = (H * W, W, 1)
    full = CeCall(hip, x, labels, w, ws, 0.25)
    for want_dx, want_mask in ((True, False), (False, True), (False, False)):
        c = CeCall(hip, x, labels, w, ws, 0.25, want_dx=want_dx, want_mask=want_mask)
        assert torch.equal(c.loss, full.loss) and c.invalid.item() == nbad
        assert not want_dx or torch.equal(c.dx, full.dx)
        assert not want_mask or torch.equal(c.mask, full.mask)


# ---- unet_argmaxk -----------------------------------------------------------------------------------------------------------
def tie_logits(rs, shape):
    """Small integers, so ties are common; every zero is +0.0 or -0.0 at random (a tie both ways: the lower class wins)."""
    x = rs.randint(-3, 4, shape).astype(np.float32)
    x[(x == 0) & (rs.rand(*shape) < 0.5)] = -0.0
    return x


ARGMAX_CASES = [(s, K) for s in ((1, 1, 1), (3, 7, 257), (2, 66, 33)) for K in ref.ALL_K] + [((2, 1025, 1024), 3)]


@pytest.mark.parametrize("shape,K", ARGMAX_CASES, ids=["%dx%dx%d-K%d" % (s + (K,)) for s, K in ARGMAX_CASES])
def test_argmaxk_edge_shapes(hip, shape, K):
    """Bit-equal to the first maximum on a strided view inside NaN.  2 x 1025 x 1024 pixels exceed 8192 blocks x 256 lanes:
    the grid-stride loop's second trip."""
    L = hip.lib()
    B, H, W = shape
    assert shape != (2, 1025, 1024) or B * H * W > 8192 * 256
    rs = np.random.RandomState(K * 131 + H)
    x = tie_logits(rs, (B, K, H, W))
    if B * H * W > 1:
        z = np.signbit(x) & (x == 0)
        assert z.any() and ((x == 0) & ~z).any()
    mem = gd.Arena()
    view, (bs, ps, rs_) = strided(mem, x)
    am = mem.out((B, H, W), torch.int64, "argmax")
    hip.check(L.unet_argmaxk(view, bs, ps, rs_, K, mem.ptr(am), B, H, W, hip.stream()), "unet_argmaxk")
    torch.cuda.synchronize()
    mem.verify(am)
    assert np.array_equal(am.cpu().numpy(), ref.argmax_first(x))


# ---- unet_eval_confusion ----------------------------------------------------------------------------------------------------
EVAL_SHAPES = [(1, 1, 0), (2, 60, 4), (3, 255, 1), (2, 257, 0), (1, 300, 3)]       # (B, n, pad)
EVAL_K = (2, 3, 5, 9, 16)
EVAL_CASES = [(s, EVAL_K[(i + j) % 5]) for i, s in enumerate(EVAL_SHAPES) for j in (0, 2)]


@pytest.mark.parametrize("shape,K", EVAL_CASES, ids=["%dx%d+%d-K%d" % (s + (K,)) for s, K in EVAL_CASES])
def test_eval_confusion_edge_shapes(hip, shape, K):
    """mask, conf and invalid exact against argmax_first / confusion; the centre crop of a [B,K,n+2pad,n+2pad] view whose pad
    ring and surroundings are NaN.  n = 257 and 300 exceed the 65 536 threads an image gets: the grid-stride loop and the
    block histogram over a second trip.  At n = 257 every label of image 1 is invalid: conf[1] = 0, invalid[1] = n^2.
    With labels = NULL the mask is identical and conf / invalid, passed or not, are not touched."""
    L = hip.lib()
    B, n, pad = shape
    assert n * n <= 65536 or n in (257, 300)
    rs = np.random.RandomState(K * 17 + n)
    x = tie_logits(rs, (B, K, n, n))
    lab = rs.randint(0, K, (B, n, n)).astype(np.int64)
    if n >= 60:
        lab[B - 1, 5, :4] = [-1, K, 99, -2 ** 40]
    if n == 257:
        lab[1] = rs.choice([-1, K, K + 7, 2 ** 40], (n, n))
    mask_ref = ref.argmax_first(x)
    conf_ref, bad_ref = ref.confusion(mask_ref, lab, K)
    if n == 257:
        assert not conf_ref[1].any() and bad_ref[1] == n * n and conf_ref[0].sum() == n * n
    S = n + 2 * pad
    for labels, give in ((lab, True), (None, False), (None, True)):
        mem = gd.Arena()
        # the [B,K,S,S] logits sit at (1, 2) of a [B,K,S+2,S+4] NaN tensor; their own pad ring is NaN too
        view, (bs, ps, rs_) = strided(mem, x, top=1 + pad, left=2 + pad, bottom=1 + pad, right=2 + pad)
        view = C.c_void_p(view.value - (pad * (S + 4) + pad) * 4)
        ld = None if labels is None else put(mem, labels, "labels")
        mask = mem.out((B, n, n), torch.int64, "mask")
        conf = mem.out((B, K, K), torch.int64, "conf")
        inv = mem.out((B,), torch.int64, "invalid")
        hip.check(L.unet_eval_confusion(view, bs, ps, rs_, pad, K, mem.ptr(ld), mem.ptr(mask), B, n, mem.ptr(conf) if give else None,
                                        mem.ptr(inv) if give else None, hip.stream()), "unet_eval_confusion")
        torch.cuda.synchronize()
        if labels is None:
            mem.verify(mask)
            assert still_poison(conf) and still_poison(inv)
        else:
            mem.verify(mask, conf, inv)
            assert np.array_equal(conf.cpu().numpy(), conf_ref) and np.array_equal(inv.cpu().numpy(), bad_ref)
        assert np.array_equal(mask.cpu().numpy(), mask_ref)


# ---- unet_head1xk_fwd / _bwd ------------------------------------------------------------------------------------------------
# pixel counts either side of the forward block's 256 (C = 64) and 512 (C = 32) pixels and of the backward's 512-pixel chunk
HEAD_SHAPES = {64: [(1, 1, 1), (3, 5, 17), (2, 8, 16), (1, 1, 257), (1, 7, 73), (2, 8, 32), (3, 9, 19)],
               32: [(1, 1, 1), (1, 7, 73), (2, 8, 32), (3, 9, 19), (5, 5, 41)]}
HEAD_K = (3, 4, 5, 8, 9, 16)
HEAD_CASES = [(C_, s, HEAD_K[(i + j) % 6]) for C_ in (64, 32) for i, s in enumerate(HEAD_SHAPES[C_]) for j in (0, 3)]


def head_call(hip, x, w, b, dl, bf16, name="unet_head1xk", K=None):
    """forward + backward on Arena buffers: (y, dz, dw, db, scratch bytes)"""
    L = hip.lib()
    B, H, W, C_ = x.shape
    Kw = w.shape[0]
    mem = gd.Arena()
    xd = mem.inp(x.to(torch.bfloat16) if bf16 else x, "x")
    wd, bd, dld = mem.inp(w, "w"), mem.inp(b, "bias"), mem.inp(dl, "dlogits")
    y = mem.out((B, Kw, H, W), torch.float32, "y")
    dz = mem.out((B, H, W, C_), torch.bfloat16 if bf16 else torch.float32, "dz")
    dw = mem.out((Kw, C_), torch.float32, "dw")
    db = mem.out((Kw,), torch.float32, "db")
    kk = () if K is None else (K,)
    sb = getattr(L, name + "_bwd_scratch_bytes")(B, H, W, C_, *kk)
    sc = mem.scratch(sb, "head bwd scratch")
    hip.check(getattr(L, name + "_fwd")(mem.ptr(xd), B, H, W, C_, *kk, mem.ptr(wd), mem.ptr(bd), mem.ptr(y), hip.stream()), name + "_fwd")
    hip.check(getattr(L, name + "_bwd")(mem.ptr(xd), B, H, W, C_, *kk, mem.ptr(wd), mem.ptr(dld), mem.ptr(dz), mem.ptr(dw), mem.ptr(db),
                                        mem.ptr(sc), hip.stream()), name + "_bwd")
    torch.cuda.synchronize()
    mem.verify(y, dz, dw, db)
    return y, dz, dw, db, sb


def head_inputs(shape, K, C_, bf16):
    B, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(K * 100 + C_ + B * H * W)
    x = torch.randn(B, H, W, C_, generator=g)
    if bf16:
        x = x.to(torch.bfloat16).float()
    return x, torch.randn(K, C_, 1, 1, generator=g) * 0.2, torch.randn(K, generator=g) * 0.1, torch.randn(B, K, H, W, generator=g) * 1e-3


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C_,shape,K", HEAD_CASES, ids=["C%d-%dx%dx%d-K%d" % ((c,) + s + (K,)) for c, s, K in HEAD_CASES])
def test_head1xk_edge_shapes(hip, math_mode, C_, shape, K, dtype):
    """y, dz, dw and db within the bounds of multiclass_ref.head_reference_and_bounds; all four guarded outputs, scratch exact."""
    assert sorted(b * h * w for b, h, w in HEAD_SHAPES[64]) == [1, 255, 256, 257, 511, 512, 513]
    assert sorted(b * h * w for b, h, w in HEAD_SHAPES[32]) == [1, 511, 512, 513, 1025]
    B, H, W = shape
    n = B * H * W
    assert H != W or n == 1
    bf16 = dtype == "bf16"
    math_mode(2 if bf16 else 3)
    x, w, b, dl = head_inputs(shape, K, C_, bf16)
    y, dz, dw, db, sb = head_call(hip, x, w, b, dl, bf16, K=K)
    nb = -(-n // 512)
    assert sb == nb * (K * C_ + K) * 4                       # one partial row of K C + K floats per 512-pixel chunk
    r = ref.head_reference_and_bounds(x, w, b, dl, nb, bf16)
    ey = ((y.permute(0, 2, 3, 1).reshape(n, K).double().cpu() - r["y"]).abs() / r["yb"]).max().item()
    edz = ((dz.float().reshape(n, C_).double().cpu() - r["dz"]).abs() / r["dzb"]).max().item()
    edw = ((dw.double().cpu() - r["dw"]).abs() / r["dwb"]).max().item()
    edb = ((db.double().cpu() - r["db"]).abs() / r["dbb"]).max().item()
    print("head1xk C=%d %s K=%d %s: err / bound y %.3g, dz %.3g, dw %.3g, db %.3g" % (C_, shape, K, dtype, ey, edz, edw, edb))
    assert ey <= 1 and edz <= 1 and edw <= 1 and edb <= 1


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C_", [64, 32])
def test_head1xk_k2_is_head1x1(hip, math_mode, C_, dtype):
    """At K = 2 and 257 pixels the entry points are the head1x1 kernels: bit-identical, the same scratch size."""
    bf16 = dtype == "bf16"
    math_mode(2 if bf16 else 3)
    x, w, b, dl = head_inputs((1, 1, 257), 2, C_, bf16)
    yk, dzk, dwk, dbk, sbk = head_call(hip, x, w, b, dl, bf16, K=2)
    y1, dz1, dw1, db1, sb1 = head_call(hip, x, w, b, dl, bf16, name="unet_head1x1")
    assert sbk == sb1
    assert torch.equal(yk, y1) and torch.equal(dzk, dz1) and torch.equal(dwk, dw1) and torch.equal(dbk, db1)
