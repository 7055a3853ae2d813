"""Per-op tests of the 2-class step-side kernels of loss.hip (bce_logits, bce_step, onehot2, argmax2) and of direct.hip's
sgd_momentum through the C ABI against the fp64 references of tests/step_ref.py: logits large enough for the
log1pf(expf(-|x|)) and ex / (1 + ex) branches, element counts either side of BCE_PER_BLOCK (4096), BCE_PX_PER_BLOCK (2048) and SGD_CHUNK (4096), H != W, every
weight broadcast, strided logits inside NaN.  Every pointer handed to the library comes from a guarded.Arena
(tests/guarded.py); mem.verify(outputs...) after every call = every element written, every guard intact.
Tolerances are those of test_ops_gpu.py::test_step_side_kernels: 1e-5 relative on the loss, 1e-5 normalised on the gradient;
masks and one-hot targets are bit-exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded as gd
import step_ref
from gpu_support import hip, nerr, put, rejected, still_poison, strided

pytestmark = pytest.mark.gpu

SPECIAL = np.float32([0.0, -0.0, 1e-8, -1e-8, 17, -17, 88, -88, 104, -104, 1e4, -1e4])


def logits_and_labels(B, H, W):
    """randn x 3 mixed with SPECIAL on 40 % of the elements, ties planted (equal planes, +0.0 against -0.0 both ways)."""
    rs = np.random.RandomState(B * 1000 + H)
    x = (rs.randn(B, 2, H, W) * 3).astype(np.float32)
    pick = rs.rand(B, 2, H, W) < 0.4
    x[pick] = rs.choice(SPECIAL, int(pick.sum()))
    labels = rs.randint(0, 2, (B, H, W)).astype(np.int64)
    if B * H * W == 1:
        x[0, :, 0, 0] = (104.0, -104.0)
    else:
        f = x.reshape(B, 2, -1)
        f[0, 1, 0] = f[0, 0, 0]
        f[-1, 0, -1] = 0.0; f[-1, 1, -1] = -0.0
        if H * W > 2:
            f[0, 0, 1] = -0.0; f[0, 1, 1] = 0.0
    return x, labels


def weight_forms(B, H, W):
    """(name, array handed to the library, its four element strides, the same weight broadcast to [B,2,H,W])"""
    rs = np.random.RandomState(5)
    full = (rs.rand(B, 2, H, W) + 0.5).astype(np.float32)
    cls = (rs.rand(2, H, W) + 0.5).astype(np.float32)           # the reference's [B,H,W] with B meeting the class axis
    pix = (rs.rand(B, H, W) + 0.5).astype(np.float32)
    one = np.float32([0.75])
    return [("none", None, (0, 0, 0, 0), None),
            ("full", full, (2 * H * W, H * W, W, 1), full),
            ("class-aligned", cls, (0, H * W, W, 1), np.broadcast_to(cls[None], (B, 2, H, W))),
            ("per-pixel", pix, (H * W, 0, W, 1), np.broadcast_to(pix[:, None], (B, 2, H, W))),
            ("scalar", one, (0, 0, 0, 0), np.broadcast_to(one.reshape(1, 1, 1, 1), (B, 2, H, W)))]


# 1, 2047, 2048, 2049 and 3 * 2048 + 5 pixels (bce_step's 2048 per block) = 2, 4094, 4096, 4098 and 3 * 4096 + 10 elements
# (bce_logits' 4096 per block), with H != W; 3 x 683: a block over three images; then 257 blocks of either kernel: the second trip
# of the finisher's 256 threads over the partials (the loop it shares with the soft-max CE and Dice finishers)
SHAPES = [(1, 1, 1), (1, 23, 89), (2, 16, 64), (3, 1, 683), (11, 13, 43), (2, 513, 512)]


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_bce_step_and_bce_logits(hip, B, H, W):
    """fp64 reference: max(x,0) - x z + log1p(exp(-|x|)), weighted mean over all 2 B H W terms; gradient
    w (sigmoid(x) - z) / n * grad_scale.  Loss and gradient are finite for logits up to +-1e4, the gradient is exactly 0 where
    x >= 104 with z = 1 and where x <= -104 with z = 0 (expf(-104) is below the smallest fp32 denormal), and bce_step equals
    onehot2 + bce_logits + argmax2 on the same data: gradient bit-equal, loss within the tolerance."""
    L = hip.lib()
    npix = B * H * W
    assert [b * h * w for b, h, w in SHAPES] == [1, 2047, 2048, 2049, 3 * 2048 + 5, 256 * 2048 + 1024] and (H != W or npix == 1)
    assert -(-SHAPES[-1][0] * 513 * 512 // 2048) == 257 == -(-2 * SHAPES[-1][0] * 513 * 512 // 4096) and 683 < 2048 < 3 * 683
    x, labels = logits_and_labels(B, H, W)
    z = step_ref.onehot2(labels)
    mask_ref = step_ref.argmax2(x)
    assert (mask_ref == 0).any()
    worst_l = worst_g = 0.0
    for k, (name, w, ws, wfull) in enumerate(weight_forms(B, H, W)):
        gs = (1.0, 0.25)[k % 2]
        loss_ref, grad_ref = step_ref.bce(x, z, wfull, gs)
        mem = gd.Arena()
        lab = put(mem, labels, "labels")
        wd = None if w is None else put(mem, w, "weight " + name)
        view, (xsB, xsC, xsH) = strided(mem, x)
        # fused: integer labels, strided logits
        loss = mem.out((1,), torch.float32, "loss"); dx = mem.out((B, 2, H, W), torch.float32, "dlogits")
        mask = mem.out((B, H, W), torch.int64, "mask")
        sc = mem.scratch(L.unet_bce_step_scratch_bytes(npix), "bce_step scratch")
        hip.check(L.unet_bce_step(view, xsB, xsC, xsH, mem.ptr(lab), mem.ptr(wd), ws[0], ws[1], ws[2], ws[3], B, H, W, mem.ptr(loss), mem.ptr(dx), gs,
                                  mem.ptr(mask), mem.ptr(sc), hip.stream()))
        mem.verify(loss, dx, mask)
        g = dx.cpu().numpy()
        assert np.isfinite(loss.item()) and np.isfinite(g).all()
        el, eg = abs(loss.item() - loss_ref) / abs(loss_ref), nerr(g, grad_ref)
        worst_l, worst_g = max(worst_l, el), max(worst_g, eg)
        assert el < 1e-5 and eg < 1e-5, (name, el, eg)
        assert np.array_equal(mask.cpu().numpy(), mask_ref)
        sat = ((x >= 104) & (z == 1)) | ((x <= -104) & (z == 0))
        assert np.all(g[sat] == 0.0) and (npix < 2047 or (((x >= 104) & (z == 1)).any() and ((x <= -104) & (z == 0)).any()))
        # the same from the separate kernels: one-hot target, dense logits
        ll = mem.out((B, 2, H, W), torch.float32, "one-hot")
        hip.check(L.unet_onehot2(mem.ptr(lab), mem.ptr(ll), B, H, W, hip.stream()))
        mem.verify(ll)
        assert np.array_equal(ll.cpu().numpy(), z.astype(np.float32))
        loss2 = mem.out((1,), torch.float32, "loss (bce_logits)"); dx2 = mem.out((B, 2, H, W), torch.float32, "dlogits (bce_logits)")
        sc2 = mem.scratch(L.unet_bce_scratch_bytes(2 * npix), "bce_logits scratch")
        xd = put(mem, x, "logits")
        hip.check(L.unet_bce_logits(mem.ptr(xd), mem.ptr(ll), mem.ptr(wd), ws[0], ws[1], ws[2], ws[3], B, H, W, mem.ptr(loss2), mem.ptr(dx2), gs,
                                    mem.ptr(sc2), hip.stream()))
        mem.verify(loss2, dx2)
        assert abs(loss2.item() - loss_ref) < 1e-5 * abs(loss_ref) and abs(loss2.item() - loss.item()) < 1e-5 * abs(loss_ref)
        assert nerr(dx2.cpu().numpy(), grad_ref) < 1e-5
        assert torch.equal(dx2, dx), name                        # bit-equal
        am = mem.out((B, H, W), torch.int64, "argmax")
        hip.check(L.unet_argmax2(view, xsB, xsC, xsH, mem.ptr(am), B, H, W, hip.stream()))
        mem.verify(am)
        assert torch.equal(am, mask)
    print("bce %dx%dx%d: worst loss err %.3g (relative), worst gradient err %.3g (normalised)" % (B, H, W, worst_l, worst_g))


def test_bce_optional_outputs(hip):
    """dlogits and mask are each optional; an output that is not requested stays poison."""
    L = hip.lib()
    B, H, W = 3, 1, 683
    npix = B * H * W
    x, labels = logits_and_labels(B, H, W)
    z = step_ref.onehot2(labels)
    loss_ref, grad_ref = step_ref.bce(x, z)
    for want_dx, want_mask in ((True, False), (False, True), (False, False)):
        mem = gd.Arena()
        view, (xsB, xsC, xsH) = strided(mem, x)
        loss = mem.out((1,), torch.float32, "loss"); dx = mem.out((B, 2, H, W), torch.float32, "dlogits")
        mask = mem.out((B, H, W), torch.int64, "mask")
        sc = mem.scratch(L.unet_bce_step_scratch_bytes(npix), "bce_step scratch")
        hip.check(L.unet_bce_step(view, xsB, xsC, xsH, mem.ptr(put(mem, labels, "labels")), None, 0, 0, 0, 0, B, H, W, mem.ptr(loss),
                                  mem.ptr(dx) if want_dx else None, 1.0, mem.ptr(mask) if want_mask else None, mem.ptr(sc), hip.stream()))
        mem.verify(loss, dx if want_dx else None, mask if want_mask else None)
        assert abs(loss.item() - loss_ref) < 1e-5 * abs(loss_ref)
        assert nerr(dx.cpu().numpy(), grad_ref) < 1e-5 if want_dx else still_poison(dx)
        assert np.array_equal(mask.cpu().numpy(), step_ref.argmax2(x)) if want_mask else still_poison(mask)
    mem = gd.Arena()
    loss = mem.out((1,), torch.float32, "loss"); dx = mem.out((B, 2, H, W), torch.float32, "dlogits (not passed)")
    sc = mem.scratch(L.unet_bce_scratch_bytes(2 * npix), "bce_logits scratch")
    hip.check(L.unet_bce_logits(mem.ptr(put(mem, x, "logits")), mem.ptr(put(mem, z.astype(np.float32), "target")), None, 0, 0, 0, 0, B, H, W,
                                mem.ptr(loss), None, 1.0, mem.ptr(sc), hip.stream()))
    mem.verify(loss)
    assert abs(loss.item() - loss_ref) < 1e-5 * abs(loss_ref) and still_poison(dx)


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 5, 7), (2, 1031, 1021)])
def test_onehot2_and_argmax2(hip, B, H, W):
    """Bit-exact; strided logits inside NaN; ties (equal planes, +0.0 against -0.0) give class 0.  2 x 1031 x 1021 pixels
    exceed 8192 blocks x 256 lanes: the grid-stride loops."""
    L = hip.lib()
    assert (B, H, W) != (2, 1031, 1021) or B * H * W > 8192 * 256
    x, labels = logits_and_labels(B, H, W)
    mem = gd.Arena()
    view, (bs, ps, rs_) = strided(mem, x)
    am = mem.out((B, H, W), torch.int64, "argmax")
    hip.check(L.unet_argmax2(view, bs, ps, rs_, mem.ptr(am), B, H, W, hip.stream()))
    mem.verify(am)
    assert np.array_equal(am.cpu().numpy(), step_ref.argmax2(x))
    ll = mem.out((B, 2, H, W), torch.float32, "one-hot")
    hip.check(L.unet_onehot2(mem.ptr(put(mem, labels, "labels")), mem.ptr(ll), B, H, W, hip.stream()))
    mem.verify(ll)
    assert np.array_equal(ll.cpu().numpy(), step_ref.onehot2(labels).astype(np.float32))


# ---- unet_sgd_momentum ------------------------------------------------------------------------------------------------------
class SgdCase:
    """Parameters, gradients and momentum buffers from one Arena; buffers start as poison (the first step must not read them).
    misaligned: indices of tensors whose parameter and buffer start 4 bytes into their allocation."""

    def __init__(self, hip, sizes, misaligned=(), seed=0):
        self.hip, self.mem = hip, gd.Arena()
        self.gen = torch.Generator().manual_seed(seed)
        self.off = [1 if i in misaligned else 0 for i in range(len(sizes))]
        self.p_base = [self.mem.inp(torch.randn(n + o, generator=self.gen), "p%d" % i) for i, (n, o) in enumerate(zip(sizes, self.off))]
        self.b_base = [self.mem.out((n + o,), torch.float32, "buf%d" % i) for i, (n, o) in enumerate(zip(sizes, self.off))]
        self.ps = [b[o:] if o else b for b, o in zip(self.p_base, self.off)]
        self.bufs = [b[o:] if o else b for b, o in zip(self.b_base, self.off)]
        self.p0 = [b.clone() for b in self.p_base]
        self.addr = {}
        for base, t, o in zip(self.p_base + self.b_base, self.ps + self.bufs, self.off * 2):
            self.addr[id(t)] = self.mem.address(base) + 4 * o

    def make_grad(self, p):
        g = self.mem.inp(torch.randn(p.shape, generator=self.gen), "grad")
        self.addr[id(g)] = self.mem.address(g)
        return g

    def ptrs(self, tensors):
        """void*[]: addresses inside the guarded allocations (a zero-size tensor has no data_ptr of its own)"""
        arr = (C.c_void_p * max(len(tensors), 1))()
        for i, t in enumerate(tensors):
            arr[i] = self.addr[id(t)]
        return arr

    def after_call(self, step, gs, bufs):
        self.mem.verify(*[b for b, o in zip(self.b_base, self.off) if not o])
        for pb, bb, o in zip(self.p_base, self.b_base, self.off):
            if o:                                                   # the element in front of a misaligned tensor is not its own
                assert still_poison(bb[:1]) and not still_poison(bb[1:2])
        if step == 0:                                               # buf = g exactly and p finite: buf was not read
            for g, b, p in zip(gs, bufs, self.ps):
                assert torch.equal(b, g) and bool(torch.isfinite(p).all())

    def run(self, **kw):
        return step_ref.sgd_vs_oracle(self.hip, self.ps, bufs=self.bufs, make_grad=self.make_grad, ptrs=self.ptrs, after_call=self.after_call, **kw)


SGD_SIZES = [1, 4095, 4096, 0, 4097, 8192, 70001]              # either side of SGD_CHUNK = 4096, a zero-size tensor in the middle


@pytest.mark.parametrize("misaligned", [(), (1,), (0, 2, 4, 6)], ids=["vector", "one-unaligned", "four-unaligned"])
def test_sgd_momentum_sizes_and_alignment(hip, misaligned):
    """The elementwise bound of step_ref.sgd_vs_oracle (shared with test_step_side_kernels) over three steps.  All pointers
    16-byte aligned: the vector kernel, with 4-byte accesses on each tensor's tail; one tensor 4 bytes off beside aligned ones:
    the 4-byte kernel for all.  The first step runs on poisoned momentum buffers: buf == g bit-exactly and p finite, so buf was
    not read.  The chunk loop beyond the 16384-block cap needs more than 6.7e7 elements and is not reached here."""
    case = SgdCase(hip, SGD_SIZES, misaligned)
    case.run(nsteps=3)
    for pb, p0, o in zip(case.p_base, case.p0, case.off):
        if o:
            assert torch.equal(pb[:1], p0[:1])


def test_sgd_momentum_table_limits(hip):
    """46 tensors are accepted; 47 and 0 are rejected and nothing is written."""
    L = hip.lib()
    sizes = [(37 * i) % 300 + 1 for i in range(46)]; sizes[20] = 4097; sizes[45] = 4096
    SgdCase(hip, sizes).run(nsteps=2)
    case = SgdCase(hip, sizes + [5])
    gs = [case.make_grad(p) for p in case.ps]
    numel = (C.c_size_t * 47)(*[p.numel() for p in case.ps])
    for n in (47, 0):
        rc = L.unet_sgd_momentum(case.ptrs(case.ps), case.ptrs(gs), case.ptrs(case.bufs), numel, n, 0.1, 0.9, 1, hip.stream())
        rejected(hip, rc, case.mem, *case.bufs)
        assert all(torch.equal(p, p0) for p, p0 in zip(case.ps, case.p0))


@pytest.mark.parametrize("misaligned", [(), (1,)], ids=["vector", "scalar"])
def test_sgd_momentum_lr0_and_mu0(hip, misaligned):
    """lr = 0 leaves p bit-identical; mu = 0 gives buf == g at every step."""
    case = SgdCase(hip, SGD_SIZES, misaligned)
    case.run(nsteps=3, lr=0.0)
    assert all(torch.equal(pb, p0) for pb, p0 in zip(case.p_base, case.p0))
    case = SgdCase(hip, SGD_SIZES, misaligned, seed=1)
    seen = []

    def bufs_equal_grads(step, gs, bufs):
        case.after_call(step, gs, bufs)
        assert all(torch.equal(b, g) for b, g in zip(bufs, gs))
        seen.append(step)
    step_ref.sgd_vs_oracle(hip, case.ps, nsteps=3, mu=0.0, bufs=case.bufs, make_grad=case.make_grad, ptrs=case.ptrs, after_call=bufs_equal_grads)
    assert seen == [0, 1, 2]
