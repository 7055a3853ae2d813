"""Arithmetic mode 1 (bf16x3: every fp32 operand split into two bf16 terms, three bf16 MFMAs per product, fp32
accumulation; csrc/igemmx.hip and the wgrad<...;split3> instantiations of csrc/wgrad.hip), per op through the C ABI
against fp64 torch on the CPU.

Operands are NOT bf16-representable: splitting them is the point of the mode.  Each element is judged on its own
(tests/kernel_bounds.py derives the bound):
    |y - z| <= (C_SPLIT + lam sqrt(3K) 2^-24) A,   C_SPLIT = 2^-15 (1 + 2^-7),  lam = 8 (failure probability 2.6e-14),
A = the same contraction of absolute values in fp64 (weight and bias gradients: over the pixel sum).  A split probe
(positive operands whose split is fixed, bf16-exact partners) pins the split itself: the mean of (y - z_split) / A stays
within 2^-18, where a truncating lo conversion would show 2^-16.6.  Every case runs with both operand stagings
(unet_set_lds_dma 1 and 0) and asserts the kernel family it reached."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import kernel_bounds as kb
import guarded as gd
import kernel_paths as kp
from gpu_support import dma, hip_fixture, nchw, nhwc, rnd

pytestmark = pytest.mark.gpu

WORST = {}          # worst |y - z| / A per output kind, printed at the end of the module (-s)


hip = hip_fixture(math=1)


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for k, v in sorted(WORST.items()):
        print("bf16x3 %-6s worst |y-z|/A %.3e (bound %.3e at its K)" % (k, v[0], v[1]))


# (every buffer handed to the library comes from a guarded.Arena: tests/guarded.py; operands are drawn with rnd(fp32=True):
#  fp32 values, not bf16)


def judge(kind, y, z, A, K):
    st = kb.check_bf16x3(y.detach().double().cpu().numpy(), z.detach().double().numpy(), A.detach().double().numpy(), K)
    w = WORST.get(kind, (0.0, st["bound_rel"]))
    WORST[kind] = (max(w[0], st["worst_rel"]), st["bound_rel"])
    assert not torch.isnan(y).any()


def not_bf16(*ts):
    for t in ts:
        assert (t.float().to(torch.bfloat16).double() != t).float().mean() > 0.9


def family_of(rec, prefix):
    return [f for f in rec.families if f.startswith(prefix)]


def fwd_family(K, pad):
    return "igemmx<%s;%d;split3>" % ("128;128" if K % 128 == 0 else "256;64", int(pad))


@pytest.mark.parametrize("B,Hs,pad,C1,C2,K", [(2, 21, 0, 64, 0, 64), (1, 20, 0, 128, 0, 128), (2, 18, 0, 32, 0, 32), (1, 16, 0, 96, 0, 96),
                                              (2, 8, 6, 64, 64, 64),            # virtual concat, positive pad: the split forward (b.add = y)
                                              (1, 10, 3, 32, 32, 128),
                                              (2, 30, -3, 64, 64, 128)])        # crop
def test_conv3x3_fwd_bf16x3(hip, dma, B, Hs, pad, C1, C2, K):
    mem = gd.Arena()
    H = Hs + 2 * pad
    a = rnd(B, C1, Hs, Hs, seed=1, fp32=True); u = rnd(B, C2, H, H, seed=2, fp32=True) if C2 else None
    w = rnd(K, C1 + C2, 3, 3, seed=3, scale=0.05, fp32=True); b = rnd(K, seed=4, fp32=True)
    not_bf16(a, w)
    x = torch.cat((F.pad(a, (pad,) * 4), u), 1) if C2 else a
    z = F.relu(F.conv2d(x, w, b))
    A = F.conv2d(x.abs(), w.abs(), b.abs())
    y = mem.out((B, H - 2, H - 2, K), torch.float32, "y")
    sc = mem.scratch(hip.lib().unet_conv3x3_scratch_bytes(C1 + C2, K))
    with kp.record() as rec:
        hip.check(hip.lib().unet_conv3x3_fwd(hip.ptr(mem.inp(nhwc(a))), Hs, Hs, C1, pad, hip.ptr(mem.inp(nhwc(u))) if C2 else None, C2, B, H, H,
                                             hip.ptr(mem.inp(w.float().cuda())), hip.ptr(mem.inp(b.float().cuda())), K, 1, hip.ptr(y), mem.ptr(sc),
                                             hip.stream()), "conv3x3_fwd")
    mem.verify(y)
    judge("fwd", nchw(y), z, A, 9 * (C1 + C2) + 1)
    fams = family_of(rec, "igemmx<")
    split = C2 and pad > 0
    assert fams == ([fwd_family(K, 0), fwd_family(K, 1)] if split else [fwd_family(K, 0)]), rec      # (a crop reads inside both sources)


@pytest.mark.parametrize("B,H,C,K,use_mask,use_add", [(2, 21, 64, 64, True, False), (1, 18, 64, 128, False, True), (2, 13, 128, 256, True, True),
                                                      (2, 22, 32, 32, True, True), (1, 16, 96, 96, False, False)])
def test_conv3x3_bwd_bf16x3(hip, dma, B, H, C, K, use_mask, use_add):
    mem = gd.Arena()
    x = rnd(B, C, H, H, seed=1, fp32=True); w = rnd(K, C, 3, 3, seed=2, scale=0.05, fp32=True); dz = rnd(B, K, H - 2, H - 2, seed=3, fp32=True)
    mask = rnd(B, C, H, H, seed=4, fp32=True).clamp_min(0) if use_mask else None
    add = rnd(B, C, H, H, seed=5, fp32=True) if use_add else None
    not_bf16(x, w, dz)
    dx_z = conv2d_input(x.shape, w, dz); dx_A = conv2d_input(x.shape, w.abs(), dz.abs())
    if add is not None:
        dx_z = dx_z + add; dx_A = dx_A + add.abs()
    if mask is not None:
        dx_z = dx_z * (mask > 0); dx_A = dx_A * (mask > 0)
    dw_z = conv2d_weight(x, w.shape, dz); dw_A = conv2d_weight(x.abs(), w.shape, dz.abs())
    dx = mem.out((B, H, H, C), torch.float32, "dx"); dw = mem.out((K, C, 3, 3), torch.float32, "dw"); db = mem.out((K,), torch.float32, "db")
    sc = mem.scratch(hip.lib().unet_conv3x3_bwd_scratch_bytes(B, H, H, C, K))
    with kp.record() as rec:
        hip.check(hip.lib().unet_conv3x3_bwd(hip.ptr(mem.inp(nhwc(x))), H, H, C, 0, None, 0, B, H, H, hip.ptr(mem.inp(w.float().cuda())), K,
                                             hip.ptr(mem.inp(nhwc(dz))), hip.ptr(dx), hip.ptr(mem.inp(nhwc(mask))) if use_mask else None,
                                             hip.ptr(mem.inp(nhwc(add))) if use_add else None, None, None, hip.ptr(dw), hip.ptr(db),
                                             mem.ptr(sc), hip.stream()), "conv3x3_bwd")
    mem.verify(dx, dw, db)
    judge("dgrad", nchw(dx), dx_z, dx_A, 9 * K + 1)
    judge("wgrad", dw, dw_z, dw_A, B * (H - 2) ** 2)
    judge("bgrad", db, dz.sum((0, 2, 3)), dz.abs().sum((0, 2, 3)), B * (H - 2) ** 2)
    assert family_of(rec, "igemmx<") == ["igemmx<%s;1;split3>" % ("128;128" if C % 128 == 0 else "256;64")], rec
    assert family_of(rec, "wgrad<") == ["wgrad<3;3;1;split3>"], rec
    assert [f["buf"] for f in rec.fields("wgrad<3;3;1;split3>")] == [str(dma)]


@pytest.mark.parametrize("B,Hs,pad,C,K", [(2, 8, 6, 64, 64), (1, 12, 3, 32, 64), (2, 30, -3, 64, 128)])
def test_conv3x3_bwd_virtual_concat_bf16x3(hip, dma, B, Hs, pad, C, K):
    mem = gd.Arena()
    H = Hs + 2 * pad
    a = rnd(B, C, Hs, Hs, seed=1, fp32=True).requires_grad_(True); u = rnd(B, C, H, H, seed=2, fp32=True).requires_grad_(True)
    w = rnd(K, 2 * C, 3, 3, seed=3, scale=0.05, fp32=True).requires_grad_(True); dz = rnd(B, K, H - 2, H - 2, seed=4, fp32=True)
    F.conv2d(torch.cat((F.pad(a, (pad,) * 4), u), 1), w).backward(dz)
    aa = a.detach().abs().requires_grad_(True); ua = u.detach().abs().requires_grad_(True); wa = w.detach().abs().requires_grad_(True)
    F.conv2d(torch.cat((F.pad(aa, (pad,) * 4), ua), 1), wa).backward(dz.abs())
    dx1 = mem.out((B, Hs, Hs, C), torch.float32, "dx1"); dx2 = mem.out((B, H, H, C), torch.float32, "dx2")
    dw = mem.out((K, 2 * C, 3, 3), torch.float32, "dw"); db = mem.out((K,), torch.float32, "db")
    sc = mem.scratch(hip.lib().unet_conv3x3_bwd_scratch_bytes(B, H, H, 2 * C, K))
    with kp.record() as rec:
        hip.check(hip.lib().unet_conv3x3_bwd(hip.ptr(mem.inp(nhwc(a.detach()))), Hs, Hs, C, pad, hip.ptr(mem.inp(nhwc(u.detach()))), C, B, H, H,
                                             hip.ptr(mem.inp(w.detach().float().cuda())), K, hip.ptr(mem.inp(nhwc(dz))), hip.ptr(dx1), None, None,
                                             hip.ptr(dx2), None, hip.ptr(dw), hip.ptr(db), mem.ptr(sc), hip.stream()), "conv3x3_bwd concat")
    mem.verify(dx1, dx2, dw, db)
    judge("dgrad", nchw(dx1), a.grad, aa.grad, 9 * K)
    judge("dgrad", nchw(dx2), u.grad, ua.grad, 9 * K)
    judge("wgrad", dw, w.grad, wa.grad, B * (H - 2) ** 2)
    judge("bgrad", db, dz.sum((0, 2, 3)), dz.abs().sum((0, 2, 3)), B * (H - 2) ** 2)
    assert family_of(rec, "wgrad<") == ["wgrad<3;3;1;split3>"] * 2, rec
    assert {f["buf"] for f in rec.fields("wgrad<3;3;1;split3>")} == {str(dma)}


@pytest.mark.parametrize("B,H,Ci,Co", [(2, 7, 128, 64), (1, 13, 256, 128), (3, 11, 64, 32), (2, 9, 96, 96)])
def test_upconv2_fwd_bwd_bf16x3(hip, dma, B, H, Ci, Co):
    mem = gd.Arena()
    x = rnd(B, Ci, H, H, seed=1, fp32=True).clamp_min(0); w = rnd(Ci, Co, 2, 2, seed=2, scale=0.05, fp32=True); b = rnd(Co, seed=3, fp32=True)
    dy = rnd(B, Co, 2 * H, 2 * H, seed=4, fp32=True)
    not_bf16(w, dy)
    z = F.conv_transpose2d(x, w, b, stride=2); A = F.conv_transpose2d(x.abs(), w.abs(), b.abs(), stride=2)
    xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True)
    F.conv_transpose2d(xr, wr, stride=2).backward(dy)
    xa = x.abs().requires_grad_(True); wa = w.abs().requires_grad_(True)
    F.conv_transpose2d(xa, wa, stride=2).backward(dy.abs())
    sc = mem.scratch(hip.lib().unet_upconv2_scratch_bytes(B, H, H, max(Ci, 64), max(Co, 64)))
    y = mem.out((B, 2 * H, 2 * H, Co), torch.float32, "y")
    xd = mem.inp(nhwc(x))
    dx = mem.out((B, H, H, Ci), torch.float32, "dx"); dw = mem.out((Ci, Co, 2, 2), torch.float32, "dw"); db = mem.out((Co,), torch.float32, "db")
    with kp.record() as rec:
        hip.check(hip.lib().unet_upconv2_fwd(hip.ptr(xd), B, H, H, Ci, hip.ptr(mem.inp(w.float().cuda())), hip.ptr(mem.inp(b.float().cuda())), Co,
                                             hip.ptr(y), mem.ptr(sc), hip.stream()), "upconv2_fwd")
        hip.check(hip.lib().unet_upconv2_bwd(hip.ptr(xd), B, H, H, Ci, hip.ptr(mem.inp(w.float().cuda())), Co, hip.ptr(mem.inp(nhwc(dy))),
                                             hip.ptr(dx), hip.ptr(xd), hip.ptr(dw), hip.ptr(db), mem.ptr(sc), hip.stream()), "upconv2_bwd")
    mem.verify(y, dx, dw, db)
    judge("upfwd", nchw(y), z, A, Ci + 1)
    judge("updgrd", nchw(dx), xr.grad * (x > 0), xa.grad * (x > 0), 4 * Co)
    judge("upwgrd", dw, wr.grad, wa.grad, B * H * H)
    judge("bgrad", db, dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3)), 4 * B * H * H)
    assert family_of(rec, "wgrad") == ["wgrad<2;2;2;split3>", "wgrad_reduce"], rec
    assert [f["buf"] for f in rec.fields("wgrad<2;2;2;split3>")] == [str(dma)]
    assert all(f.startswith("igemmx<") and f.endswith(";split3>") for f in rec.families if f.startswith("igemm")), rec


def test_split_probe_pins_the_split(hip):
    """Forward (igemmx: activations split), dgrad (igemmx: dz split) and weight gradient (wgrad split3: X split) on split
    probes with positive bf16-exact partners: the mean of (y - z_split) / A, z_split = the exact sum of the three
    prescribed bf16 products, must stay within 2^-18 (a truncated lo: about -2^-16.6)."""
    mem = gd.Arena()
    B, H, C, K = 2, 18, 64, 64
    probe = lambda *s, seed: torch.from_numpy(kb.split_probe(s, seed))
    hi_lo = lambda t: torch.from_numpy(sum(kb.split3(t.numpy())))        # hi + lo: what the split keeps of a bf16-exact partner
    pos16 = lambda *s, seed, scale: (rnd(*s, seed=seed, scale=scale, fp32=True).abs() + scale / 8).to(torch.bfloat16).double()
    x = probe(B, C, H, H, seed=1); w = pos16(K, C, 3, 3, seed=2, scale=0.05)
    dz = probe(B, K, H - 2, H - 2, seed=3)
    y = mem.out((B, H - 2, H - 2, K), torch.float32, "y"); zb = mem.inp(torch.zeros(K))
    dx = mem.out((B, H, H, C), torch.float32, "dx"); dw = mem.out((K, C, 3, 3), torch.float32, "dw")
    sc = mem.scratch(hip.lib().unet_conv3x3_scratch_bytes(C, K)); sc2 = mem.scratch(hip.lib().unet_conv3x3_bwd_scratch_bytes(B, H, H, C, K))
    hip.check(hip.lib().unet_conv3x3_fwd(hip.ptr(mem.inp(nhwc(x))), H, H, C, 0, None, 0, B, H, H, hip.ptr(mem.inp(w.float().cuda())), hip.ptr(zb), K, 0,
                                         hip.ptr(y), mem.ptr(sc), hip.stream()), "fwd")
    hip.check(hip.lib().unet_conv3x3_bwd(hip.ptr(mem.inp(nhwc(x))), H, H, C, 0, None, 0, B, H, H, hip.ptr(mem.inp(w.float().cuda())), K,
                                         hip.ptr(mem.inp(nhwc(dz))), hip.ptr(dx), None, None, None, None, None, None, mem.ptr(sc2), hip.stream()), "dgrad")
    dzb = pos16(B, K, H - 2, H - 2, seed=5, scale=1.0)
    hip.check(hip.lib().unet_conv3x3_bwd(hip.ptr(mem.inp(nhwc(x))), H, H, C, 0, None, 0, B, H, H, hip.ptr(mem.inp(w.float().cuda())), K,
                                         hip.ptr(mem.inp(nhwc(dzb))), None, None, None, None, None, hip.ptr(dw), None, mem.ptr(sc2), hip.stream()), "wgrad")
    mem.verify(y, dx, dw)
    cases = [("fwd", nchw(y), F.conv2d(x, w), F.conv2d(hi_lo(x), w), 9 * C),
             ("dgrad", nchw(dx), conv2d_input(x.shape, w, dz), conv2d_input(x.shape, w, hi_lo(dz)), 9 * K),
             ("wgrad", dw, conv2d_weight(x, w.shape, dzb), conv2d_weight(hi_lo(x), w.shape, dzb), B * (H - 2) ** 2)]
    for name, got, z, zs, Kn in cases:
        got = got.cpu().double().numpy(); A = z.numpy()                  # positive operands: A = z
        kb.check_bf16x3(got, z.numpy(), A, Kn)
        bias = kb.split_bias(got, zs.numpy(), A)
        print("split probe %s: mean (y - z_split)/A = %.3g (tolerance %.3g)" % (name, bias, kb.SPLIT_BIAS_TOL))
        assert abs(bias) <= kb.SPLIT_BIAS_TOL, name
