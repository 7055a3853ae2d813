"""Per-op parity of the HIP kernels (through the C ABI) against fp64 torch CPU references and the
C oracle.  Floating point: tolerance = normalised max error (|d|_inf / |ref|_inf) <= 2e-5 for fp32
accumulation over up to 9216 terms (tolerances are normalised by tensor scale)."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded as gd
import kernel_paths as kp
import step_ref
from gpu_support import hip, library_state, nchw, nerr, nhwc, rnd

pytestmark = pytest.mark.gpu

TOL = 2e-5


# Every buffer handed to the library comes from a guarded.Arena (tests/guarded.py): outputs and scratch are poisoned and of the
# exact size, inputs are copies with poison around them; mem.verify(outputs...) = every element written, every guard intact.


ConvMode = collections.namedtuple("ConvMode", "mode dma")


@pytest.fixture(params=[(0, 1), (3, 1), (0, 0), (3, 0)], ids=["direct", "winograd", "direct-glds", "winograd-glds"])
def conv_mode(hip, request):
    """The 3x3 layers have two fp32 evaluations: the direct fmaf chain (math mode 0) and Winograd F(2x2,3x3) (mode 3);
    each stages its operands either by buffer-descriptor LDS-DMA (default) or by global_load_lds — the instantiation
    tensors >= 2 GiB take (BASELINE config #5 at batch 16), forced here with unet_set_lds_dma(0);
    tests/test_large_tensors_gpu.py reaches it by size, with the knob at its default."""
    mode, dma = request.param
    with library_state(math=mode, lds_dma=dma):
        yield ConvMode(mode, dma)


@pytest.mark.parametrize("B,H,C,K", [(2, 21, 64, 64), (1, 37, 64, 128), (3, 14, 128, 128), (1, 12, 256, 512), (2, 9, 128, 64), (1, 30, 32, 32),
                                     (3, 26, 128, 128), (1, 22, 256, 512), (2, 45, 64, 64),
                                     (1, 66, 512, 512),
                                     # minimal Winograd tile grids (9 x 9, 13 x 13 tiles per image): every 64-tile workgroup crosses an image boundary, ragged last one
                                     (4, 20, 64, 64), (5, 28, 64, 128),
                                     # 32 filter rows (the base-32 net of BASELINE configs[4]): half a 64-row block of transformed filters
                                     (2, 40, 32, 32), (1, 34, 32, 64), (1, 44, 64, 32), (2, 22, 96, 96)])
def test_conv3x3_fwd(hip, conv_mode, B, H, C, K):
    mem = gd.Arena()
    x = rnd(B, C, H, H, seed=1); w = rnd(K, C, 3, 3, seed=2, scale=0.05); b = rnd(K, seed=3)
    ref = F.relu(F.conv2d(x, w, b))
    y = mem.out((B, H - 2, H - 2, K), torch.float32, "y")
    sc = mem.scratch(hip.lib().unet_conv3x3_scratch_bytes(C, K))
    with kp.record() as rec:
        hip.check(hip.lib().unet_conv3x3_fwd(hip.ptr(mem.inp(nhwc(x))), H, H, C, 0, None, 0, B, H, H, hip.ptr(mem.inp(w.float().cuda())),
                                             hip.ptr(mem.inp(b.float().cuda())), K, 1, hip.ptr(y), mem.ptr(sc), hip.stream()), "conv3x3_fwd")
    mem.verify(y)
    assert nerr(nchw(y), ref) < TOL
    assert rec.main_families() == [kp.fp32_conv_family(*conv_mode, H - 2, K, [C])], rec       # (mode 3: a listed fallback runs igemm)


def test_conv3x3_random_shapes(hip):
    """30 random shapes (channel counts incl. 192, batch 1-3, extents 6-64, virtual concat with pad -3..7) through the
    forward and backward entry points in the default mode, against fp64 (tools/fuzz_conv.py)."""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("fuzz_conv", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_conv.py"))
    fz = importlib.util.module_from_spec(spec); spec.loader.exec_module(fz)
    assert fz.run(30, 11, verbose=False, arena=gd.Arena) < TOL


@pytest.mark.parametrize("B,Hs,pad,C1,C2,K", [(2, 8, 6, 64, 64, 64), (1, 10, 3, 128, 128, 128), (1, 6, 0, 64, 64, 128),
                                               (1, 24, 4, 64, 64, 64), (2, 30, -3, 64, 64, 128), (1, 20, 1, 128, 128, 64),
                                               (1, 26, 5, 32, 32, 32), (2, 32, -2, 32, 32, 32)])
def test_conv3x3_fwd_virtual_concat(hip, conv_mode, B, Hs, pad, C1, C2, K):
    mem = gd.Arena()
    """crop_and_concat (network.py:108-127) is never materialised: the conv reads two sources."""
    H = Hs + 2 * pad
    a = rnd(B, C1, Hs, Hs, seed=1); u = rnd(B, C2, H, H, seed=2)
    w = rnd(K, C1 + C2, 3, 3, seed=3, scale=0.05); b = rnd(K, seed=4)
    cat = torch.cat((F.pad(a, (pad,) * 4), u), 1)
    ref = F.relu(F.conv2d(cat, w, b))
    y = mem.out((B, H - 2, H - 2, K), torch.float32, "y")
    sc = mem.scratch(hip.lib().unet_conv3x3_scratch_bytes(C1 + C2, K))
    with kp.record() as rec:
        hip.check(hip.lib().unet_conv3x3_fwd(hip.ptr(mem.inp(nhwc(a))), Hs, Hs, C1, pad, hip.ptr(mem.inp(nhwc(u))), C2, B, H, H,
                                             hip.ptr(mem.inp(w.float().cuda())), hip.ptr(mem.inp(b.float().cuda())), K, 1, hip.ptr(y), mem.ptr(sc),
                                             hip.stream()), "conv3x3_fwd concat")
    mem.verify(y)
    assert nerr(nchw(y), ref) < TOL
    # one two-source launch, or (zero-padded skip, small window) the up-conv source then the skip's window; Winograd where it applies
    assert rec.main_families() == kp.concat_fwd_families(*conv_mode, Hs, pad, C1, C2, K), rec


@pytest.mark.parametrize("B,H,C,K,use_mask,use_add", [(2, 21, 64, 64, True, False), (1, 38, 64, 128, False, True),
                                                      (2, 13, 128, 256, True, True), (1, 70, 64, 64, True, False), (2, 25, 128, 256, True, True),
                                                      (1, 66, 512, 512, True, True), (4, 20, 64, 64, True, True),
                                                      (2, 40, 32, 32, True, True), (1, 34, 32, 64, True, False), (1, 44, 64, 32, False, True)])
def test_conv3x3_bwd(hip, conv_mode, B, H, C, K, use_mask, use_add):
    mem = gd.Arena()
    x = rnd(B, C, H, H, seed=1).requires_grad_(True)
    w = rnd(K, C, 3, 3, seed=2, scale=0.05).requires_grad_(True)
    dz = rnd(B, K, H - 2, H - 2, seed=3)
    mask = rnd(B, C, H, H, seed=4).clamp_min(0) if use_mask else None     # a ReLU output: many exact zeros
    add = rnd(B, C, H, H, seed=5) if use_add else None
    F.conv2d(x, w).backward(dz)
    dx_ref = x.grad.clone()
    if add is not None:
        dx_ref = dx_ref + add
    if mask is not None:
        dx_ref = dx_ref * (mask > 0)
    dx = mem.out((B, H, H, C), torch.float32, "dx"); dw = mem.out((K, C, 3, 3), torch.float32, "dw"); db = mem.out((K,), torch.float32, "db")
    sc = mem.scratch(hip.lib().unet_conv3x3_bwd_scratch_bytes(B, H, H, C, K))
    with kp.record() as rec:
        hip.check(hip.lib().unet_conv3x3_bwd(hip.ptr(mem.inp(nhwc(x.detach()))), H, H, C, 0, None, 0, B, H, H, hip.ptr(mem.inp(w.detach().float().cuda())), K,
                                             hip.ptr(mem.inp(nhwc(dz))), hip.ptr(dx), hip.ptr(mem.inp(nhwc(mask))) if use_mask else None,
                                             hip.ptr(mem.inp(nhwc(add))) if use_add else None, None, None, hip.ptr(dw), hip.ptr(db),
                                             mem.ptr(sc), hip.stream()), "conv3x3_bwd")
    mem.verify(dx, dw, db)
    assert rec.main_families()[0] == kp.fp32_conv_family(*conv_mode, H, C, [K], pad=True), rec
    assert rec.main_families()[1] == kp.wgrad_family(*conv_mode, C, K), rec
    assert nerr(nchw(dx), dx_ref) < TOL
    assert nerr(dw, w.grad) < TOL
    assert nerr(db, dz.sum((0, 2, 3))) < TOL


@pytest.mark.parametrize("B,Hs,pad,C,K", [(2, 8, 6, 64, 64), (1, 12, 3, 128, 128), (1, 8, 0, 64, 64), (1, 24, 4, 64, 64), (2, 30, -3, 64, 128),
                                          (1, 26, 5, 32, 32), (2, 32, -2, 32, 64)])
def test_conv3x3_bwd_virtual_concat(hip, conv_mode, B, Hs, pad, C, K):
    mem = gd.Arena()
    H = Hs + 2 * pad
    a = rnd(B, C, Hs, Hs, seed=1).requires_grad_(True); u = rnd(B, C, H, H, seed=2).requires_grad_(True)
    w = rnd(K, 2 * C, 3, 3, seed=3, scale=0.05).requires_grad_(True)
    dz = rnd(B, K, H - 2, H - 2, seed=4)
    F.conv2d(torch.cat((F.pad(a, (pad,) * 4), u), 1), w).backward(dz)
    dx1 = mem.out((B, Hs, Hs, C), torch.float32, "dx1"); dx2 = mem.out((B, H, H, C), torch.float32, "dx2")
    dw = mem.out((K, 2 * C, 3, 3), torch.float32, "dw"); db = mem.out((K,), torch.float32, "db")
    sc = mem.scratch(hip.lib().unet_conv3x3_bwd_scratch_bytes(B, H, H, 2 * C, K))
    with kp.record() as rec:
        hip.check(hip.lib().unet_conv3x3_bwd(hip.ptr(mem.inp(nhwc(a.detach()))), Hs, Hs, C, pad, hip.ptr(mem.inp(nhwc(u.detach()))), C, B, H, H,
                                             hip.ptr(mem.inp(w.detach().float().cuda())), K, hip.ptr(mem.inp(nhwc(dz))), hip.ptr(dx1), None, None,
                                             hip.ptr(dx2), None, hip.ptr(dw), hip.ptr(db), mem.ptr(sc), hip.stream()), "conv3x3_bwd concat")
    mem.verify(dx1, dx2, dw, db)
    assert rec.main_families(reduces=False) == kp.concat_bwd_families(*conv_mode, Hs, pad, C, C, K), rec
    assert nerr(nchw(dx1), a.grad) < TOL      # pad-backward == crop of the padded gradient
    assert nerr(nchw(dx2), u.grad) < TOL
    assert nerr(dw, w.grad) < TOL
    assert nerr(db, dz.sum((0, 2, 3))) < TOL


@pytest.mark.parametrize("B,H,Ci,Co", [(2, 7, 128, 64), (1, 13, 256, 128), (1, 4, 1024, 512), (3, 17, 64, 32)])
def test_upconv2_fwd(hip, B, H, Ci, Co):
    mem = gd.Arena()
    x = rnd(B, Ci, H, H, seed=1); w = rnd(Ci, Co, 2, 2, seed=2, scale=0.05); b = rnd(Co, seed=3)
    ref = F.conv_transpose2d(x, w, b, stride=2)
    y = mem.out((B, 2 * H, 2 * H, Co), torch.float32, "y")
    sc = mem.scratch(hip.lib().unet_upconv2_scratch_bytes(B, H, H, max(Ci, 64), max(Co, 64)))
    with kp.record() as rec:
        hip.check(hip.lib().unet_upconv2_fwd(hip.ptr(mem.inp(nhwc(x))), B, H, H, Ci, hip.ptr(mem.inp(w.float().cuda())), hip.ptr(mem.inp(b.float().cuda())), Co,
                                             hip.ptr(y), mem.ptr(sc), hip.stream()), "upconv2_fwd")
    mem.verify(y)
    assert nerr(nchw(y), ref) < TOL
    # a 1x1 GEMM with 4 Co filter rows scattered 2x2 (no Winograd in any fp32 mode, no padded taps)
    assert rec.main_families() == ["igemm<%s;0>" % ("128;128" if 4 * Co % 128 == 0 else "256;64")], rec


@pytest.fixture(params=[1, 0], ids=["pixel-linear", "row-walking"])
def up_staging(hip, request):
    """The up-conv weight gradient runs as the pixel-linear kernel (buffer-descriptor LDS-DMA); with unet_set_lds_dma(0) - what
    tensors >= 2 GiB take by themselves - it falls back to the row-walking kernel."""
    with library_state(lds_dma=request.param):
        yield request.param


# (the weight gradient is the pixel-linear kernel: fewer pixels than one 32-pixel chunk, a ragged last chunk, chunks that cross
#  image boundaries, the half-filled channel tiles of the base-32 net, several channel tiles in both directions)
@pytest.mark.parametrize("B,H,Ci,Co", [(2, 7, 128, 64), (1, 13, 256, 128), (1, 18, 128, 64), (1, 5, 64, 64), (3, 11, 64, 32), (5, 6, 256, 256)])
def test_upconv2_bwd(hip, B, H, Ci, Co, up_staging):
    mem = gd.Arena()
    x = rnd(B, Ci, H, H, seed=1).clamp_min(0).requires_grad_(True)     # the producer's ReLU output
    w = rnd(Ci, Co, 2, 2, seed=2, scale=0.05).requires_grad_(True)
    dy = rnd(B, Co, 2 * H, 2 * H, seed=3)
    F.conv_transpose2d(x, w, stride=2).backward(dy)
    dx_ref = x.grad * (x.detach() > 0)
    dx = mem.out((B, H, H, Ci), torch.float32, "dx"); dw = mem.out((Ci, Co, 2, 2), torch.float32, "dw"); db = mem.out((Co,), torch.float32, "db")
    sc = mem.scratch(hip.lib().unet_upconv2_scratch_bytes(B, H, H, Ci, Co))
    xd = mem.inp(nhwc(x.detach()))
    with kp.record() as rec:
        hip.check(hip.lib().unet_upconv2_bwd(hip.ptr(xd), B, H, H, Ci, hip.ptr(mem.inp(w.detach().float().cuda())), Co, hip.ptr(mem.inp(nhwc(dy))),
                                             hip.ptr(dx), hip.ptr(xd), hip.ptr(dw), hip.ptr(db), mem.ptr(sc), hip.stream()), "upconv2_bwd")
    mem.verify(dx, dw, db)
    assert (up_staging and "wgrad_up<f32>" in rec.families) or (not up_staging and rec.reached("wgrad<2;2;2;split0> buf=0")), rec
    assert nerr(nchw(dx), dx_ref) < TOL
    assert nerr(dw, w.grad) < TOL
    assert nerr(db, dy.sum((0, 2, 3))) < TOL


def test_maxpool2_fwd_bwd_exact(hip):
    mem = gd.Arena()
    """Pool is a selection: bit-exact, including first-max-wins ties (all-zero windows after ReLU)."""
    B, H, Cc = 2, 12, 64
    pre = rnd(B, Cc, H, H, seed=1).clamp_min(0).float()
    pre[0, :, 0:2, 0:2] = 0.0
    pre[1, 3, 4:6, 4:6] = 1.25                                   # positive tie: first (row-major) wins
    p = pre.clone().requires_grad_(True)
    y_ref = F.max_pool2d(F.relu(p), 2, 2)
    dy = rnd(B, Cc, H // 2, H // 2, seed=2).float()
    y_ref.backward(dy)
    y = mem.out((B, H // 2, H // 2, Cc), torch.float32, "y"); dpre = mem.out((B, H, H, Cc), torch.float32, "dpre")
    xd = mem.inp(nhwc(pre))
    hip.check(hip.lib().unet_maxpool2_fwd(hip.ptr(xd), hip.ptr(y), B, H, H, Cc, hip.stream()))
    hip.check(hip.lib().unet_maxpool2_bwd(hip.ptr(xd), hip.ptr(mem.inp(nhwc(dy))), hip.ptr(dpre), B, H, H, Cc, hip.stream()))
    mem.verify(y, dpre)
    assert torch.equal(y.permute(0, 3, 1, 2).cpu(), y_ref.detach())
    assert torch.equal(dpre.permute(0, 3, 1, 2).cpu(), p.grad)


def test_head1x1_fwd_bwd(hip):
    mem = gd.Arena()
    B, H, Cc = 2, 37, 64
    x = rnd(B, Cc, H, H, seed=1).clamp_min(0).requires_grad_(True)
    w = rnd(2, Cc, 1, 1, seed=2, scale=0.1).requires_grad_(True); b = rnd(2, seed=3)
    ref = F.conv2d(x, w, b)
    dl = rnd(B, 2, H, H, seed=4)
    ref.backward(dl)
    logits = mem.out((B, 2, H, H), torch.float32, "logits")
    xd = mem.inp(nhwc(x.detach()))
    hip.check(hip.lib().unet_head1x1_fwd(hip.ptr(xd), B, H, H, Cc, hip.ptr(mem.inp(w.detach().float().cuda())), hip.ptr(mem.inp(b.float().cuda())),
                                         hip.ptr(logits), hip.stream()))
    mem.verify(logits)
    assert nerr(logits, ref) < TOL
    dz = mem.out((B, H, H, Cc), torch.float32, "dz"); dw = mem.out((2, Cc, 1, 1), torch.float32, "dw"); db = mem.out((2,), torch.float32, "db")
    sc = mem.scratch(hip.lib().unet_head1x1_bwd_scratch_bytes(B, H, H, Cc))
    hip.check(hip.lib().unet_head1x1_bwd(hip.ptr(xd), B, H, H, Cc, hip.ptr(mem.inp(w.detach().float().cuda())), hip.ptr(mem.inp(dl.float().cuda())),
                                         hip.ptr(dz), hip.ptr(dw), hip.ptr(db), mem.ptr(sc), hip.stream()))
    mem.verify(dz, dw, db)
    assert nerr(nchw(dz), x.grad * (x.detach() > 0)) < TOL
    assert nerr(dw, w.grad) < TOL
    assert nerr(db, dl.sum((0, 2, 3))) < TOL


@pytest.mark.parametrize("B,S,K", [(2, 44, 64), (1, 188, 64), (3, 60, 32), (1, 572, 64)])
def test_conv1ch_fwd_bwd_vs_c_oracle(hip, B, S, K):
    mem = gd.Arena()
    from oracle import oracle_c
    x = rnd(B, 1, S, S, seed=1).float(); w = rnd(K, 1, 3, 3, seed=2).float(); b = rnd(K, seed=3).float()
    ref = oracle_c.conv_valid_fwd(x.double().numpy(), w.double().numpy(), b.double().numpy(), True)
    y = mem.out((B, S - 2, S - 2, K), torch.float32, "y")
    with kp.record() as rec:
        hip.check(hip.lib().unet_conv1ch_fwd(hip.ptr(mem.inp(x.cuda())), B, S, hip.ptr(mem.inp(w.cuda())), hip.ptr(mem.inp(b.cuda())), K, hip.ptr(y), hip.stream()))
    mem.verify(y)
    assert nerr(nchw(y), torch.from_numpy(ref)) < TOL
    assert [f for f, r in zip(rec.families, rec.rows) if r["kind"] == kp.K_CONV11C] == ["conv1ch_fwd"], rec
    dz = rnd(B, K, S - 2, S - 2, seed=4).float()
    _, dw_ref, db_ref = oracle_c.conv_valid_bwd(x.double().numpy(), w.double().numpy(), dz.double().numpy(), need_dx=False)
    dw = mem.out((K, 1, 3, 3), torch.float32, "dw"); db = mem.out((K,), torch.float32, "db")
    sc = mem.scratch(hip.lib().unet_conv1ch_bwd_scratch_bytes(B, S, K))
    with kp.record() as rec:
        hip.check(hip.lib().unet_conv1ch_bwd(hip.ptr(mem.inp(x.cuda())), B, S, K, hip.ptr(mem.inp(nhwc(dz))), hip.ptr(dw), hip.ptr(db), mem.ptr(sc), hip.stream()))
    mem.verify(dw, db)
    assert [f for f, r in zip(rec.families, rec.rows) if r["kind"] == kp.K_CONV11C] == ["conv1ch_wgrad"], rec
    assert nerr(dw, torch.from_numpy(dw_ref)) < TOL
    assert nerr(db, torch.from_numpy(db_ref)) < TOL


def test_step_side_kernels(hip, golden_dir):
    mem = gd.Arena()
    import os
    from oracle import oracle_c, prng
    L = hip.lib()
    ka = np.load(os.path.join(golden_dir, "known_answers.npz"))
    g = np.load(os.path.join(golden_dir, "unet_S220.npz"))
    lg = torch.from_numpy(g["logits_f64"]).float().cuda()
    labels = torch.from_numpy(prng.make_labels(3, 2, 36)).cuda()
    B, _, H, W = lg.shape
    ll = mem.out(lg.shape, torch.float32, "ll")
    hip.check(L.unet_onehot2(hip.ptr(labels), hip.ptr(ll), B, H, W, hip.stream()))
    mem.verify(ll)
    assert torch.equal(ll[:, 1].cpu(), labels[:, 0].float().cpu()) and torch.equal(ll[:, 0].cpu(), 1 - labels[:, 0].float().cpu())
    loss = mem.out((1,), torch.float32, "loss"); dx = mem.out(lg.shape, torch.float32, "dx")
    sc = mem.scratch(L.unet_bce_scratch_bytes(lg.numel()))
    # L1 unweighted: golden from the reference's nn.BCEWithLogitsLoss
    hip.check(L.unet_bce_logits(hip.ptr(lg), hip.ptr(ll), None, 0, 0, 0, 0, B, H, W, hip.ptr(loss), hip.ptr(dx), 1.0, mem.ptr(sc), hip.stream()))
    mem.verify(loss, dx)
    assert abs(loss.item() - float(ka["bce_plain_loss"])) < 1e-5 * abs(float(ka["bce_plain_loss"]))
    assert nerr(dx, torch.from_numpy(ka["bce_plain_grad"])) < 1e-5
    # L1 weighted with the reference's broadcast (Q4): weight [B,H,W] aligned so that B meets the class axis
    wm = torch.from_numpy(ka["class_balance_rand"]).float().cuda()           # [2,H,W]
    loss = mem.out((1,), torch.float32, "loss (weighted)"); dx = mem.out(lg.shape, torch.float32, "dx (weighted)")   # fresh poison per call
    hip.check(L.unet_bce_logits(hip.ptr(lg), hip.ptr(ll), hip.ptr(wm), 0, H * W, W, 1, B, H, W, hip.ptr(loss), hip.ptr(dx), 1.0,
                                mem.ptr(sc), hip.stream()))
    mem.verify(loss, dx)
    assert abs(loss.item() - float(ka["bce_weighted_loss"])) < 1e-5 * abs(float(ka["bce_weighted_loss"]))
    assert nerr(dx, torch.from_numpy(ka["bce_weighted_grad"])) < 1e-5
    # L2 argmax: integer result, bit-exact against the reference
    am = mem.out((B, H, W), torch.int64, "am")
    hip.check(L.unet_argmax2(hip.ptr(lg), 2 * H * W, H * W, W, hip.ptr(am), B, H, W, hip.stream()))
    mem.verify(am)
    assert np.array_equal(am.cpu().numpy(), ka["argmax_S220"])
    tie = torch.zeros(1, 2, 4, 4, device="cuda"); am2 = mem.out((1, 4, 4), torch.int64, "am2")
    hip.check(L.unet_argmax2(hip.ptr(tie), 32, 16, 4, hip.ptr(am2), 1, 4, 4, hip.stream()))
    mem.verify(am2)
    assert int(am2.sum()) == 0                                               # ties -> class 0
    # L1 + L2 fused (unet_bce_step): integer labels instead of the one-hot target, loss + gradient + argmax in one pass;
    # the logits are a centre-cropped VIEW of a larger tensor, as in the trainer (trainer.py:60-61)
    big = torch.full((B, 2, H + 4, W + 6), 123.0, device="cuda")
    big[:, :, 2:2 + H, 3:3 + W] = lg
    view = big[:, :, 2:2 + H, 3:3 + W]
    sc2 = mem.scratch(L.unet_bce_step_scratch_bytes(B * H * W))
    for wptr, wstr, kl, kg in ((None, (0, 0, 0, 0), "bce_plain_loss", "bce_plain_grad"), (hip.ptr(wm), (0, H * W, W, 1), "bce_weighted_loss", "bce_weighted_grad")):
        loss = mem.out((1,), torch.float32, "loss"); dx2 = mem.out(lg.shape, torch.float32, "dx2"); am3 = mem.out((B, H, W), torch.int64, "am3")
        hip.check(L.unet_bce_step(hip.ptr(view), view.stride(0), view.stride(1), view.stride(2), hip.ptr(labels), wptr, wstr[0], wstr[1], wstr[2], wstr[3],
                                  B, H, W, hip.ptr(loss), hip.ptr(dx2), 1.0, hip.ptr(am3), mem.ptr(sc2), hip.stream()))
        mem.verify(loss, dx2, am3)
        assert abs(loss.item() - float(ka[kl])) < 1e-5 * abs(float(ka[kl]))
        assert nerr(dx2, torch.from_numpy(ka[kg])) < 1e-5
        assert np.array_equal(am3.cpu().numpy(), ka["argmax_S220"])
    # grad_scale, and the optional outputs left out
    loss = mem.out((1,), torch.float32, "loss (grad_scale)"); dx2 = mem.out(lg.shape, torch.float32, "dx2 (grad_scale)")
    hip.check(L.unet_bce_step(hip.ptr(lg), 2 * H * W, H * W, W, hip.ptr(labels), None, 0, 0, 0, 0, B, H, W, hip.ptr(loss), hip.ptr(dx2), 0.25,
                              None, mem.ptr(sc2), hip.stream()))
    mem.verify(loss, dx2)
    assert nerr(dx2, 0.25 * torch.from_numpy(ka["bce_plain_grad"])) < 1e-5
    loss = mem.out((1,), torch.float32, "loss (alone)")
    hip.check(L.unet_bce_step(hip.ptr(lg), 2 * H * W, H * W, W, hip.ptr(labels), None, 0, 0, 0, 0, B, H, W, hip.ptr(loss), None, 1.0,
                              None, mem.ptr(sc2), hip.stream()))
    mem.verify(loss)
    assert abs(loss.item() - float(ka["bce_plain_loss"])) < 1e-5 * abs(float(ka["bce_plain_loss"]))
    # module-level wrapper: loss.backward() delivers that gradient to the logits
    import optim as hip_optim
    lgr = lg.clone().requires_grad_(True)
    l2, m2 = hip_optim.bce_argmax_step(lgr, labels, weight=wm)
    l2.backward()
    assert nerr(lgr.grad, torch.from_numpy(ka["bce_weighted_grad"])) < 1e-5 and np.array_equal(m2.cpu().numpy(), ka["argmax_S220"])
    # L3 SGD momentum, two steps, against the pinned C oracle in fp64, elementwise: the helper and the derivation of its bound
    # live in tests/step_ref.py, shared with tests/test_step_ops_gpu.py
    def sgd_vs_oracle(ps, nsteps=2, lr=1e-4, mu=0.99):
        step_ref.sgd_vs_oracle(hip, ps, nsteps=nsteps, lr=lr, mu=mu)
    torch.manual_seed(0)
    sgd_vs_oracle([torch.randn(n, device="cuda") for n in (5000, 3, 70001)])
    # pointers that are not 16-byte aligned take the 4-byte kernel: same bound
    base = [torch.randn(n + 1, device="cuda") for n in (5000, 70001)]
    sgd_vs_oracle([b[1:] for b in base])
