"""Path coverage per arithmetic mode: which kernel family each per-op case reaches (tests/kernel_paths.py reads the
library's per-launch tags), pinned to literal strings, with parity for every row; the union of the rows' families must
be the complete set the dispatch code offers for the mode, so a predicate change that moves coverage elsewhere fails.
Also: unet_set_lds_dma is a staging knob - outputs must be bit-identical under 1 and 0 (include/unet_hip.h names the
one exception)."""
import pytest
import torch
import torch.nn.functional as F

import guarded as gd
import kernel_paths as kp
from gpu_support import hip, library_state, nerr, rnd

pytestmark = pytest.mark.gpu

MAIN_KINDS = {kp.K_IGEMM, kp.K_WGRAD, kp.K_REDUCE, kp.K_WINO}


def run_op(hip, mode, dma, op, args):
    """Runs one per-op case in `mode` with staging `dma`; returns (record, outputs {name: device tensor}, references
    {name: (fp64 reference, is_activation)}).  Every requested output is checked to be fully written and every guard intact."""
    L = hip.lib()
    adt = torch.bfloat16 if mode == 2 else torch.float32
    q = (lambda t: t.to(torch.bfloat16).double()) if mode == 2 else (lambda t: t)       # what the kernels see of a tensor
    dev = lambda t: t.permute(0, 2, 3, 1).contiguous().to(adt).cuda()
    host = lambda t: t.permute(0, 3, 1, 2).double().cpu()
    mem = gd.Arena()                                                # every buffer the library sees: poisoned, guarded, exact (tests/guarded.py)
    k = mem.inp
    sc = lambda n: mem.ptr(mem.scratch(n))
    out, ref = {}, {}
    with library_state(math=mode, lds_dma=dma):
        with kp.record(L) as rec:
            if op in ("fwd", "bwd"):
                B, Hs, pad, C1, C2, K = args
                H = Hs + 2 * pad
                a = q(rnd(B, C1, Hs, Hs, seed=1, fp32=True)).requires_grad_(True)
                u = q(rnd(B, C2, H, H, seed=2, fp32=True)).requires_grad_(True) if C2 else None
                w = rnd(K, C1 + C2, 3, 3, seed=3, scale=0.05, fp32=True); b = rnd(K, seed=4, fp32=True)
                wq = q(w).requires_grad_(True)                      # (the gradient must not flow through the bf16 cast)
                x = torch.cat((F.pad(a, (pad,) * 4), u), 1) if C2 else a
                z = F.conv2d(x, wq, b)
                ad, ud = k(dev(a.detach())), (k(dev(u.detach())) if C2 else None)
                wd = k(w.detach().float().cuda())
                if op == "fwd":
                    y = mem.out((B, H - 2, H - 2, K), adt, "y")
                    hip.check(L.unet_conv3x3_fwd(hip.ptr(ad), Hs, Hs, C1, pad, hip.ptr(ud) if C2 else None, C2, B, H, H, hip.ptr(wd),
                                                 hip.ptr(k(b.float().cuda())), K, 1, hip.ptr(y), sc(L.unet_conv3x3_scratch_bytes(C1 + C2, K)),
                                                 hip.stream()), "conv3x3_fwd")
                    out["y"] = y; ref["y"] = (F.relu(z.detach()), True)
                else:
                    dz = q(rnd(B, K, H - 2, H - 2, seed=5, fp32=True))
                    z.backward(dz)
                    dx1 = mem.out((B, Hs, Hs, C1), adt, "dx1")
                    dx2 = mem.out((B, H, H, C2), adt, "dx2") if C2 else None
                    dw = mem.out((K, C1 + C2, 3, 3), torch.float32, "dw"); db = mem.out((K,), torch.float32, "db")
                    hip.check(L.unet_conv3x3_bwd(hip.ptr(ad), Hs, Hs, C1, pad, hip.ptr(ud) if C2 else None, C2, B, H, H, hip.ptr(wd), K,
                                                 hip.ptr(k(dev(dz))), hip.ptr(dx1), None, None, hip.ptr(dx2) if C2 else None, None,
                                                 hip.ptr(dw), hip.ptr(db), sc(L.unet_conv3x3_bwd_scratch_bytes(B, H, H, C1 + C2, K)),
                                                 hip.stream()), "conv3x3_bwd")
                    out.update(dx1=dx1, dw=dw, db=db); ref.update(dx1=(a.grad, True), dw=(wq.grad, False), db=(dz.sum((0, 2, 3)), False))
                    if C2:
                        out["dx2"] = dx2; ref["dx2"] = (u.grad, True)
            else:                                                   # "up": up-conv forward + backward
                B, H, Ci, Co = args
                x = q(rnd(B, Ci, H, H, seed=1, fp32=True).clamp_min(0)).requires_grad_(True)
                w = rnd(Ci, Co, 2, 2, seed=2, scale=0.05, fp32=True); b = rnd(Co, seed=3, fp32=True)
                wq = q(w).requires_grad_(True)
                dy = q(rnd(B, Co, 2 * H, 2 * H, seed=4, fp32=True))
                z = F.conv_transpose2d(x, wq, b, stride=2)
                z.backward(dy)
                s = sc(L.unet_upconv2_scratch_bytes(B, H, H, max(Ci, 64), max(Co, 64)))
                xd, wd = k(dev(x.detach())), k(w.detach().float().cuda())
                y = mem.out((B, 2 * H, 2 * H, Co), adt, "y")
                dx = mem.out((B, H, H, Ci), adt, "dx"); dw = mem.out((Ci, Co, 2, 2), torch.float32, "dw"); db = mem.out((Co,), torch.float32, "db")
                hip.check(L.unet_upconv2_fwd(hip.ptr(xd), B, H, H, Ci, hip.ptr(wd), hip.ptr(k(b.float().cuda())), Co, hip.ptr(y), s, hip.stream()), "upconv2_fwd")
                hip.check(L.unet_upconv2_bwd(hip.ptr(xd), B, H, H, Ci, hip.ptr(wd), Co, hip.ptr(k(dev(dy))), hip.ptr(dx), hip.ptr(xd), hip.ptr(dw), hip.ptr(db),
                                             s, hip.stream()), "upconv2_bwd")
                out.update(y=y, dx=dx, dw=dw, db=db)
                ref.update(y=(z.detach(), True), dx=(x.grad * (x.detach() > 0), True), dw=(wq.grad, False), db=(dy.sum((0, 2, 3)), False))
    mem.verify(*out.values())
    out = {n: (host(t) if t.dim() == 4 and n.startswith(("y", "dx")) else t.cpu()) for n, t in out.items()}
    return rec, out, ref


def parity(mode, out, ref):
    for n, (r, act) in ref.items():
        tol = 4e-3 if (mode == 2 and act) else 1e-4 if mode == 1 else 2e-5
        e = nerr(out[n], r)
        assert e < tol, "%s: normalised error %.3g >= %.3g" % (n, e, tol)


# (op, args, lds_dma, expected families - literal strings, optionally with a field one launch must carry)
#   fwd / bwd args: B, Hs, pad, C1, C2, K (C2 > 0: virtual concat of a pad-ed source 1 and source 2);  up: B, H, Ci, Co
TABLES = {
    0: [("fwd", (2, 21, 0, 64, 0, 128), 1, ["igemm<128;128;0>"]),
        ("fwd", (2, 21, 0, 64, 0, 64), 1, ["igemm<256;64;0>"]),
        ("fwd", (2, 8, 6, 64, 64, 128), 1, ["igemm<128;128;0>", "igemm<128;128;1>"]),        # split forward: launch 2 reads the padded skip
        ("bwd", (1, 18, 0, 64, 0, 128), 1, ["igemm<256;64;1>", "wgrad<3;3;1;split0> buf=0", "wgrad_reduce"]),
        ("bwd", (1, 18, 0, 128, 0, 64), 0, ["igemm<128;128;1>", "wgrad<3;3;1;split0> buf=0", "wgrad_reduce"]),
        ("fwd", (1, 20, 0, 32, 0, 64), 0, ["igemm<256;64;0>"]),
        ("up", (1, 7, 128, 64), 1, ["igemm<128;128;0>", "wgrad_up<f32>", "wgrad_reduce"]),
        ("up", (2, 32, 64, 64), 1, ["igemm<128;128;0>", "igemm<256;64;0>", "wgrad_up<f32> groups=64", "wgrad_reduce"]),   # >= 64 slabs: the wide reduce
        ("up", (1, 7, 128, 64), 0, ["wgrad<2;2;2;split0> buf=0", "wgrad_reduce"])],
    3: [("fwd", (2, 20, 0, 64, 0, 64), 1, ["wino32<1>"]),
        ("fwd", (2, 20, 0, 64, 0, 64), 0, ["wino32<0>"]),
        ("bwd", (2, 20, 0, 64, 0, 64), 1, ["wino32<1>", "wgradw<1>", "wgradw_reduce"]),
        ("bwd", (2, 20, 0, 64, 0, 128), 0, ["wino32<0>", "wgradw<0>", "wgradw_reduce"]),
        ("fwd", (1, 17, 0, 64, 0, 64), 1, ["igemm<256;64;0>"]),                # cdiv(OW, 2) = 8 < 9: the implicit GEMM
        ("fwd", (1, 17, 0, 64, 0, 128), 1, ["igemm<128;128;0>"]),
        ("fwd", (1, 20, 0, 64, 0, 48), 1, ["igemm<256;64;0>"]),                # Nn % 32 != 0 (legal in the forward): the implicit GEMM
        ("bwd", (1, 12, 0, 128, 0, 64), 1, ["igemm<128;128;1>", "wgradw<1>", "wgradw_reduce"]),     # dgrad of a small tile: cdiv(12, 2) < 9
        ("bwd", (1, 12, 0, 64, 0, 64), 0, ["igemm<256;64;1>", "wgradw<0>", "wgradw_reduce"]),
        ("bwd", (2, 20, 0, 32, 0, 32), 1, ["wino32<1>", "wgrad<3;3;1;split0> buf=0", "wgrad_reduce"]),   # 32 channels: no Winograd wgrad
        ("up", (1, 7, 128, 64), 1, ["igemm<128;128;0>", "wgrad_up<f32>", "wgrad_reduce"]),          # up-conv: as in mode 0
        ("up", (1, 7, 128, 64), 0, ["wgrad<2;2;2;split0> buf=0", "wgrad_reduce"])],
    1: [("fwd", (2, 21, 0, 64, 0, 128), 1, ["igemmx<128;128;0;split3>"]),
        ("fwd", (2, 21, 0, 64, 0, 64), 0, ["igemmx<256;64;0;split3>"]),
        ("fwd", (2, 8, 6, 64, 64, 64), 1, ["igemmx<256;64;0;split3>", "igemmx<256;64;1;split3>"]),
        ("bwd", (1, 18, 0, 128, 0, 64), 1, ["igemmx<128;128;1;split3>", "wgrad<3;3;1;split3> buf=1", "wgrad_reduce"]),
        ("bwd", (1, 18, 0, 128, 0, 64), 0, ["igemmx<128;128;1;split3>", "wgrad<3;3;1;split3> buf=0", "wgrad_reduce"]),
        ("up", (1, 7, 128, 64), 1, ["igemmx<128;128;0;split3>", "wgrad<2;2;2;split3> buf=1", "wgrad_reduce"]),
        ("up", (1, 7, 64, 32), 0, ["igemmx<128;128;0;split3>", "igemmx<256;64;0;split3>", "wgrad<2;2;2;split3> buf=0", "wgrad_reduce"])],
    2: [("fwd", (2, 21, 0, 64, 0, 64), 1, ["convb64<8;32> pad=0"]),
        ("bwd", (2, 21, 0, 64, 0, 64), 1, ["convb64<8;32> pad=2", "wgradb<3;3;1> buf=1", "wgrad_reduce"]),
        ("fwd", (1, 21, 0, 128, 0, 128), 1, ["igemmb3<0> OW=19"]),
        ("bwd", (1, 19, 0, 128, 0, 128), 0, ["igemmb3<1> OW=19", "wgradb<3;3;1> buf=1", "wgrad_reduce"]),
        ("fwd", (1, 20, 0, 128, 0, 128), 1, ["igemmb<128;128;0>"]),             # OW = 18: below the band kernel's 19
        ("fwd", (1, 14, 0, 128, 0, 64), 1, ["igemmb<256;64;0>"]),
        ("bwd", (2, 13, 0, 128, 0, 256), 1, ["igemmb<128;128;1>", "wgradb<3;3;1> buf=1", "wgrad_reduce"]),
        ("bwd", (1, 14, 0, 64, 0, 128), 1, ["igemmb<256;64;1>", "wgradb<3;3;1> buf=1", "wgrad_reduce"]),
        ("up", (1, 7, 128, 64), 0, ["igemmb<128;128;0>", "wgrad_up<bf16>", "wgrad_reduce"])],
}

# every family the dispatch code offers in each mode for the 3x3 and up-conv per-op entry points (mode 3 = Winograd plus every
# fallback of mode 0's kernels: implicit GEMM where wino_applicable fails, the exact weight gradient where wgradw_applicable does)
FP32 = {"igemm<128;128;0>", "igemm<128;128;1>", "igemm<256;64;0>", "igemm<256;64;1>", "wgrad<3;3;1;split0>", "wgrad<2;2;2;split0>",
        "wgrad_up<f32>", "wgrad_reduce"}
COMPLETE = {
    0: FP32,
    3: FP32 | {"wino32<0>", "wino32<1>", "wgradw<0>", "wgradw<1>", "wgradw_reduce"},
    1: {"igemmx<128;128;0;split3>", "igemmx<128;128;1;split3>", "igemmx<256;64;0;split3>", "igemmx<256;64;1;split3>", "wgrad<3;3;1;split3>",
        "wgrad<2;2;2;split3>", "wgrad_reduce"},
    2: {"convb64<8;32>", "igemmb3<0>", "igemmb3<1>", "igemmb<128;128;0>", "igemmb<128;128;1>", "igemmb<256;64;0>", "igemmb<256;64;1>",
        "wgradb<3;3;1>", "wgrad_up<bf16>", "wgrad_reduce"},
}

# families of the dispatch code the per-op ABI cannot reach with legal shapes, and why
UNREACHABLE = {
    3: {"wino fallback cdiv(OH, 2) < 7 alone": "per-op tiles are square (H == W, checked), so OH < 13 implies OW < 13, which the "
        "cdiv(OW, 2) < 9 test already sends to the implicit GEMM first"},
    0: {"wgrad<2;2;2;split0> buf=1": "at lds_dma = 1 every full-window up-conv takes the pixel-linear kernel (up_applicable) unless a "
        "tensor is >= 2 GiB, which then also forbids buffer staging"},
    1: {"wgrad_up<f32>": "bf16x3 keeps the row-walking kernel (up_applicable)"},
}


@pytest.mark.parametrize("mode", [0, 3, 1, 2])
def test_path_coverage(hip, mode):
    seen = set()
    groups = []
    for op, args, dma, expect in TABLES[mode]:
        rec, out, ref = run_op(hip, mode, dma, op, args)
        main = {f for f, r in zip(rec.families, rec.rows) if r["kind"] in MAIN_KINDS}
        for spec in expect:
            assert rec.reached(spec), "mode %d %s %s lds_dma=%d: expected %r, got %r" % (mode, op, args, dma, spec, rec.tags)
        assert main <= COMPLETE[mode], "mode %d %s %s: families outside the mode's set: %r" % (mode, op, args, main - COMPLETE[mode])
        parity(mode, out, ref)
        seen |= main
        groups += [int(f["groups"]) for fam in set(rec.families) if fam.startswith("wgrad") and not fam.startswith("wgradw")
                   for f in rec.fields(fam) if "groups" in f]
    assert seen == COMPLETE[mode], "mode %d: not reached %r" % (mode, COMPLETE[mode] - seen)
    if mode == 0:
        assert max(groups) >= 64 and min(groups) < 64          # both widths of wgrad_reduce (nP >= 64 -> 16 lanes per slab)


# (op, args): every per-op path whose kernels read the staging knob, per mode
IDENTITY_CASES = [("fwd", (2, 21, 0, 64, 0, 128)), ("fwd", (2, 21, 0, 64, 0, 64)), ("fwd", (2, 8, 6, 64, 64, 64)), ("fwd", (2, 30, -3, 64, 64, 128)),
                  ("bwd", (1, 18, 0, 64, 0, 128)), ("bwd", (2, 13, 0, 128, 0, 256)), ("bwd", (2, 8, 6, 64, 64, 64)), ("bwd", (2, 20, 0, 64, 0, 64)),
                  ("up", (1, 7, 128, 64)), ("up", (2, 32, 64, 64))]
IDENTITY_32 = [("fwd", (2, 20, 0, 32, 0, 32)), ("bwd", (2, 20, 0, 32, 0, 32)), ("bwd", (1, 12, 3, 32, 32, 64))]


@pytest.mark.parametrize("mode", [0, 3, 1, 2])
def test_lds_dma_is_bit_identical(hip, mode):
    """unet_set_lds_dma(1) and (0) give the same bits for every output - except the fp32 up-conv weight and bias gradient
    (modes 0 and 3), which moves from the pixel-linear kernel to the row-walking one and sums in another order
    (include/unet_hip.h); that pair is held to the fp32 parity bound instead."""
    cases = IDENTITY_CASES + (IDENTITY_32 if mode != 2 else [])
    for op, args in cases:
        r1, o1, ref = run_op(hip, mode, 1, op, args)
        r0, o0, _ = run_op(hip, mode, 0, op, args)
        for n in o1:
            if op == "up" and n in ("dw", "db") and mode in (0, 3):
                assert "wgrad_up<f32>" in r1.families and r0.reached("wgrad<2;2;2;split0> buf=0")
                assert nerr(o0[n], ref[n][0]) < 2e-5 and nerr(o1[n], ref[n][0]) < 2e-5
                print("mode %d up %s %s: pixel-linear vs row-walking %s" % (mode, args, n, "bit-identical" if torch.equal(o0[n], o1[n]) else
                                                                         "differ by %.3g (normalised)" % nerr(o0[n], o1[n])))
                continue
            assert torch.equal(o1[n], o0[n]), "mode %d %s %s: %s differs between lds_dma 1 (%r) and 0 (%r)" % (mode, op, args, n, r1.families, r0.families)
