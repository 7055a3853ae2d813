"""Per-op tests of the layer-side memory-bound kernels of csrc/direct.hip through the C ABI: the conv11c forward, its weight
and bias gradient (with the reduce) and its input gradient, the 2 x 2 max-pool forward and backward, and the stand-alone bias
gradient that unet_conv3x3_bwd / unet_upconv2_bwd run when db is asked for without dw or over a padded single source; with them
the optional outputs of those two entry points, the single source with a signed pad and the rectangular up-conv forward.
References, data, bounds and shape lists are tests/layer_ref.py's, proved well-posed without a device by
tests/test_layer_ref_cpu.py.

Every pointer handed to the library comes from a guarded.Arena (tests/guarded.py): scratch is exact to the byte,
mem.verify(outputs...) after every call = every element written, every guard intact; an output passed as NULL has a poisoned
buffer beside it that must stay poison.  The kernel that ran is pinned through kernel_paths.record().  Both storage types run:
fp32 (arithmetic mode 3) and bf16 (mode 2).

Two kinds of data.  Exact: small integers (image and weights in [-4, 4], gradients in [-8, 8], all exact in bf16) with
max(A) < 2^24 asserted first, so every fp32 partial sum is an exact integer in any order and the result must equal the
reference bit for bit: one dropped or doubled row shows at any term count.  Random: gpu_support.rnd with exact zeros planted,
held per element to layer_ref.bound (Higham's bound for a sum in any order, derived there); the worst error / bound of each
case is printed."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded as gd
import kernel_paths as kp
import layer_ref as lr
from gpu_support import hip, math_mode, nerr, rejected, rnd, still_poison

pytestmark = pytest.mark.gpu

ADT = {4: torch.float32, 2: torch.bfloat16}


@pytest.fixture(params=[4, 2], ids=["fp32", "bf16"])
def es(hip, math_mode, request):
    """Element size of the activation tensors: 4 = fp32 (arithmetic mode 3), 2 = bf16 (mode 2)."""
    math_mode(3 if request.param == 4 else 2)
    return request.param


def dev(mem, a, dtype=torch.float32, label=None):
    """numpy array -> guarded device tensor of `dtype`"""
    return mem.inp(torch.from_numpy(np.ascontiguousarray(a)).to(dtype), label)


def seen(t):
    """What a kernel reads of a device tensor, as float64 numpy (a bf16 tensor holds rounded values)."""
    return t.float().cpu().numpy().astype(np.float64)


def host(t):
    return t.float().cpu().numpy()


def randn(seed, shape, scale=1.0, zeros=True):
    a = (rnd(*shape, seed=seed, fp32=True) * scale).numpy().astype(np.float32)
    return lr.plant_zeros(a, seed + 100) if zeros else a


def families(rec, kind):
    return [f for f, r in zip(rec.families, rec.rows) if r["kind"] == kind]


def same_bits(got, ref, what):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    bad = lr.bits(got) != lr.bits(ref)
    assert not bad.any(), "%s: %d of %d elements differ from the exact result, first at %s: %r != %r" % (
        what, bad.sum(), bad.size, tuple(int(i) for i in np.argwhere(bad)[0]), got[bad][0], ref[bad][0])


def within(got, ref, bnd, what):
    r = lr.ratio(got, ref, bnd)
    print("%s: worst error / bound %.3g" % (what, r))
    assert r <= 1.0, "%s: error / bound %.3g" % (what, r)
    return r


# ---- conv11c forward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,K", lr.FWD_CASES, ids=["B%d-S%d-K%d" % c for c in lr.FWD_CASES])
def test_conv11c_fwd(hip, es, B, S, K):
    """A partial pass (So < pixels per pass), ragged passes for both lanes-per-pixel values, rows that cross images, and
    (B = 1030) more rows than the 2048-workgroup grid."""
    L = hip.lib()
    So = S - 2
    for kind in ("exact", "random"):
        if kind == "exact":
            x, w, b = lr.ints(1, (B, S, S), 4), lr.ints(2, (K, 3, 3), 4), lr.ints(3, (K,), 4)
        else:
            x, w, b = randn(1, (B, S, S)), randn(2, (K, 3, 3), 0.5, zeros=False), randn(3, (K,), zeros=False)
        ref, A = lr.conv11c_fwd(x, w, b)
        mem = gd.Arena()
        y = mem.out((B, So, So, K), ADT[es], "y")
        with kp.record(L) as rec:
            hip.check(L.unet_conv1ch_fwd(mem.ptr(dev(mem, x)), B, S, mem.ptr(dev(mem, w)), mem.ptr(dev(mem, b)), K, mem.ptr(y), hip.stream()), "conv1ch_fwd")
        mem.verify(y)
        assert families(rec, kp.K_CONV11C) == ["conv1ch_fwd"] and len(rec.rows) == 1, rec
        what = "conv11c fwd %s B=%d S=%d K=%d %s" % (ADT[es], B, S, K, kind)
        if kind == "exact":
            assert A.max() < lr.EXACT_LIMIT and ref.max() <= 256
            same_bits(host(y), ref, what)
        else:
            assert (ref == 0).any() and (ref > 0).any()
            within(host(y), ref, lr.bound(9, A, ref, bf16_out=es == 2), what)


# ---- conv11c weight and bias gradient ---------------------------------------------------------------------------------------
def wgrad_call(hip, es, x, dz, B, S, K, want_dw=True, want_db=True):
    """One unet_conv1ch_bwd on Arena buffers with exact scratch; returns (dw, db, what dz the kernel saw)."""
    L = hip.lib()
    mem = gd.Arena()
    dzd = dev(mem, dz, ADT[es], "dz")
    dw = mem.out((K, 3, 3), torch.float32, "dw"); db = mem.out((K,), torch.float32, "db")
    nbytes = L.unet_conv1ch_bwd_scratch_bytes(B, S, K)
    assert nbytes == lr.conv11c_wgrad_scratch_bytes(B, S, K)
    sc = mem.scratch(nbytes, "conv1ch_bwd scratch")
    with kp.record(L) as rec:
        hip.check(L.unet_conv1ch_bwd(mem.ptr(dev(mem, x)), B, S, K, mem.ptr(dzd), mem.ptr(dw) if want_dw else None, mem.ptr(db) if want_db else None,
                                     mem.ptr(sc), hip.stream()), "conv1ch_bwd")
    mem.verify(dw if want_dw else None, db if want_db else None)
    assert families(rec, kp.K_CONV11C) == ["conv1ch_wgrad"] and len(rec.rows) == 1, rec
    assert want_dw or still_poison(dw)
    assert want_db or still_poison(db)
    return host(dw), host(db), dzd


def wgrad_exact(hip, es, B, S, K, subsets):
    x, dz = lr.ints(1, (B, S, S), 4), lr.ints(2, (B, S - 2, S - 2, K), 8)
    dw_ref, Aw, db_ref, Ab = lr.conv11c_wgrad(x, dz)
    assert max(Aw.max(), Ab.max()) < lr.EXACT_LIMIT
    for want_dw, want_db in subsets:
        dw, db, _ = wgrad_call(hip, es, x, dz, B, S, K, want_dw, want_db)
        what = "conv11c wgrad %s B=%d S=%d K=%d exact (dw %d, db %d)" % (ADT[es], B, S, K, want_dw, want_db)
        if want_dw:
            same_bits(dw, dw_ref, what + " dw")
        if want_db:
            same_bits(db, db_ref, what + " db")


@pytest.mark.parametrize("B,S,K", lr.WGRAD_CASES, ids=["B%d-S%d-K%d" % c for c in lr.WGRAD_CASES])
def test_conv11c_wgrad(hip, es, B, S, K):
    """2, 64, 66 and 1024 partial vectors (around the reduce's 64 lanes), 1026 and 2050 rows (rows per block 2 and 3, the last
    block short), larger tiles, and for K = 32 either side of the LDS switch at 3 S = 40 K.  dw alone, db alone and both."""
    wgrad_exact(hip, es, B, S, K, [(True, True), (True, False), (False, True)])
    x, dz = randn(1, (B, S, S)), randn(2, (B, S - 2, S - 2, K))
    dw, db, dzd = wgrad_call(hip, es, x, dz, B, S, K)
    dw_ref, Aw, db_ref, Ab = lr.conv11c_wgrad(x, seen(dzd))
    n = B * (S - 2) ** 2
    what = "conv11c wgrad %s B=%d S=%d K=%d random" % (ADT[es], B, S, K)
    within(dw, dw_ref, lr.bound(n, Aw), what + " dw")
    within(db, db_ref, lr.bound(n, Ab), what + " db")


def test_conv11c_wgrad_large(hip, es):
    """S = 856, K = 64: the staged rows, not the reduction, size the LDS (3 S > 40 K); 729316 terms per sum, exact."""
    wgrad_exact(hip, es, *lr.WGRAD_LARGE, [(True, True)])


# ---- conv11c input gradient -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,K", lr.DGRAD_CASES, ids=["B%d-S%d-K%d" % c for c in lr.DGRAD_CASES])
def test_conv11c_dgrad(hip, es, B, S, K):
    L = hip.lib()
    for kind in ("exact", "random"):
        if kind == "exact":
            dz, w = lr.ints(1, (B, S - 2, S - 2, K), 8), lr.ints(2, (K, 3, 3), 4)
        else:
            dz, w = randn(1, (B, S - 2, S - 2, K)), randn(2, (K, 3, 3), 0.5)
        mem = gd.Arena()
        dzd = dev(mem, dz, ADT[es], "dz")
        dx = mem.out((B, S, S), torch.float32, "dx")
        with kp.record(L) as rec:
            hip.check(L.unet_conv1ch_dgrad(mem.ptr(dzd), B, S, K, mem.ptr(dev(mem, w)), mem.ptr(dx), hip.stream()), "conv1ch_dgrad")
        mem.verify(dx)
        assert families(rec, kp.K_CONV11C) == ["conv1ch_dgrad"] and len(rec.rows) == 1, rec
        ref, A = lr.conv11c_dgrad(seen(dzd), w)
        what = "conv11c dgrad %s B=%d S=%d K=%d %s" % (ADT[es], B, S, K, kind)
        if kind == "exact":
            assert A.max() < lr.EXACT_LIMIT
            same_bits(host(dx), ref, what)
        else:
            within(host(dx), ref, lr.bound(9 * K, A), what)


# ---- 2 x 2 max-pool ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(lr.POOL_CASES)), ids=["%dx%dx%dx%d" % c for c in lr.POOL_CASES])
def test_maxpool2_bit_exact(hip, es, case):
    """H != W, C / 4 = 1, 3, 15, 16, 32, 256, thread totals 255, 256 and 257; values from a small set with 0.0, -0.0 and
    negatives, every tie pattern planted (layer_ref.POOL_PATTERNS).  A selection: forward and backward bit for bit."""
    L = hip.lib()
    B, H, W, C = lr.POOL_CASES[case]
    pre, dy, _ = lr.pool_case(10 + case, B, H, W, C)
    mem = gd.Arena()
    y = mem.out((B, H // 2, W // 2, C), ADT[es], "y"); dpre = mem.out((B, H, W, C), ADT[es], "dpre")
    xd = dev(mem, pre, ADT[es], "pre")
    with kp.record(L) as rec:
        hip.check(L.unet_maxpool2_fwd(mem.ptr(xd), mem.ptr(y), B, H, W, C, hip.stream()), "maxpool2_fwd")
        hip.check(L.unet_maxpool2_bwd(mem.ptr(xd), mem.ptr(dev(mem, dy, ADT[es], "dy")), mem.ptr(dpre), B, H, W, C, hip.stream()), "maxpool2_bwd")
    mem.verify(y, dpre)
    assert rec.families == ["maxpool2_fwd", "maxpool2_bwd"], rec
    same_bits(host(y), lr.maxpool2_fwd(pre), "maxpool2_fwd %s %s" % (ADT[es], (B, H, W, C)))
    same_bits(host(dpre), lr.maxpool2_bwd(pre, dy), "maxpool2_bwd %s %s" % (ADT[es], (B, H, W, C)))


# ---- stand-alone bias gradient ----------------------------------------------------------------------------------------------
def conv_db_alone(hip, es, dz, B, H, C, K):
    """unet_conv3x3_bwd(dx = NULL, dw = NULL, db) on Arena buffers; returns (db, record, the dz the kernel saw)."""
    L = hip.lib()
    mem = gd.Arena()
    dzd = dev(mem, dz, ADT[es], "dz")
    x = dev(mem, np.zeros((B, H, H, C), np.float32), ADT[es], "x"); w = dev(mem, np.zeros((K, C, 3, 3), np.float32), label="w")
    db = mem.out((K,), torch.float32, "db")
    sc = mem.scratch(L.unet_conv3x3_bwd_scratch_bytes(B, H, H, C, K), "conv3x3_bwd scratch")
    with kp.record(L) as rec:
        hip.check(L.unet_conv3x3_bwd(mem.ptr(x), H, H, C, 0, None, 0, B, H, H, mem.ptr(w), K, mem.ptr(dzd), None, None, None, None, None, None,
                                     mem.ptr(db), mem.ptr(sc), hip.stream()), "conv3x3_bwd (db alone)")
    mem.verify(db)
    return host(db), rec, dzd


BIAS_CASES = [(e, B, H, K) for e in (4, 2) for B, H in lr.BIAS_SHAPES for K in lr.BIAS_K[e]]


@pytest.mark.parametrize("e,B,H,K", BIAS_CASES, ids=["%s-B%d-H%d-K%d" % ((("fp32", "bf16")[c[0] == 2],) + c[1:]) for c in BIAS_CASES])
def test_bias_grad_alone(hip, math_mode, e, B, H, K):
    """M = 1 ... 18432 rows: one row, either side of the 2048-row block, 2, 5 and 9 partial rows for the reduce (its unroll by
    four and the tail); K = 96 leaves 16 threads of the block idle (10 row slots), K = 1024 has one slot."""
    math_mode(3 if e == 4 else 2)
    Ho = H - 2
    M = B * Ho * Ho
    for kind in ("exact", "random"):
        dz = lr.ints(1, (B, Ho, Ho, K), 8) if kind == "exact" else randn(1, (B, Ho, Ho, K))
        db, rec, dzd = conv_db_alone(hip, e, dz, B, H, 32, K)
        assert rec.families == ["bias_grad"], rec
        ref, A = lr.column_sums(seen(dzd))
        what = "bias_grad %s M=%d K=%d %s" % (ADT[e], M, K, kind)
        if kind == "exact":
            assert A.max() < lr.EXACT_LIMIT
            same_bits(db, ref, what)
        else:
            within(db, ref, lr.bound(M, A), what)


def test_bias_grad_alone_vs_riding_conv(hip, es):
    """db from the stand-alone kernel and db riding on the weight-gradient launch: each within the bound of the fp64 sum, so
    within twice the bound of each other; bias_grad runs only when nothing carries db."""
    L = hip.lib()
    B, H, C, K = 7, 19, 64, 64
    Ho = H - 2
    dz = randn(1, (B, Ho, Ho, K))
    alone, rec, dzd = conv_db_alone(hip, es, dz, B, H, C, K)
    assert rec.families == ["bias_grad"], rec
    mem = gd.Arena()
    x = dev(mem, randn(2, (B, H, H, C)), ADT[es], "x"); w = dev(mem, randn(3, (K, C, 3, 3), 0.05), label="w")
    dw = mem.out((K, C, 3, 3), torch.float32, "dw"); db = mem.out((K,), torch.float32, "db")
    sc = mem.scratch(L.unet_conv3x3_bwd_scratch_bytes(B, H, H, C, K))
    with kp.record(L) as rec:
        hip.check(L.unet_conv3x3_bwd(mem.ptr(x), H, H, C, 0, None, 0, B, H, H, mem.ptr(w), K, mem.ptr(dev(mem, dz, ADT[es], "dz")), None, None, None, None, None,
                                     mem.ptr(dw), mem.ptr(db), mem.ptr(sc), hip.stream()), "conv3x3_bwd (dw, db)")
    mem.verify(dw, db)
    assert "bias_grad" not in rec.families and rec.main_families(reduces=False) == [kp.wgrad_family(3 if es == 4 else 2, 1, C, K)], rec
    ref, A = lr.column_sums(seen(dzd))
    bnd = lr.bound(B * Ho * Ho, A)
    within(alone, ref, bnd, "conv db alone %s" % ADT[es])
    within(host(db), ref, bnd, "conv db riding %s" % ADT[es])
    assert np.all(np.abs(alone.astype(np.float64) - host(db)) <= 2 * bnd)


@pytest.mark.parametrize("B,H,Ci,Co", lr.BIAS_UP_CASES)
def test_bias_grad_upconv(hip, es, B, H, Ci, Co):
    """unet_upconv2_bwd(dx = NULL, dw = NULL, db): the column sums of dy as 4 B H^2 rows of Co; and, where the weight gradient
    takes the shape (the bf16 one needs whole 64-channel tiles), db riding on it."""
    L = hip.lib()
    M = 4 * B * H * H
    out = {}
    can_ride = es == 4 or Co % 64 == 0
    for kind, ride in (("exact", False), ("random", False)) + ((("random", True),) if can_ride else ()):
        dy = lr.ints(1, (B, 2 * H, 2 * H, Co), 8) if kind == "exact" else randn(1, (B, 2 * H, 2 * H, Co))
        mem = gd.Arena()
        dyd = dev(mem, dy, ADT[es], "dy")
        x = dev(mem, np.maximum(randn(2, (B, H, H, Ci)), 0), ADT[es], "x"); w = dev(mem, randn(3, (Ci, Co, 2, 2), 0.05), label="w")
        dw = mem.out((Ci, Co, 2, 2), torch.float32, "dw"); db = mem.out((Co,), torch.float32, "db")
        sc = mem.scratch(L.unet_upconv2_scratch_bytes(B, H, H, max(Ci, 64), max(Co, 64)))
        with kp.record(L) as rec:
            hip.check(L.unet_upconv2_bwd(mem.ptr(x), B, H, H, Ci, mem.ptr(w), Co, mem.ptr(dyd), None, None, mem.ptr(dw) if ride else None, mem.ptr(db),
                                         mem.ptr(sc), hip.stream()), "upconv2_bwd")
        mem.verify(dw if ride else None, db)
        assert ride or still_poison(dw)
        assert rec.families == ["bias_grad"] if not ride else "bias_grad" not in rec.families and len(rec.main_families()) >= 1, rec
        ref, A = lr.column_sums(seen(dyd))
        what = "upconv db %s M=%d Co=%d %s%s" % (ADT[es], M, Co, kind, " riding" if ride else "")
        if kind == "exact":
            assert A.max() < lr.EXACT_LIMIT
            same_bits(host(db), ref, what)
        else:
            bnd = lr.bound(M, A)
            within(host(db), ref, bnd, what)
            out[ride] = host(db).astype(np.float64)
    assert not can_ride or np.all(np.abs(out[True] - out[False]) <= 2 * bnd)


# ---- optional outputs of unet_conv3x3_bwd / unet_upconv2_bwd ----------------------------------------------------------------
def conv_bwd_subset(hip, es, args, data, want):
    """One unet_conv3x3_bwd with the outputs named in `want` (of dx1, dx2, dw, db); every output buffer is allocated, the
    ones not asked for must stay poison.  Returns ({name: host array}, record)."""
    L = hip.lib()
    B, Hs, pad, C1, C2, K = args
    H = Hs + 2 * pad
    a, u, w, dz = data
    mem = gd.Arena()
    ad = dev(mem, a, ADT[es], "x1"); ud = dev(mem, u, ADT[es], "x2") if C2 else None
    bufs = {"dx1": mem.out((B, Hs, Hs, C1), ADT[es], "dx1"), "dw": mem.out((K, C1 + C2, 3, 3), torch.float32, "dw"), "db": mem.out((K,), torch.float32, "db")}
    if C2:
        bufs["dx2"] = mem.out((B, H, H, C2), ADT[es], "dx2")
    p = lambda n: mem.ptr(bufs[n]) if n in want else None
    sc = mem.scratch(L.unet_conv3x3_bwd_scratch_bytes(B, H, H, C1 + C2, K))
    with kp.record(L) as rec:
        hip.check(L.unet_conv3x3_bwd(mem.ptr(ad), Hs, Hs, C1, pad, mem.ptr(ud), C2, B, H, H, mem.ptr(dev(mem, w, label="w")), K, mem.ptr(dev(mem, dz, ADT[es], "dz")),
                                     p("dx1"), None, None, p("dx2"), None, p("dw"), p("db"), mem.ptr(sc), hip.stream()), "conv3x3_bwd %s" % sorted(want))
    mem.verify(*[bufs[n] for n in want])
    for n, t in bufs.items():
        assert n in want or still_poison(t), "%s was not requested but written (%s)" % (n, sorted(want))
    return {n: host(bufs[n]) for n in want}, rec


@pytest.mark.parametrize("args", [(1, 20, 0, 64, 0, 64), (1, 12, 4, 64, 64, 64)], ids=["plain", "concat"])
def test_conv3x3_bwd_optional_outputs(hip, es, args):
    """Each subset of {dx (dx1, dx2), dw, db}, and over the concat dx1 and dx2 alone: what is requested is bit-identical to the
    full call, the rest stays poison.  Integer data: db is exact whichever kernel sums it (riding on the weight gradient in the
    full call, bias_grad without dw), so bit-identity holds for it too; bias_grad runs exactly when db is wanted without dw."""
    B, Hs, pad, C1, C2, K = args
    H = Hs + 2 * pad
    data = (lr.ints(1, (B, Hs, Hs, C1), 4), lr.ints(2, (B, H, H, C2), 4) if C2 else None, lr.ints(3, (K, C1 + C2, 3, 3), 4), lr.ints(4, (B, H - 2, H - 2, K), 8))
    dxs = ("dx1", "dx2") if C2 else ("dx1",)
    full, rec = conv_bwd_subset(hip, es, args, data, set(dxs) | {"dw", "db"})
    assert "bias_grad" not in rec.families, rec
    db_ref, A = lr.column_sums(data[3])
    assert A.max() < lr.EXACT_LIMIT
    same_bits(full["db"], db_ref, "db of the full call")
    groups = [set(g) for r in (1, 2) for g in itertools.combinations((dxs, ("dw",), ("db",)), r)]
    subsets = [set().union(*g) for g in groups] + ([{"dx1"}, {"dx2"}] if C2 else [])
    for want in subsets:
        got, rec = conv_bwd_subset(hip, es, args, data, want)
        assert ("bias_grad" in rec.families) == ("db" in want and "dw" not in want), (sorted(want), rec)
        for n in want:
            same_bits(got[n], full[n], "%s of %s" % (n, sorted(want)))


def test_upconv2_bwd_optional_outputs(hip, es):
    L = hip.lib()
    B, H, Ci, Co = 2, 7, 128, 64
    x, w, dy = np.abs(lr.ints(1, (B, H, H, Ci), 4)), lr.ints(2, (Ci, Co, 2, 2), 4), lr.ints(3, (B, 2 * H, 2 * H, Co), 8)

    def call(want):
        mem = gd.Arena()
        xd = dev(mem, x, ADT[es], "x")
        bufs = {"dx": mem.out((B, H, H, Ci), ADT[es], "dx"), "dw": mem.out((Ci, Co, 2, 2), torch.float32, "dw"), "db": mem.out((Co,), torch.float32, "db")}
        p = lambda n: mem.ptr(bufs[n]) if n in want else None
        sc = mem.scratch(L.unet_upconv2_scratch_bytes(B, H, H, Ci, Co))
        with kp.record(L) as rec:
            hip.check(L.unet_upconv2_bwd(mem.ptr(xd), B, H, H, Ci, mem.ptr(dev(mem, w, label="w")), Co, mem.ptr(dev(mem, dy, ADT[es], "dy")), p("dx"), mem.ptr(xd),
                                         p("dw"), p("db"), mem.ptr(sc), hip.stream()), "upconv2_bwd %s" % sorted(want))
        mem.verify(*[bufs[n] for n in want])
        for n, t in bufs.items():
            assert n in want or still_poison(t), "%s was not requested but written (%s)" % (n, sorted(want))
        assert ("bias_grad" in rec.families) == ("db" in want and "dw" not in want), (sorted(want), rec)
        return {n: host(bufs[n]) for n in want}

    full = call({"dx", "dw", "db"})
    same_bits(full["db"], lr.column_sums(dy)[0], "db of the full call")
    for r in (1, 2):
        for want in itertools.combinations(("dx", "dw", "db"), r):
            got = call(set(want))
            for n in want:
                same_bits(got[n], full[n], "%s of %s" % (n, sorted(want)))


# ---- single source with a signed pad ----------------------------------------------------------------------------------------
def act_tol(mode):
    """The per-mode parity tolerances of tests/test_kernel_paths_gpu.py for the same kernels (normalised maximum): fp32
    accumulation 2e-5; bf16 activations 4e-3."""
    return 4e-3 if mode == 2 else 2e-5


@pytest.mark.parametrize("mode", [0, 3, 2])
@pytest.mark.parametrize("pad", [2, -2], ids=["pad+2", "pad-2"])
@pytest.mark.parametrize("B,H1,C,K", [(2, 22, 64, 64), (1, 30, 32, 64)])
def test_conv3x3_single_source_signed_pad(hip, math_mode, mode, pad, B, H1, C, K):
    """x2 = NULL with pad1 = +2 (zero border) and -2 (crop), forward and backward, against fp64 conv2d(F.pad(x, (pad,) * 4)).
    db cannot ride on a weight-gradient launch that misses part of dz, so it is the stand-alone bias_grad.  The bf16 kernels
    take sources of whole 64-channel tiles only: C = 32 in mode 2 is refused before anything is enqueued, pad or no pad."""
    math_mode(mode)
    L = hip.lib()
    e = 2 if mode == 2 else 4
    adt = ADT[e]
    H = H1 + 2 * pad
    Ho = H - 2
    mem = gd.Arena()
    if mode == 2 and C % 64:
        xd = dev(mem, randn(1, (B, H1, H1, C)), adt, "x"); dzd = dev(mem, randn(4, (B, Ho, Ho, K)), adt, "dz")
        wd = dev(mem, randn(2, (K, C, 3, 3), 0.05), label="w"); bd = dev(mem, randn(3, (K,)))
        y = mem.out((B, Ho, Ho, K), adt, "y"); sc = mem.scratch(L.unet_conv3x3_scratch_bytes(C, K))
        rejected(hip, L.unet_conv3x3_fwd(mem.ptr(xd), H1, H1, C, pad, None, 0, B, H, H, mem.ptr(wd), mem.ptr(bd), K, 1, mem.ptr(y), mem.ptr(sc), hip.stream()), mem, y, sc)
        dx = mem.out((B, H1, H1, C), adt, "dx"); dw = mem.out((K, C, 3, 3), torch.float32, "dw"); db = mem.out((K,), torch.float32, "db")
        sc = mem.scratch(L.unet_conv3x3_bwd_scratch_bytes(B, H, H, C, K))
        rejected(hip, L.unet_conv3x3_bwd(mem.ptr(xd), H1, H1, C, pad, None, 0, B, H, H, mem.ptr(wd), K, mem.ptr(dzd), mem.ptr(dx), None, None, None, None,
                                         mem.ptr(dw), mem.ptr(db), mem.ptr(sc), hip.stream()), mem, dx, dw, db, sc)
        return
    xd = dev(mem, randn(1, (B, H1, H1, C)), adt, "x"); dzd = dev(mem, randn(4, (B, Ho, Ho, K)), adt, "dz")
    w32, b32 = randn(2, (K, C, 3, 3), 0.05, zeros=False), randn(3, (K,), zeros=False)
    wq = torch.from_numpy(w32).to(adt).double() if mode == 2 else torch.from_numpy(w32).double()      # mode 2 packs the filters as bf16
    x = torch.from_numpy(seen(xd)).permute(0, 3, 1, 2).requires_grad_(True)
    wq.requires_grad_(True)
    z = F.conv2d(F.pad(x, (pad,) * 4), wq, torch.from_numpy(b32).double())
    dz = torch.from_numpy(seen(dzd)).permute(0, 3, 1, 2)
    z.backward(dz)
    y = mem.out((B, Ho, Ho, K), adt, "y")
    wd = dev(mem, w32, label="w")
    with kp.record(L) as rec:
        hip.check(L.unet_conv3x3_fwd(mem.ptr(xd), H1, H1, C, pad, None, 0, B, H, H, mem.ptr(wd), mem.ptr(dev(mem, b32)), K, 1, mem.ptr(y),
                                     mem.ptr(mem.scratch(L.unet_conv3x3_scratch_bytes(C, K))), hip.stream()), "conv3x3_fwd")
    mem.verify(y)
    assert rec.main_families() == [kp.single_pad_fwd_family(mode, 1, H1, pad, C, K)], rec
    ey = nerr(y.float().permute(0, 3, 1, 2), F.relu(z.detach()))
    dx = mem.out((B, H1, H1, C), adt, "dx"); dw = mem.out((K, C, 3, 3), torch.float32, "dw"); db = mem.out((K,), torch.float32, "db")
    with kp.record(L) as rec:
        hip.check(L.unet_conv3x3_bwd(mem.ptr(xd), H1, H1, C, pad, None, 0, B, H, H, mem.ptr(wd), K, mem.ptr(dzd), mem.ptr(dx), None, None, None, None,
                                     mem.ptr(dw), mem.ptr(db), mem.ptr(mem.scratch(L.unet_conv3x3_bwd_scratch_bytes(B, H, H, C, K))), hip.stream()), "conv3x3_bwd")
    mem.verify(dx, dw, db)
    assert rec.main_families(reduces=False) == kp.single_pad_bwd_families(mode, 1, H1, pad, C, K), rec
    assert rec.families.count("bias_grad") == 1, rec
    edx, edw = nerr(dx.float().permute(0, 3, 1, 2), x.grad), nerr(dw, wq.grad)
    print("single source pad %+d mode %d %s: normalised errors y %.3g, dx %.3g, dw %.3g" % (pad, mode, (B, H1, C, K), ey, edx, edw))
    assert ey < act_tol(mode) and edx < act_tol(mode) and edw < 2e-5
    ref, A = lr.column_sums(seen(dzd))
    within(host(db), ref, lr.bound(B * Ho * Ho, A), "single source pad %+d mode %d db" % (pad, mode))
    if pad < 0:                                                     # the cropped border of the source gets no gradient at all
        g = host(dx)
        ring = np.ones((H1, H1), bool); ring[-pad:H1 + pad, -pad:H1 + pad] = False
        assert np.all(g[:, ring] == 0)


# ---- rectangular up-conv forward --------------------------------------------------------------------------------------------
def test_upconv2_fwd_rectangular(hip, es):
    """unet_upconv2_bwd takes square tiles only; the forward takes H and W separately and must be right for H != W."""
    L = hip.lib()
    B, H, W, Ci, Co = 2, 5, 9, 64, 32
    mem = gd.Arena()
    xd = dev(mem, randn(1, (B, H, W, Ci)), ADT[es], "x")
    w32, b32 = randn(2, (Ci, Co, 2, 2), 0.05, zeros=False), randn(3, (Co,), zeros=False)
    wq = torch.from_numpy(w32).to(ADT[es]).double()
    ref = F.conv_transpose2d(torch.from_numpy(seen(xd)).permute(0, 3, 1, 2), wq, torch.from_numpy(b32).double(), stride=2)
    y = mem.out((B, 2 * H, 2 * W, Co), ADT[es], "y")
    sc = mem.scratch(L.unet_upconv2_scratch_bytes(B, H, W, max(Ci, 64), max(Co, 64)))
    with kp.record(L) as rec:
        hip.check(L.unet_upconv2_fwd(mem.ptr(xd), B, H, W, Ci, mem.ptr(dev(mem, w32, label="w")), mem.ptr(dev(mem, b32)), Co, mem.ptr(y), mem.ptr(sc), hip.stream()),
                  "upconv2_fwd")
    mem.verify(y)
    assert rec.main_families() == ["igemm%s<128;128;0>" % ("b" if es == 2 else "")], rec
    e = nerr(y.float().permute(0, 3, 1, 2), ref)
    print("upconv2_fwd %dx%d %s: normalised error %.3g" % (H, W, ADT[es], e))
    assert e < act_tol(2 if es == 2 else 3)


# ---- rejections -------------------------------------------------------------------------------------------------------------
def test_rejections(hip, es):
    """A size or width the kernels do not take returns an error before any launch: nothing is written."""
    L = hip.lib()
    mem = gd.Arena()
    x = dev(mem, np.zeros((1, 8, 8), np.float32)); w = dev(mem, np.zeros((64, 3, 3), np.float32)); b = dev(mem, np.zeros(64, np.float32))
    y = mem.out((1, 6, 6, 64), ADT[es], "y"); dz = dev(mem, np.zeros((1, 6, 6, 64), np.float32), ADT[es])
    dw = mem.out((64, 3, 3), torch.float32, "dw"); db = mem.out((64,), torch.float32, "db"); dx = mem.out((1, 8, 8), torch.float32, "dx")
    sc = mem.scratch(L.unet_conv1ch_bwd_scratch_bytes(1, 8, 64))
    for S, K in ((6, 64), (8, 48)):
        rejected(hip, L.unet_conv1ch_fwd(mem.ptr(x), 1, S, mem.ptr(w), mem.ptr(b), K, mem.ptr(y), hip.stream()), mem, y)
        rejected(hip, L.unet_conv1ch_bwd(mem.ptr(x), 1, S, K, mem.ptr(dz), mem.ptr(dw), mem.ptr(db), mem.ptr(sc), hip.stream()), mem, dw, db, sc)
    rejected(hip, L.unet_conv1ch_dgrad(mem.ptr(dz), 1, 8, 48, mem.ptr(w), mem.ptr(dx), hip.stream()), mem, dx)
    pre = dev(mem, np.zeros((1, 6, 6, 8), np.float32), ADT[es]); dy = dev(mem, np.zeros((1, 3, 3, 8), np.float32), ADT[es])
    py = mem.out((1, 3, 3, 8), ADT[es], "pooled"); dpre = mem.out((1, 6, 6, 8), ADT[es], "dpre")
    for H, W, C in ((5, 6, 8), (6, 5, 8), (6, 6, 6)):
        rejected(hip, L.unet_maxpool2_fwd(mem.ptr(pre), mem.ptr(py), 1, H, W, C, hip.stream()), mem, py)
        rejected(hip, L.unet_maxpool2_bwd(mem.ptr(pre), mem.ptr(dy), mem.ptr(dpre), 1, H, W, C, hip.stream()), mem, dpre)
    # a single source whose padded extent is not the input extent, forward and backward
    c = dev(mem, np.zeros((1, 8, 8, 64), np.float32), ADT[es]); cw = dev(mem, np.zeros((64, 64, 3, 3), np.float32))
    cy = mem.out((1, 8, 8, 64), ADT[es], "conv y"); cdb = mem.out((64,), torch.float32, "conv db")
    rejected(hip, L.unet_conv3x3_fwd(mem.ptr(c), 8, 8, 64, 2, None, 0, 1, 10, 10, mem.ptr(cw), mem.ptr(b), 64, 1, mem.ptr(cy),
                                     mem.ptr(mem.scratch(L.unet_conv3x3_scratch_bytes(64, 64))), hip.stream()), mem, cy)
    rejected(hip, L.unet_conv3x3_bwd(mem.ptr(c), 8, 8, 64, 2, None, 0, 1, 10, 10, mem.ptr(cw), 64, mem.ptr(cy), None, None, None, None, None, None,
                                     mem.ptr(cdb), mem.ptr(mem.scratch(L.unet_conv3x3_bwd_scratch_bytes(1, 10, 10, 64, 64))), hip.stream()), mem, cdb)
