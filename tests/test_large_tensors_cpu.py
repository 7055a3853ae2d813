"""tests/large_ref.py checked without a device, at shapes of a few hundred pixels: the generators keep their bounds, fp32
evaluations of the direct and of the Winograd forms equal fp64 bit for bit on that data (the premise of every exact
comparison in tests/test_large_tensors_gpu.py), the references agree with torch's own convolutions, the sampler always
holds the straddling pixels, and the sampled reference finds one wrong element planted at each kind of strategic position
- and misses it when the sampler drops those pixels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_bounds as kb
import large_ref as lg

B, H, C, K = 3, 14, 8, 8
Ho = H - 2


def data(seed=0, dtype=torch.float32, thin=True):
    g = lg.gen("cpu", seed)
    x = lg.ints(torch.empty(B, H, H, C, dtype=dtype), lg.XMAX, g)
    w = lg.ints(torch.empty(K, C, 3, 3), lg.WMAX, g)
    b = lg.ints(torch.empty(K), lg.BMAX, g)
    dz = lg.ints(torch.empty(B, Ho, Ho, K, dtype=dtype), lg.DZMAX, g)
    add = lg.ints(torch.empty(B, H, H, C, dtype=dtype), lg.AMAX, g)
    mask = lg.bits01(torch.empty(B, H, H, C, dtype=dtype), g)
    return x, w, b, dz, add, mask


def nchw(t):
    return t.double().permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- generators -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generators_keep_their_bounds(dtype):
    x, w, b, dz, add, mask = data(dtype=dtype)
    for t, m in ((x, lg.XMAX), (w, lg.WMAX), (b, lg.BMAX), (dz, lg.DZMAX), (add, lg.AMAX)):
        v = t.double()
        assert bool((v == v.round()).all()) and float(v.abs().max()) <= m, "integers within the stated bound"
        assert t.numel() < 100 or (float(v.max()) == m and float(v.min()) == -m), "which both ends reach"
        assert bool((t.to(torch.bfloat16).double() == v).all()), "exact in bf16 (and so their own first bf16x3 piece)"
    assert set(mask.double().unique().tolist()) == {0.0, 1.0}
    assert lg.direct_bound(128) < lg.EXACT and lg.wino_fwd_bound(128) < lg.EXACT
    # the same seed, the same data; another seed, other data
    assert torch.equal(data()[0], data()[0]) and not torch.equal(data(0)[0], data(1)[0])


def test_thin_keeps_the_density_the_forced_pixels_and_the_bound():
    g = lg.gen("cpu", 5)
    dz = lg.ints(torch.empty(4, 64, 64, 8), lg.DZMAX, g)
    forced = [0, 4095, 3 * 4096, 4 * 4096 - 1, 8191, 8192]
    nz = lg.thin(dz, g, forced, density=2.0 ** -6)
    flat = dz.view(-1, 8)
    assert set(forced) <= set(nz.tolist())
    assert bool((flat[torch.tensor(forced)] != 0).all()), "a forced pixel is non-zero in every channel"
    rest = torch.ones(flat.shape[0], dtype=torch.bool); rest[nz] = False
    assert bool((flat[rest] == 0).all()) and not bool(torch.signbit(flat[rest]).any()), "the others are +0"
    assert 128 <= len(nz) <= 512, "16384 pixels at 1 / 64"
    assert float(flat.abs().max()) <= lg.DZMAX
    assert lg.wgradw_bound(lg.XMAX, flat.abs().sum(0)) < lg.EXACT


# ---- exactness --------------------------------------------------------------------------------------------------------------
def test_fp32_direct_forms_equal_fp64_in_two_orders():
    x, w, b, dz, add, mask = data()
    y64 = lg.direct_fwd(x, w, b, torch.float64)
    assert torch.equal(y64, nhwc(F.conv2d(nchw(x), w.double(), b.double()))), "the loop is the convolution"
    for rev in (False, True):
        y32 = lg.direct_fwd(x, w, b, torch.float32, reverse=rev)
        assert y32.dtype == torch.float32 and torch.equal(y32.double(), y64)
    dw64 = lg.direct_wgrad(x, dz, torch.float64)
    for rev in (False, True):
        assert torch.equal(lg.direct_wgrad(x, dz, torch.float32, reverse=rev).double(), dw64)
    assert float(y64.abs().max()) <= lg.direct_bound(C)


def test_fp32_winograd_forms_equal_fp64():
    x, w, b, dz, add, mask = data()
    y64 = lg.direct_fwd(x, w, b, torch.float64)
    y32 = lg.wino_fwd(x, w, b, torch.float32)
    assert y32.dtype == torch.float32 and torch.equal(y32.double(), y64), "F(2x2, 3x3) in fp32"
    assert torch.equal(lg.wino_fwd(x, w, b, torch.float64), y64)
    dw64 = lg.direct_wgrad(x, dz, torch.float64)
    dw32 = lg.wino_wgrad(x, dz, torch.float32)
    assert dw32.dtype == torch.float32 and torch.equal(dw32.double(), dw64), "F(3x3 <- 2x2) in fp32"
    # the filter transforms produce multiples of 1/4 within the stated range
    g = torch.tensor(lg.G3, dtype=torch.float64)
    U = torch.einsum("ai,kcij,bj->kcab", g, w.double(), g)
    assert bool((4 * U == (4 * U).round()).all()) and float(U.abs().max()) <= 9 * lg.WMAX / 4.0
    g2 = torch.tensor(lg.G2, dtype=torch.float64)
    Z = torch.einsum("ai,...ijk,bj->...abk", g2, lg._tiles(dz.double(), 2, 2), g2)
    assert bool((4 * Z == (4 * Z).round()).all())


def test_rounded_outputs_are_one_rounding_of_the_exact_value():
    """Mode 2: an integer result stored as bf16 is kernel_bounds.rne_bf16 of it, which torch's own conversion agrees with."""
    x, w, b, dz, add, mask = data(dtype=torch.bfloat16)
    big = lg.direct_fwd(x.float(), 37 * w, b, torch.float64)            # (beyond 8 bits, so that rounding happens)
    assert float(big.abs().max()) > 512
    assert np.array_equal(kb.rne_bf16(big.numpy()), big.float().to(torch.bfloat16).double().numpy())


# ---- references -------------------------------------------------------------------------------------------------------------
def test_references_are_the_convolutions():
    x, w, b, dz, add, mask = data()
    dst = (B, Ho, Ho)
    every = torch.arange(B * Ho * Ho)
    y, A = lg.conv_fwd_ref([(x, 0)], w, b, every, dst)
    full = nhwc(F.relu(F.conv2d(nchw(x), w.double(), b.double())))
    assert torch.equal(y, full.reshape(-1, K)) and bool((A >= y.abs()).all())
    # virtual concat: a cropped-in (pad -2 is a crop, +2 a zero border) first source and a full second one
    x1 = lg.ints(torch.empty(B, H - 4, H - 4, C), lg.XMAX, lg.gen("cpu", 9))
    w2 = lg.ints(torch.empty(K, 2 * C, 3, 3), lg.WMAX, lg.gen("cpu", 10))
    y2, _ = lg.conv_fwd_ref([(x1, 2), (x, 0)], w2, b, every, dst)
    cat = torch.cat([F.pad(nchw(x1), (2,) * 4), nchw(x)], 1)
    assert torch.equal(y2, nhwc(F.relu(F.conv2d(cat, w2.double(), b.double()))).reshape(-1, K))
    # backward, through autograd in fp64
    xin = nchw(x).requires_grad_(True)
    wd = w.double().requires_grad_(True)
    bd = b.double().requires_grad_(True)
    F.conv2d(xin, wd, bd).backward(nchw(dz))
    allx = torch.arange(B * H * H)
    dx, _ = lg.conv_dgrad_ref(dz, w, 0, C, allx, (B, H, H), 0)
    assert torch.equal(dx, nhwc(xin.grad).reshape(-1, C))
    dxm, _ = lg.conv_dgrad_ref(dz, w, 0, C, allx, (B, H, H), 0, mask=mask, add=add)
    assert torch.equal(dxm, (nhwc(xin.grad) + add.double()).mul(mask.double()).reshape(-1, C))
    nz = (dz != 0).any(-1).flatten().nonzero().flatten()
    dw, Aw, db, Ab = lg.wgrad_ref(x, 0, dz, nz)
    assert torch.equal(dw, wd.grad) and torch.equal(db, bd.grad) and bool((Aw >= dw.abs()).all())
    # the window of a padded first source: dx1 is the crop of the full gradient
    g1, _ = lg.conv_dgrad_ref(dz, w2, 0, C, torch.arange(B * (H - 4) ** 2), (B, H - 4, H - 4), 2)
    cat2 = cat.clone().requires_grad_(True)
    F.conv2d(cat2, w2.double()).backward(nchw(dz))
    assert torch.equal(g1, nhwc(cat2.grad[:, :C, 2:-2, 2:-2]).reshape(-1, C))


def test_upconv_references_are_the_transposed_convolution():
    g = lg.gen("cpu", 3)
    Ci, Co, h = 8, 4, 5
    x = lg.ints(torch.empty(B, h, h, Ci), lg.XMAX, g).abs_()
    w = lg.ints(torch.empty(Ci, Co, 2, 2), lg.WMAX, g)
    b = lg.ints(torch.empty(Co), lg.BMAX, g)
    dy = lg.ints(torch.empty(B, 2 * h, 2 * h, Co), lg.DZMAX, g)
    xin = nchw(x).requires_grad_(True); wd = w.double().requires_grad_(True); bd = b.double().requires_grad_(True)
    y = F.conv_transpose2d(xin, wd, bd, stride=2)
    y.backward(nchw(dy))
    got, _ = lg.upconv_fwd_ref(x, w, b, torch.arange(B * 4 * h * h), (B, 2 * h, 2 * h))
    assert torch.equal(got, nhwc(y.detach()).reshape(-1, Co))
    allx = torch.arange(B * h * h)
    dx, _ = lg.upconv_dgrad_ref(dy, w, allx, (B, h, h))
    assert torch.equal(dx, nhwc(xin.grad).reshape(-1, Ci))
    dw, _, db, _ = lg.upconv_wgrad_ref(x, dy, allx)
    assert torch.equal(dw, wd.grad) and torch.equal(db, bd.grad)


# ---- sampler ----------------------------------------------------------------------------------------------------------------
# a small tensor with small "limits" in place of 2^31 and 2^32: the arithmetic is the same
LIM = (B * H * H * C * 4 // 3 + 4, B * Ho * Ho * K * 4 * 5 // 9 + 8)


def small_sources():
    return [((B, H, H), C * 4, 0)]


def test_sampler_always_includes_the_strategic_pixels():
    dst = (B, Ho, Ho)
    kinds = lg.strategic(dst, K * 4, small_sources(), LIM)
    n = Ho * Ho
    assert kinds["corner"] == sorted({0, Ho - 1, n - Ho, n - 1, n, 2 * n - 1, 2 * n, 2 * n + Ho - 1, 3 * n - Ho, 3 * n - 1})
    assert kinds["dst"] and kinds["src"] and not set(kinds["dst"]) & set(kinds["corner"])
    # the destination straddlers are neighbours whose byte ranges lie on either side of the limit
    for lim in LIM:
        p = lim // (K * 4)
        if p < B * Ho * Ho:
            assert p in kinds["dst"] and (lim - 1) // (K * 4) in kinds["dst"]
    # every reader of a source straddler really reads it
    q = LIM[0] // (C * 4)
    rd = lg.readers(q, (B, H, H), dst, 0)
    assert rd and set(rd) <= set(kinds["src"])
    x = torch.zeros(B, H, H, C); x.view(-1, C)[q] = 1
    p = lg.gather_patches(x, torch.tensor(rd), dst, 0)
    assert bool((p.sum((1, 2)) == C).all())
    for seed in range(20):
        s = set(lg.sample_pixels(dst, K * 4, small_sources(), seed, n=16, limits=LIM).tolist())
        for kind, px in kinds.items():
            assert set(px) <= s, kind
    # at full size: the real limits, the real shapes
    big = lg.sample_pixels((16, 1024, 1024), 64 * 4, [((16, 1026, 1026), 64 * 4, 0)], 0, n=1 << 10)
    assert len(big) >= 1 << 10 and big.dtype == torch.int64
    full = lg.sample_pixels((16, 1020, 1020), 32 * 4, [((16, 1022, 1022), 32 * 4, 0)], 11)
    assert len(full) >= lg.N_SAMPLES and len(torch.unique(full)) == len(full), "distinct pixels, at least 2^16 of them"
    assert len(lg.sample_pixels((B, Ho, Ho), K * 4, small_sources(), 0, n=400, limits=LIM)) >= 400, "also when most draws repeat"
    want = lg.strategic((16, 1024, 1024), 64 * 4, [((16, 1026, 1026), 64 * 4, 0)])
    assert (1 << 31) // 256 in want["dst"] and (1 << 31) // 256 - 1 in want["dst"] and len(want["src"]) >= 18
    assert set(want["dst"]) | set(want["src"]) <= set(big.tolist())
    assert lg.straddlers(16 * 1024 * 1024, 256) == [(1 << 31) // 256 - 1, (1 << 31) // 256, 16 * 1024 * 1024 - 1], "2^32 is the tensor's end: only the pixel below it"
    assert lg.straddlers(16 * 1026 * 1026, 256)[2:] == [(1 << 32) // 256 - 1, (1 << 32) // 256]


@pytest.mark.parametrize("kind", ["corner", "dst", "src"])
def test_sampled_reference_finds_a_planted_error(kind):
    """One element off by one at a strategic pixel of each kind: the sampled comparison names it; with a sampler that drops
    the straddling pixels, the "dst" and "src" plants go unnoticed (16 random pixels of 432 rarely hit them: the seeds below
    are ones that do not), which is what those pixels are in the sample for."""
    x, w, b, dz, add, mask = data()
    dst = (B, Ho, Ho)
    every = torch.arange(B * Ho * Ho)
    good, _ = lg.conv_fwd_ref([(x, 0)], w, b, every, dst, relu=False)
    y = good.float().reshape(B, Ho, Ho, K)
    kinds = lg.strategic(dst, K * 4, small_sources(), LIM)
    target = kinds[kind][-1]
    pix = lg.sample_pixels(dst, K * 4, small_sources(), 1, n=16, limits=LIM)
    lg.assert_sampled(y, pix, good[pix], "clean")
    bad = y.clone()
    bad.view(-1, K)[target, 3] += 1
    with pytest.raises(AssertionError, match=r"planted: 1 of \d+ sampled elements differ.*first at pixel %d channel 3" % target):
        lg.assert_sampled(bad, pix, good[pix], "planted")
    if kind != "corner":
        seed = next(s for s in range(100) if target not in lg.sample_pixels(dst, K * 4, small_sources(), s, n=16, limits=LIM, keep_strategic=False).tolist())
        blind = lg.sample_pixels(dst, K * 4, small_sources(), seed, n=16, limits=LIM, keep_strategic=False)
        lg.assert_sampled(bad, blind, good[blind], "the broken sampler sees nothing")
        with pytest.raises(AssertionError):
            lg.assert_sampled(bad, lg.sample_pixels(dst, K * 4, small_sources(), seed, n=16, limits=LIM), good[lg.sample_pixels(dst, K * 4, small_sources(), seed, n=16, limits=LIM)], "planted")


def test_assert_sampled_applies_the_expected_rounding_and_rejects_nan():
    ref = torch.tensor([[257.0, 3.0], [-1027.0, 0.0]], dtype=torch.float64)
    got = torch.tensor([[256.0, 3.0], [-1024.0, 0.0]]).to(torch.bfloat16)
    lg.assert_sampled(got, torch.arange(2), ref, "bf16", post=kb.rne_bf16)
    with pytest.raises(AssertionError):
        lg.assert_sampled(got, torch.arange(2), ref, "unrounded")
    nan = torch.tensor([[float("nan"), 3.0]])
    with pytest.raises(AssertionError):
        lg.assert_sampled(nan, torch.arange(1), torch.tensor([[0.0, 3.0]], dtype=torch.float64), "nan")
    assert lg.same_bits(torch.tensor([0.0, 1.0]), torch.tensor([0.0, 1.0])) and not lg.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
