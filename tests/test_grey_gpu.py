"""The grey-value variation on the device (grey.hip: unet_grey_vary, unet_grey_normals; data.grey_variation,
data.augment(grey=...), data.CropDataset(grey=...)) against the fp64 restatement tests/grey_ref.py, which tests/test_grey_cpu.py
pins.  Every buffer handed to the raw entry points is a poisoned guarded.Arena buffer, the scratch of exactly the bytes
unet_grey_scratch_bytes asks for.  The references are computed once per case.

Shapes (the raw op sees a sample as n pixels): n = 37 x 53 = 1961 with B = 3 (n % 4 = 1: the bases of samples 1 and 2 are not
16-byte aligned, so they take the 4-byte accesses, sample 0 the 16-byte ones, and there is a one-pixel tail; two workgroups,
i.e. two partial sums, per sample); n = 64 x 48 = 3072 (all 16-byte accesses, no tail, three workgroups); n = 1, 3, 5 (tail only;
one group plus a tail); B = 65 at n = 7 (two chunks of the 64 samples a call takes).  augment's samples of 236 x 236 pixels
take 55 partials per sample, the timing tool's (tools/grey_time.py) all 64.

The bound.  The device forms a value u_dev in fp64 and narrows it once, so |fp32(u_dev) - u_ref| <= half a spacing of fp32 at
u_dev + |u_dev - u_ref|; asserted is ONE fp32 spacing of the reference value plus an absolute term A >= |u_dev - u_ref|.  With
e = 2^-53, values in [0,1] after the clamp, and the device's pow, log, cos, sin (and sqrt) taken at <= 16 ulp, numpy's at <= 1:
  mean    any order of summation of n fp64 terms errs by <= (n - 1) e sum|x|, the division adds one rounding, and the
          restatement's own np.sum errs too: |m_dev - m_ref| <= (n + 2) e mean|x|                        (kernel_bounds' rule)
  affine  u = (x - m) c + m + b is the same three roundings on both sides (contraction is off in grey.hip), so the two values
          differ by |1 - c| |m_dev - m_ref| plus <= 4 roundings at magnitude V = c (max|x| + |m|) + |m| + |b|:
          E_aff = (n + 2) e mean|x| |1 - c| + 4 e V;  the clamp does not expand it
  gamma   s^g with s = u (or 1 - u): 17 e for the two pow, and E_aff grows by the derivative g s^(g - 1) <= L, where
          L = max(g, g S_MIN^(g - 1)): the case builder asserts that every pixel of a sample whose affine AND gamma stages run
          is either clamped by a margin of 1e-9 (both sides then hold exactly 0 or 1) or has s >= S_MIN = 1e-6
  noise   r = sqrt(-2 log u1) <= R_MAX = sqrt(66 log 2) = 6.77 (u1 >= 2^-33); log at 17 ulp is a relative 8.5 e on r, sqrt one
          more, cos / sin an absolute 17 e: |z_dev - z_ref| <= 28 e R_MAX, times sigma; the product and the sum add 2 roundings
          at magnitude <= 1 + sigma R_MAX
  A = L E_aff + 17 e + sigma 28 e R_MAX + 2 e (1 + sigma R_MAX), with the terms of skipped stages left out.
It comes out below 1e-12 for every case of SHAPES (asserted in case()), i.e. far below the fp32 spacing except next to 0; for
augment's samples of 236 x 236 pixels the mean's term is larger with n and A reaches some 1e-11."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import grey_ref as ref
import guarded
from gpu_support import dev

pytestmark = pytest.mark.gpu

E = 2.0 ** -53
R_MAX = math.sqrt(66 * math.log(2))
S_MIN = 1e-6
SHAPES = ((3, 1961), (3, 3072), (3, 1), (3, 3), (3, 5), (65, 7))
ROWS = {            # gamma, contrast, brightness, sigma, invert: a different row per sample, cycled over the batch
    "affine": ((1.0, 1.2, -0.05, 0.0, 0.0), (1.0, 0.8, 0.08, 0.0, 1.0), (1.0, 1.0, 0.1, 0.0, 0.0)),
    "gamma": ((0.7, 1.0, 0.0, 0.0, 0.0), (1.5, 1.0, 0.0, 0.0, 1.0), (0.8, 1.0, 0.0, 0.0, 1.0)),
    "noise": ((1.0, 1.0, 0.0, 0.05, 0.0), (1.0, 1.0, 0.0, 0.02, 1.0), (1.0, 1.0, 0.0, 0.1, 0.0)),
    "all": ((0.75, 1.2, -0.05, 0.03, 0.0), (1.4, 0.8, 0.06, 0.05, 1.0), (0.8, 1.1, 0.02, 0.01, 1.0)),
}
SEED, STEP = 0x9E3779B97F4A7C15, (3 << 32) | 11


def images(seed, B, n):
    """float32 [B,n] in [0,1]: mostly dark background, a fifth of the pixels bright, each sample with 0 and 1 in it when
    it has the room (what the normalisation leaves)"""
    rs = np.random.RandomState(seed)
    x = (0.15 * rs.rand(B, n) + 0.8 * (rs.rand(B, n) < 0.2) * rs.rand(B, n)).astype(np.float32)
    if n >= 16:
        x[:, 3], x[:, n - 2] = 0.0, 1.0
    return x


def rows_for(kind, B):
    return np.array([ROWS[kind][b % 3] for b in range(B)], np.float64)


def abs_term(xn, params):
    """A of the module docstring per sample, [B]; xn = the (normalised) float64 input [B,n].  Asserts what L rests on."""
    B, n = xn.shape
    A = np.zeros(B)
    for b in range(B):
        g, c, br, sigma, inv = params[b]
        affine, gamma, noise = (c != 1.0 or br != 0.0), g != 1.0, sigma != 0.0
        e_in = 0.0
        if affine:
            m = float(np.mean(xn[b]))
            V = c * (float(np.abs(xn[b]).max()) + abs(m)) + abs(m) + abs(br)
            e_in = (n + 2) * E * float(np.mean(np.abs(xn[b]))) * abs(1 - c) + 4 * E * V
        if gamma:
            if affine:
                raw = (xn[b] - m) * c + m + br
                s = 1.0 - raw if inv else raw                    # the base of the power before the clamp
                assert ((s <= -1e-9) | (s >= S_MIN)).all(), "a pixel sits next to the base 0 of the power: another seed"
            e_in = max(g, g * S_MIN ** (g - 1)) * e_in + 17 * E
        A[b] = e_in + (sigma * 28 * E * R_MAX + 2 * E * (1 + sigma * R_MAX) if noise else 0.0)
    return A


@functools.lru_cache(maxsize=None)
def case(B, n, kind, clip=True):
    x = images(100 + n, B, n)
    params = rows_for(kind, B)
    want = ref.vary(x, params, SEED, STEP, 0, clip)
    A = abs_term(x.astype(np.float64), params)
    assert A.max() < 1e-12
    return x, params, want, A


def check(got, want, A, what):
    """got float32 [B,n], want float64 [B,n]: NaN where the reference is NaN, else within one fp32 spacing of it + A[b]"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    w = np.where(nan, 0.0, want)
    err = np.abs(np.where(nan, 0.0, got.astype(np.float64)) - w)
    bound = np.spacing(np.abs(w).astype(np.float32)).astype(np.float64) + A[:, None]
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print("%s: largest |device - fp64| = %.3g (%.3g of its bound), A <= %.3g" % (what, err.max(), (err / bound).max(), A.max()))
    assert (err <= bound).all(), "%s: sample %d pixel %d: device %r, reference %r, bound %.3g" % (
        what, worst[0], worst[1], got[worst], want[worst], bound[worst])


def raw_vary(dev, x, params, seed=SEED, step=STEP, first=0, clip=True, minmax=None, inplace=False, chunks=None, stream=None):
    """unet_grey_vary on guarded buffers; `chunks` = the samples per call (default: 64 at a time), each call with its own
    exact scratch and its first_sample.  Returns the float32 result [B,n]."""
    import _hip
    L = _hip.lib()
    arena = guarded.Arena(dev)
    B, n = x.shape
    xd = arena.inp(torch.from_numpy(x), "x")
    out = xd if inplace else arena.out((B, n), torch.float32, "out")
    mm = None if minmax is None else arena.inp(torch.from_numpy(np.ascontiguousarray(minmax, np.float32)), "minmax")
    chunks = chunks or [min(64, B - lo) for lo in range(0, B, 64)]
    assert sum(chunks) == B
    st = stream or torch.cuda.current_stream(dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
    at = lambda t, off: C.c_void_p(arena.address(t) + off)
    lo = 0
    with torch.cuda.device(dev):
        for b in chunks:
            sc = arena.scratch(L.unet_grey_scratch_bytes(b, n), "scratch")
            arr = (C.c_double * (5 * b))(*np.asarray(params[lo:lo + b], np.float64).ravel().tolist())
            rc = L.unet_grey_vary(at(xd, lo * n * 4), at(out, lo * n * 4), b, n, first + lo, arr, None if mm is None else at(mm, lo * 8),
                                  seed, step, 0 if clip else 1, arena.ptr(sc), C.c_void_p(st.cuda_stream))
            _hip.check(rc, "unet_grey_vary")
            lo += b
    st.synchronize()
    arena.verify(out)
    return out.cpu().numpy()


# ---- against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(ROWS))
@pytest.mark.parametrize("B,n", SHAPES)
def test_stages_equal_the_restatement(dev, B, n, kind):
    x, params, want, A = case(B, n, kind)
    got = raw_vary(dev, x, params)
    check(got, want, A, "grey_vary %s B=%d n=%d" % (kind, B, n))
    assert got.min() >= 0 and got.max() <= 1


@pytest.mark.parametrize("first,n", ((0, 1961), (5, 11), (2, 1), ((1 << 31) - 1 - 9, 9)))
def test_normals_equal_the_restatement(dev, first, n):
    import _hip
    arena = guarded.Arena(dev)
    out = arena.out((n,), torch.float64, "z")
    _hip.run("unet_grey_normals", dev, SEED, STEP, 77, first, n, arena.ptr(out))
    torch.cuda.synchronize()
    arena.verify(out)
    want = ref.normals(SEED, STEP, 77, first, n)
    err = float(np.abs(out.cpu().numpy() - want).max())
    print("grey_normals first=%d n=%d: largest |device - fp64| = %.3g" % (first, n, err))
    assert err <= 1e-12


# ---- against the library itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n", SHAPES)
def test_identity_returns_the_input_bit_for_bit(dev, B, n):
    x = images(7, B, n)
    got = raw_vary(dev, x, np.tile(np.array(ref.IDENTITY), (B, 1)))
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))
    # invert without gamma is the identity too
    got = raw_vary(dev, x, np.tile(np.array((1.0, 1.0, 0.0, 0.0, 1.0)), (B, 1)))
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


def test_no_clip_leaves_values_outside(dev):
    B, n = 3, 1961
    x = images(100 + n, B, n)
    params = np.array([(0.75, 1.2, -0.05, 0.3, 0.0), (1.0, 1.0, 0.0, 0.5, 0.0), ref.IDENTITY])
    got = raw_vary(dev, x, params, clip=False)
    want = ref.vary(x, params, SEED, STEP, 0, False)
    check(got, want, abs_term(x.astype(np.float64), params), "grey_vary without the clip")
    assert got[:2].min() < -0.1 and got[:2].max() > 1.1
    # the flag changes nothing but the clip; an image outside [0,1] passes through identity parameters unclipped, and clipped
    clipped = raw_vary(dev, x, params)
    assert np.array_equal(clipped, np.clip(got, 0, 1))
    wide = (3 * x - 1).astype(np.float32)
    ident = np.tile(np.array(ref.IDENTITY), (B, 1))
    assert np.array_equal(raw_vary(dev, wide, ident, clip=False).view(np.uint32), wide.view(np.uint32))
    assert np.array_equal(raw_vary(dev, wide, ident), np.clip(wide, 0, 1))


@pytest.mark.parametrize("B,n", ((3, 1961), (3, 3072), (3, 5)))
def test_in_place_equals_out_of_place(dev, B, n):
    x, params, _, _ = case(B, n, "all")
    assert np.array_equal(raw_vary(dev, x, params, inplace=True).view(np.uint32), raw_vary(dev, x, params).view(np.uint32))


@pytest.mark.parametrize("n", (1961, 3072, 5))
def test_fused_normalisation(dev, n):
    """With the min / max table the op equals unet_normalise01 followed by itself, bit for bit, in place and out of place, and
    the restatement within the bound; a constant sample is 0/0 = NaN throughout, whatever its parameters."""
    import _hip
    B = 4
    raw = np.floor(images(100 + n, B, n) * 255).astype(np.float32)
    raw[3] = 42.0                                                   # the constant sample
    mm = np.stack([raw.min(1), raw.max(1)], 1)
    params = np.concatenate([rows_for("all", 3), rows_for("all", 1)])
    fused = raw_vary(dev, raw, params, minmax=mm)
    assert np.array_equal(raw_vary(dev, raw, params, minmax=mm, inplace=True).view(np.uint32), fused.view(np.uint32))
    arena = guarded.Arena(dev)
    xd = arena.inp(torch.from_numpy(raw), "x")
    mmd = arena.inp(torch.from_numpy(mm), "minmax")
    _hip.run("unet_normalise01", dev, arena.ptr(xd), B, n, arena.ptr(mmd))
    torch.cuda.synchronize()
    arena.verify(xd)
    normed = xd.cpu().numpy()
    assert np.isnan(normed[3]).all() and normed[:3].min() == 0 and normed[:3].max() == 1
    two = raw_vary(dev, normed, params)
    assert np.array_equal(fused.view(np.uint32), two.view(np.uint32))
    want = ref.vary(raw, params, SEED, STEP, 0, True, mm)
    assert np.isnan(want[3]).all() and not np.isnan(want[:3]).any()
    xn = np.stack([ref.normalise01(raw[b], *mm[b]) for b in range(3)]).astype(np.float64)
    A = np.concatenate([abs_term(xn, params[:3]), [0.0]])
    check(fused, want, A, "grey_vary with minmax n=%d" % n)
    # identity parameters with the table: exactly unet_normalise01
    ident = raw_vary(dev, raw, np.tile(np.array(ref.IDENTITY), (B, 1)), minmax=mm)
    assert np.array_equal(ident.view(np.uint32), normed.view(np.uint32))


def test_two_streams_are_bit_equal(dev):
    x, params, _, _ = case(3, 1961, "all")
    a = raw_vary(dev, x, params, stream=torch.cuda.Stream(dev))
    b = raw_vary(dev, x, params, stream=torch.cuda.Stream(dev))
    c = raw_vary(dev, x, params)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), c.view(np.uint32))


@pytest.mark.parametrize("n", (1961, 7))
def test_chunked_calls_equal_one_call(dev, n):
    B = 6
    x = images(100 + n, B, n)
    params = rows_for("all", B)
    one = raw_vary(dev, x, params, first=5)
    for chunks in ([2, 4], [1, 1, 1, 1, 1, 1], [5, 1]):
        assert np.array_equal(raw_vary(dev, x, params, first=5, chunks=chunks).view(np.uint32), one.view(np.uint32)), chunks
    check(one, ref.vary(x, params, SEED, STEP, 5), abs_term(x.astype(np.float64), params), "grey_vary first_sample=5")


def test_noise_streams(dev):
    """Another step, seed or sample index is another noise; equal pixels of two samples get different noise; a sample with
    sigma = 0 inside a noisy batch equals its noiseless result."""
    B, n = 3, 1961
    x = np.repeat(images(3, 1, n), B, 0)                           # three copies of one image
    params = np.tile(np.array((1.0, 1.0, 0.0, 0.05, 0.0)), (B, 1))
    base = raw_vary(dev, x, params, clip=False)
    assert not np.array_equal(base[0], base[1]) and not np.array_equal(base[1], base[2])
    for kw in (dict(step=STEP + 1), dict(step=STEP + (1 << 32)), dict(seed=SEED + 1), dict(seed=SEED ^ (1 << 63)), dict(first=1)):
        other = raw_vary(dev, x, params, clip=False, **kw)
        assert (other != base).mean() > 0.99, kw
    assert np.array_equal(raw_vary(dev, x, params, clip=False, first=1)[:2], base[1:])      # the noise belongs to the global index
    params = rows_for("all", B)
    params[1, 3] = 0.0
    mixed = raw_vary(dev, x, params)
    quiet = params.copy()
    quiet[:, 3] = 0.0
    assert np.array_equal(mixed[1].view(np.uint32), raw_vary(dev, x, quiet)[1].view(np.uint32))
    assert not np.array_equal(mixed[0], raw_vary(dev, x, quiet)[0])


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def test_grey_variation_public(dev):
    """data.grey_variation on [H,W], [B,H,W] and [B,1,H,W], 65 samples in two chunks, out= and in place, minmax=; ValueErrors."""
    import data
    x, params, want, A = case(3, 1961, "all")
    t = torch.from_numpy(x).to(dev).reshape(3, 37, 53)
    raw = raw_vary(dev, x, params, seed=5, step=9)
    got = data.grey_variation(t, params, seed=5, step=9)
    assert got.shape == t.shape and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().reshape(3, -1), raw)
    assert np.array_equal(data.grey_variation(t[:, None], torch.from_numpy(params), seed=5, step=9).cpu().numpy().reshape(3, -1), raw)
    one = data.grey_variation(t[1], params[1], seed=5, step=9, first_sample=1)
    assert one.shape == (37, 53) and np.array_equal(one.cpu().numpy().ravel(), raw[1])
    out = torch.empty_like(t)
    assert data.grey_variation(t, params, seed=5, step=9, out=out) is out and np.array_equal(out.cpu().numpy().reshape(3, -1), raw)
    noclip = data.grey_variation(t, params, seed=5, step=9, clip=False)
    assert torch.equal(noclip.clamp(0, 1), got) and float(noclip.max()) > 1
    mm = torch.tensor([[0.0, 2.0]] * 3, device=dev)
    assert torch.equal(data.grey_variation(2 * t, params, seed=5, step=9, minmax=mm), got)
    same = t.clone()
    assert data.grey_variation(same, params, seed=5, step=9, out=same) is same and torch.equal(same, got)
    x65, p65, want65, A65 = case(65, 7, "all")
    got65 = data.grey_variation(torch.from_numpy(x65).to(dev).reshape(65, 1, 7), p65, seed=SEED, step=STEP)
    check(got65.cpu().numpy().reshape(65, 7), want65, A65, "grey_variation B=65")
    for bad in ((0.0, 1, 0, 0, 0), (-1.0, 1, 0, 0, 0), (1, -0.5, 0, 0, 0), (1, 1, 0, -0.1, 0), (1, 1, float("nan"), 0, 0),
                (1, 1, 0, float("inf"), 0), (1, 1, 0, 0, 0.5)):
        with pytest.raises(ValueError):
            data.grey_variation(t, np.array([ref.IDENTITY, bad, ref.IDENTITY]))
    for kw in (dict(params=params[:2]), dict(params=params, out=torch.empty(3, 37, 52, device=dev)), dict(params=params, minmax=mm[:2]),
               dict(params=params, minmax=mm.cpu()), dict(params=params, seed=-1), dict(params=params, first_sample=2 ** 32 - 2)):
        with pytest.raises(ValueError):
            data.grey_variation(t, **kw)
    for images_ in (t.double(), t.cpu(), t.reshape(3, 37, 53, 1, 1), t[:, None].expand(3, 2, 37, 53)):
        with pytest.raises(ValueError):
            data.grey_variation(images_, params)


def blobs(rs, B, H, W):
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((B, H, W), bool)
    for b in range(B):
        for _ in range(6):
            cy, cx, r = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(4, max(5, min(H, W) / 4))
            m[b] |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return m * np.float32(255)


def augment_inputs(dev):
    rs = np.random.RandomState(9)
    image = torch.from_numpy(np.floor(rs.rand(2, 96, 96) * 256).astype(np.float32)).to(dev)
    target = torch.from_numpy(blobs(rs, 2, 96, 96)).to(dev)
    return image, target, [(10, 30), (44, 3)], [30.0, 240.0]


@pytest.mark.parametrize("elastic", ("grid", "field"))
def test_augment_grey(dev, elastic):
    import data
    image, target, origins, angles = augment_inputs(dev)
    crop = 52
    params = rows_for("all", 2)
    run = lambda **kw: data.augment(image, target, origins, crop, angles, 3, 10, random_state=np.random.RandomState(7), elastic=elastic, **kw)
    plain = run()
    # identity parameters: today's result, bit for bit
    ident = run(grey=np.tile(np.array(data.GREY_IDENTITY), (2, 1)), grey_seed=3, grey_step=4)
    assert torch.equal(ident[0], plain[0]) and torch.equal(ident[1], plain[1])
    # the stage is its pieces: the normalised image of the plain call through grey_variation (the fused normalisation is
    # unet_normalise01's, bit for bit), which is the restatement within the bound
    inp, gt = run(grey=params, grey_seed=3, grey_step=4)
    assert inp.shape == plain[0].shape and inp.dtype == torch.float32 and torch.equal(gt, plain[1])
    assert torch.equal(inp, data.grey_variation(plain[0], params, seed=3, step=4))
    assert not torch.equal(inp, plain[0]) and float(inp.min()) >= 0 and float(inp.max()) <= 1
    x = plain[0].cpu().numpy().reshape(2, -1)
    check(inp.cpu().numpy().reshape(2, -1), ref.vary(x, params, 3, 4), abs_term(x.astype(np.float64), params), "augment(%s, grey)" % elastic)
    assert not torch.equal(run(grey=params, grey_seed=3, grey_step=5)[0], inp) and not torch.equal(run(grey=params, grey_seed=4, grey_step=4)[0], inp)
    assert torch.equal(run(grey=params, grey_seed=3, grey_step=4)[0], inp)
    # without noise a batched call is the per-sample calls (the noise of a sample belongs to its position in the batch)
    quiet = params.copy()
    quiet[:, 3] = 0.0
    batched = run(grey=quiet)
    rs = np.random.RandomState(7)
    for b in range(2):
        one = data.augment(image[b], target[b], origins[b], crop, angles[b], 3, 10, random_state=rs, elastic=elastic, grey=quiet[b])
        assert torch.equal(one[0], batched[0][b]) and torch.equal(one[1], batched[1][b])
    # a dict of ranges: drawn from random_state after this call's elastic draws, in grey_parameters' order
    ranges = dict(gamma=(0.6, 1.6), noise=(0.0, 0.1), p_invert=0.5)
    drawn = run(grey=ranges, grey_seed=1, grey_step=2)
    rs = np.random.RandomState(7)
    if elastic == "grid":
        kw = dict(disp=data.grid_displacements(rs, 2, 3, 10))
    else:
        S = plain[0].shape[-1]
        f = [(rs.rand(S, S), rs.rand(S, S)) for _ in range(2)]
        kw = dict(fields=(np.stack([d[0] for d in f]), np.stack([d[1] for d in f])))
    p = data.grey_parameters(rs, 2, **ranges)
    replay = data.augment(image, target, origins, crop, angles, 3, 10, elastic=elastic, grey=p, grey_seed=1, grey_step=2, **kw)
    assert torch.equal(drawn[0], replay[0]) and torch.equal(drawn[1], replay[1])
    with pytest.raises(ValueError):
        data.augment(image, target, origins, crop, angles, 3, 10, elastic=elastic, grey={}, **kw)
    with pytest.raises(ValueError):
        run(grey=params[:1])
    with pytest.raises(ValueError):
        run(grey={"gama": (1, 2)})


def test_crop_dataset_grey_trains_a_step(dev, tmp_path):
    """CropDataset(grey={...}) is stable per seed, grey_step advances by one per batch and can be set, the batch is
    data.augment(grey=...) with a host replay of the draws, and trainer.training's step accepts it: one step on a base-32 net
    at the smallest legal tile (crop 196, S = 380) gives a finite loss."""
    import data
    import network
    import prepare_ref
    import trainer
    N, H, W, crop = 2, 230, 250, 196
    rs = np.random.RandomState(77)
    imgs = (rs.rand(N, H, W) * 255).astype(np.uint8)
    inst = prepare_ref.ids_batch("discs", 21, N, H, W).astype(np.uint16)
    ranges = dict(noise=(0.01, 0.05), p_invert=0.5)
    make = lambda bs=1, **kw: data.CropDataset(imgs, inst, 3, 10, crop, bs, np.random.RandomState(5), random_state=np.random.RandomState(6),
                                               elastic="grid", grid=3, grey=ranges, grey_seed=12, **kw)
    ds = make()
    assert len(ds) == 2 and ds.grey_step == 0
    first = list(ds)
    assert ds.grey_step == 2
    assert first[0][0].shape == (1, 1, 380, 380) and first[0][0].dtype == torch.float32 and first[0][1].shape == (1, 1, crop, crop)
    again = list(make())
    for (a, b), (c, d) in zip(first, again):
        assert torch.equal(a, c) and torch.equal(b, d)
    # replay: rng gives origins and angles as without grey; random_state gives, batch after batch, the nodes, then the parameters
    replay, rstate = np.random.RandomState(5), np.random.RandomState(6)
    for i in range(N):
        xy = data.draw_crop(replay, ds.pairs, ds.target_weighted_crop_distribution[i], (H, W), crop)
        ang = replay.choice(np.arange(0, 360, 30))
        d = data.grid_displacements(rstate, 1, 3, 10)
        p = data.grey_parameters(rstate, 1, **ranges)
        want = data.augment(ds.image[[i]], ds.target[[i]], [xy], crop, [ang], 3, 10, elastic="grid", disp=d, grey=p, grey_seed=12, grey_step=i)
        assert torch.equal(first[i][0], want[0]) and torch.equal(first[i][1], want[1])
        assert 0 <= float(first[i][0].min()) and float(first[i][0].max()) <= 1
    # rng's sequence is what it is without grey: the same origins and angles, so the same targets
    plain = list(data.CropDataset(imgs, inst, 3, 10, crop, 1, np.random.RandomState(5), random_state=np.random.RandomState(6), elastic="grid"))
    assert ds.grey_step == 2 and torch.equal(plain[0][1], first[0][1]) and not torch.equal(plain[0][0], first[0][0])
    # a resumed run sets the step: the second batch of a fresh dataset whose first batch was consumed elsewhere
    ds2 = make()
    next(iter(ds2))
    assert ds2.grey_step == 1
    ds2.grey_step = 40
    later = list(ds2)
    assert ds2.grey_step == 42 and not torch.equal(later[0][0], first[0][0])
    with pytest.raises(ValueError):
        data.CropDataset(imgs, inst, 3, 10, crop, 1, np.random.RandomState(5), elastic="field", grey=ranges)
    ds = make(bs=2)
    net = network.Unet(base_ch=32).to(dev)
    trainer.training(net, ds, ds, 0, 2, dev, str(tmp_path), "grey-test")
    loss = np.loadtxt(os.path.join(str(tmp_path), "progress", "loss.out"))
    loss_val = np.loadtxt(os.path.join(str(tmp_path), "progress", "loss_val.out"))
    assert loss.size == 1 and np.isfinite(loss).all() and np.isfinite(loss_val).all()
    assert ds.grey_step == 2                                # one training batch, one validation batch
