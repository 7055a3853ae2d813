"""The restatement of the grey-value variation (tests/grey_ref.py), which tests/test_grey_gpu.py holds the device op to, pinned
on the CPU: its normals (built on tests/philox_ref.py, which test_dropout_cpu.py pins to the published known answers) by their
moments and a Kolmogorov-Smirnov test, its stages against formulas written out independently here.  data.grey_parameters
against the explicit sequence of RandomState calls.  And the new entry points: declared, in the ctypes table, in the library,
and refusing bad arguments on the host, before any device is touched."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy import stats

import grey_ref as ref
import philox_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_grey_scratch_bytes", "unet_grey_vary", "unet_grey_normals")
BADARG = -2                      # UNET_E_BADARG: what ARG_CHECK returns


# ---- the normals ------------------------------------------------------------------------------------------------------------
def test_normals_are_standard_normal():
    """2^16 draws of one (seed, step, sample): mean, variance and kurtosis within 4 standard errors of 0, 1 and 3 (standard
    errors of N independent normals: sqrt(1/N), sqrt(2/N), sqrt(24/N)), and the Kolmogorov-Smirnov test against the normal
    distribution does not reject at 1e-3 (checked for this seed: p is printed)."""
    N = 1 << 16
    z = ref.normals(2015, 3, 1, 0, N)
    assert z.shape == (N,) and z.dtype == np.float64 and np.isfinite(z).all()
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2
    p = stats.kstest(z, "norm").pvalue
    print("normals: mean %.4g var %.5g kurtosis %.5g, KS p = %.3g" % (mean, var, kurt, p))
    assert abs(mean) <= 4 * math.sqrt(1.0 / N)
    assert abs(var - 1) <= 4 * math.sqrt(2.0 / N)
    assert abs(kurt - 3) <= 4 * math.sqrt(24.0 / N)
    assert p > 1e-3
    # cos and sin halves of a pair are uncorrelated, and so are neighbouring pairs
    q = z.reshape(-1, 4)
    for a, b in ((0, 1), (2, 3), (0, 2), (1, 3)):
        assert abs(np.mean(q[:, a] * q[:, b])) <= 4 * math.sqrt(4.0 / N)


def test_normals_layout_and_streams():
    """Written out for single pixels from philox_ref's words: pixel i takes the pair (0,1) or (2,3) of counter
    (i >> 2, sample, step lo, step hi) under key (seed lo, seed hi ^ 0x47524559), cos for the even pixel, sin for the odd one.
    A window [first, first + n) is that part of the whole; another seed, step or sample is another stream; and the key differs
    from drop-out's key of the same seed."""
    seed, step, sample = 0x1234567890ABCDEF, (7 << 32) | 9, 5
    z = ref.normals(seed, step, sample, 0, 23)
    for i in (0, 1, 2, 3, 4, 9, 18, 22):
        w = philox_ref.philox4x32_10((np.uint32(i >> 2), np.uint32(sample), np.uint32(9), np.uint32(7)),
                                     (seed & 0xFFFFFFFF, (seed >> 32) ^ 0x47524559))
        pair = 0 if (i & 3) < 2 else 2
        u1, u2 = (int(w[pair]) + 0.5) / 2.0 ** 32, (int(w[pair + 1]) + 0.5) / 2.0 ** 32
        r = math.sqrt(-2.0 * math.log(u1))
        want = r * (math.cos(2 * math.pi * u2) if i % 2 == 0 else math.sin(2 * math.pi * u2))
        assert abs(z[i] - want) <= 1e-14, i
    assert np.array_equal(ref.normals(seed, step, sample, 5, 11), z[5:16])
    for other in ((seed + 1, step, sample), (seed, step + 1, sample), (seed, step, sample + 1), (seed ^ (1 << 40), step, sample)):
        assert np.abs(ref.normals(*other, 0, 23) - z).min() > 0
    # the extreme words stay finite: u1 = 2^-33 is the smallest argument of log
    assert math.isfinite(math.sqrt(-2.0 * math.log(0.5 / 2.0 ** 32)))


# ---- the stages -------------------------------------------------------------------------------------------------------------
def sample_image(seed, n):
    rs = np.random.RandomState(seed)
    return (0.15 * rs.rand(n) + 0.7 * (rs.rand(n) < 0.2) * rs.rand(n)).astype(np.float32)        # mostly background, in [0, 0.85)


@pytest.mark.parametrize("invert", (0.0, 1.0))
def test_stages_against_formulas(invert):
    x = sample_image(1, 1961)
    gamma, contrast, brightness, sigma = 0.8, 1.2, -0.05, 0.03
    r = ref.stages(x, (gamma, contrast, brightness, sigma, invert), seed=11, step=2, sample=3)
    xd = [float(v) for v in x]
    m = math.fsum(xd) / len(xd)
    assert abs(r["mean"] - m) <= len(xd) * 2.0 ** -53 * m
    z = ref.normals(11, 2, 3, 0, x.size)
    for i in range(0, x.size, 97):
        u = min(max((xd[i] - m) * contrast + m + brightness, 0.0), 1.0)
        assert abs(r["affine"][i] - u) <= 1e-15
        u = 1.0 - float(np.power(1.0 - u, gamma)) if invert else float(np.power(u, gamma))
        assert abs(r["gamma"][i] - u) <= 1e-14
        u = u + sigma * z[i]
        assert abs(r["noise"][i] - u) <= 1e-14
        assert abs(r["out"][i] - min(max(u, 0.0), 1.0)) <= 1e-14
    assert r["out"].min() >= 0 and r["out"].max() <= 1
    assert (r["affine"] == 0).any()                       # the clamp after the affine stage does work on this image
    unclipped = ref.stages(x, (gamma, contrast, brightness, 0.2, invert), seed=11, step=2, sample=3, clip=False)["out"]
    assert unclipped.min() < 0 and unclipped.max() > 1


def test_identity_stages_are_skipped():
    x = sample_image(2, 500)
    r = ref.stages(x, ref.IDENTITY)
    assert r["mean"] is None and np.array_equal(r["out"], x.astype(np.float64))
    assert np.array_equal(r["out"].astype(np.float32).view(np.uint32), x.view(np.uint32))
    # invert with gamma == 1 is the identity too, and each stage alone leaves the others' values alone
    assert np.array_equal(ref.stages(x, (1.0, 1.0, 0.0, 0.0, 1.0))["out"], x.astype(np.float64))
    only_gamma = ref.stages(x, (0.7, 1.0, 0.0, 0.0, 0.0))
    assert only_gamma["mean"] is None and np.array_equal(only_gamma["affine"], only_gamma["x"])
    assert np.array_equal(only_gamma["out"], np.power(x.astype(np.float64), 0.7))
    only_noise = ref.stages(x, (1.0, 1.0, 0.0, 0.1, 0.0), seed=1, clip=False)
    assert np.array_equal(only_noise["out"], x.astype(np.float64) + 0.1 * ref.normals(1, 0, 0, 0, 500))
    # contrast 0 collapses the sample onto its mean + brightness
    flat = ref.stages(x, (1.0, 0.0, 0.1, 0.0, 0.0))
    assert np.abs(flat["out"] - (flat["mean"] + 0.1)).max() <= 1e-15


def test_normalisation_and_nan():
    x = (sample_image(3, 300) * 255).astype(np.float32)
    lo, hi = x.min(), x.max()
    r = ref.stages(x, (0.9, 1.1, 0.0, 0.0, 0.0), minmax=(lo, hi))
    want = ((x - lo) / (hi - lo)).astype(np.float32)
    assert np.array_equal(r["x"], want.astype(np.float64)) and r["x"].min() == 0 and r["x"].max() == 1
    const = np.full(7, 3.0, np.float32)                   # 0/0: NaN, which every stage keeps
    assert np.isnan(ref.stages(const, ref.IDENTITY, minmax=(3.0, 3.0))["out"]).all()
    assert np.isnan(ref.stages(const, (0.8, 1.2, 0.1, 0.1, 0.0), minmax=(3.0, 3.0))["out"]).all()
    one_nan = sample_image(4, 50)
    one_nan[7] = np.nan                                   # a NaN pixel: alone without the affine stage, the whole sample with it
    assert np.isnan(ref.stages(one_nan, (0.8, 1.0, 0.0, 0.0, 0.0))["out"]).sum() == 1
    assert np.isnan(ref.stages(one_nan, (0.8, 1.2, 0.0, 0.0, 0.0))["out"]).all()


# ---- grey_parameters --------------------------------------------------------------------------------------------------------
def test_grey_parameters_draw_order():
    import data
    kw = dict(gamma=(0.6, 1.8), contrast=(0.5, 1.5), brightness=(-0.2, 0.3), noise=(0.01, 0.08), p_invert=0.4)
    B = 40
    p = data.grey_parameters(np.random.RandomState(3), B, **kw)
    assert p.shape == (B, 5) and p.dtype == np.float64
    rs = np.random.RandomState(3)
    for b in range(B):
        want = [np.exp(rs.uniform(np.log(0.6), np.log(1.8))), rs.uniform(0.5, 1.5), rs.uniform(-0.2, 0.3), rs.uniform(0.01, 0.08),
                1.0 if rs.uniform(0.0, 1.0) < 0.4 else 0.0]
        assert np.array_equal(p[b], want), b
    assert (p[:, 0] >= 0.6).all() and (p[:, 0] <= 1.8).all() and (p[:, 1] >= 0.5).all() and (p[:, 1] <= 1.5).all()
    assert (p[:, 2] >= -0.2).all() and (p[:, 2] <= 0.3).all() and (p[:, 3] >= 0.01).all() and (p[:, 3] <= 0.08).all()
    assert set(p[:, 4]) == {0.0, 1.0}
    d = data.grey_parameters(np.random.RandomState(3), B)                  # the defaults
    assert (d[:, 0] >= 0.7).all() and (d[:, 0] <= 1.5).all() and (d[:, 4] == 0).all()
    assert (np.log(d[:, 0]) < 0).any() and (np.log(d[:, 0]) > 0).any()
    # five draws per sample whatever the ranges: degenerate ranges consume theirs, and give the value
    states = []
    for ranges in (kw, {}, dict(gamma=(1.0, 1.0), contrast=(1.0, 1.0), brightness=(0.0, 0.0), noise=(0.0, 0.0), p_invert=0.0),
                   dict(noise=(0.02, 0.02), p_invert=1.0)):
        rs = np.random.RandomState(8)
        q = data.grey_parameters(rs, 7, **ranges)
        states.append(rs.uniform())
        if ranges.get("gamma") == (1.0, 1.0):
            assert np.array_equal(q, np.tile(np.array(data.GREY_IDENTITY), (7, 1)))
        if ranges.get("p_invert") == 1.0:
            assert (q[:, 3] == 0.02).all() and (q[:, 4] == 1).all()
    rs = np.random.RandomState(8)
    rs.uniform(size=35)
    assert states == [rs.uniform()] * 4
    assert data.grey_parameters(np.random.RandomState(1), 0).shape == (0, 5)


def test_python_value_errors():
    import data
    rs = np.random.RandomState(0)
    with pytest.raises(ValueError):
        data.grey_parameters(None, 2)
    for bad in (dict(gamma=(0.0, 1.0)), dict(gamma=(1.5, 0.7)), dict(contrast=(-0.1, 1.0)), dict(noise=(-0.01, 0.05)),
                dict(brightness=(0.0, float("inf"))), dict(p_invert=1.5), dict(noise=(0.0,))):
        with pytest.raises(ValueError):
            data.grey_parameters(rs, 2, **bad)
    host = torch.zeros(2, 8, 8)
    with pytest.raises(ValueError, match="device"):
        data.grey_variation(host, np.tile(np.array(data.GREY_IDENTITY), (2, 1)))
    with pytest.raises(ValueError):
        data.grey_variation(host.numpy(), np.tile(np.array(data.GREY_IDENTITY), (2, 1)))
    # a dict of ranges needs the host generator, in augment and in CropDataset; both refuse before any device work
    with pytest.raises(ValueError, match="random_state"):
        data.augment(host, host, [(0, 0)] * 2, 4, [0, 0], 3, 10, grey={})
    with pytest.raises(ValueError, match="random_state"):
        data.CropDataset(np.zeros((1, 8, 8)), np.zeros((1, 8, 8)), 3, 10, 4, 1, np.random.RandomState(0), grey={})
    with pytest.raises(ValueError, match="dict"):
        data.CropDataset(np.zeros((1, 8, 8)), np.zeros((1, 8, 8)), 3, 10, 4, 1, np.random.RandomState(0), random_state=rs, grey=np.zeros((1, 5)))
    with pytest.raises(ValueError, match="blur"):
        data.CropDataset(np.zeros((1, 8, 8)), np.zeros((1, 8, 8)), 3, 10, 4, 1, np.random.RandomState(0), random_state=rs, grey={"blur": 1})


# ---- the library --------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_new_entry_points():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(L, name), name
    assert L.unet_abi_version() == 4
    assert "#define UNET_GREY_MAX_SAMPLES 64" in hdr and "#define UNET_GREY_NO_CLIP 1" in hdr
    import data
    assert data.MAX_GREY_SAMPLES == 64 and data.GREY_NO_CLIP == 1
    # one fp64 partial per workgroup of the sum pass, 64 per sample at the most; 0 for a shape the op refuses
    assert 3 * 8 <= L.unet_grey_scratch_bytes(3, 5) <= 3 * 64 * 8 + 256
    assert 64 * 64 * 8 <= L.unet_grey_scratch_bytes(64, 700 * 700) <= 64 * 64 * 8 + 256
    assert L.unet_grey_scratch_bytes(0, 5) == 0 and L.unet_grey_scratch_bytes(65, 5) == 0 and L.unet_grey_scratch_bytes(1, 0) == 0


def test_library_refuses_bad_arguments_before_any_launch():
    """ARG_CHECK answers on the host, so no device is needed to be refused: each call below breaks one rule, returns
    UNET_E_BADARG and leaves a message.  (The pointers are never dereferenced.)"""
    import _hip
    _hip.build()
    L = _hip.lib()
    q = C.c_void_p(4096)

    def call(x=q, out=q, B=2, n=16, first=0, params=(1.2, 0.9, 0.1, 0.02, 0.0) * 2, minmax=None, flags=0, scratch=q, null_params=False):
        arr = None if null_params else (C.c_double * len(params))(*params)
        return L.unet_grey_vary(x, out, B, n, first, arr, minmax, 1, 2, flags, scratch, None)

    ok = (1.2, 0.9, 0.1, 0.02, 0.0)
    bad = [
        (dict(x=None), b"null"), (dict(out=None), b"null"), (dict(null_params=True), b"null"), (dict(scratch=None), b"scratch"),
        (dict(B=0), b"B = 0"), (dict(B=65, params=ok * 65), b"B = 65"), (dict(n=0), b"n = 0"), (dict(n=1 << 31), b"n = "),
        (dict(first=-1), b"first_sample"), (dict(first=(1 << 32) - 1), b"first_sample"),
        (dict(params=ok + (0.0, 1.0, 0.0, 0.0, 0.0)), b"gamma"), (dict(params=ok + (-0.5, 1.0, 0.0, 0.0, 0.0)), b"gamma"),
        (dict(params=ok + (1.0, -0.1, 0.0, 0.0, 0.0)), b"contrast"), (dict(params=ok + (1.0, 1.0, 0.0, -0.01, 0.0)), b"sigma"),
        (dict(params=ok + (1.0, 1.0, 0.0, 0.0, 0.5)), b"invert"),
        (dict(flags=2), b"flag"), (dict(flags=-1), b"flag"),
        (dict(x=C.c_void_p(4098)), b"misaligned"), (dict(minmax=C.c_void_p(4097)), b"misaligned"),
    ]
    for k in range(5):
        for v in (float("nan"), float("inf"), -float("inf")):
            row = list(ok)
            row[k] = v
            bad.append((dict(params=ok + tuple(row)), b"not finite"))
    for kw, word in bad:
        rc = call(**kw)
        assert rc == BADARG and word in L.unet_last_error(), (kw, rc, L.unet_last_error())
    # the normals
    assert L.unet_grey_normals(1, 2, 0, 0, 8, None, None) == BADARG and b"null" in L.unet_last_error()
    assert L.unet_grey_normals(1, 2, -1, 0, 8, q, None) == BADARG and b"sample" in L.unet_last_error()
    assert L.unet_grey_normals(1, 2, 1 << 32, 0, 8, q, None) == BADARG and b"sample" in L.unet_last_error()
    assert L.unet_grey_normals(1, 2, 0, (1 << 31) - 4, 8, q, None) == BADARG and b"2^31" in L.unet_last_error()
    assert L.unet_grey_normals(1, 2, 0, 0, 8, C.c_void_p(4100), None) == BADARG and b"misaligned" in L.unet_last_error()
    assert L.unet_grey_normals(1, 2, 0, 0, 0, None, None) == 0          # nothing to do is no error
