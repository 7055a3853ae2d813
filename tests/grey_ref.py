"""fp64 numpy restatement of the grey-value variation (include/unet_hip.h, unet_grey_vary), which
tests/test_grey_gpu.py holds the device op to.  The normals stand on tests/philox_ref.py, which test_dropout_cpu.py pins to the
published known answers; tests/test_grey_cpu.py pins the rest to formulas written out independently.

A sample is n float32 pixels; its parameters are (gamma, contrast, brightness, sigma, invert).  Stages, in this order, all in
float64 after the float32 normalisation: normalise (only with a min / max pair), mean, affine about the mean + clamp, gamma,
noise, clip.  A stage with identity parameters is skipped."""
import numpy as np

import philox_ref

KEY_XOR = 0x47524559                # XOR-ed into the high word of the seed: another stream than drop-out's of that seed
IDENTITY = (1.0, 1.0, 0.0, 0.0, 0.0)
_TWO_PI = 2.0 * np.pi


def normals(seed, step, sample, first, n):
    """float64 [n]: z of pixels first .. first+n-1 of global sample `sample`.  Counter (i >> 2, sample, step lo, step hi), key
    (seed lo, seed hi ^ KEY_XOR); words 0, 1 of group g = i >> 2 give pixels 4g (cos) and 4g+1 (sin), words 2, 3 give 4g+2 and
    4g+3; u = (w + 0.5) 2^-32, z = sqrt(-2 log u1) cos / sin (2 pi u2)."""
    idx = np.uint64(first) + np.arange(n, dtype=np.uint64)
    g = idx >> np.uint64(2)
    j = (idx & np.uint64(3)).astype(np.int64)
    gu, inv = np.unique(g, return_inverse=True)
    words = philox_ref.philox4x32_10((gu.astype(np.uint32), np.uint32(sample), np.uint32(step & 0xFFFFFFFF), np.uint32(step >> 32)),
                                     (seed & 0xFFFFFFFF, (seed >> 32) ^ KEY_XOR))
    w = np.stack(words, axis=1).astype(np.float64)                                   # [groups, 4]
    u = (w + 0.5) * 2.0 ** -32
    z = np.empty_like(u)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[:, a]))
        t = _TWO_PI * u[:, a + 1]
        z[:, a] = r * np.cos(t)
        z[:, a + 1] = r * np.sin(t)
    return z[inv.ravel(), j]


def normalise01(x, lo, hi):
    """unet_normalise01's float32 arithmetic: (x - lo) / (hi - lo), true division; 0/0 is NaN"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x - np.float32(lo)) / (np.float32(hi) - np.float32(lo))


def clamp01(u):
    return np.minimum(np.maximum(u, 0.0), 1.0)          # numpy's minimum / maximum keep a NaN


def stages(x, params, seed=0, step=0, sample=0, clip=True, minmax=None):
    """One sample: x float32 of any shape -> the float64 value of every stage, as a dict (x, mean, affine_raw = the affine
    stage before its clamp, affine, gamma, noise, out); a skipped stage repeats its input, mean is None when the affine stage
    is skipped."""
    gamma, contrast, brightness, sigma, invert = (float(v) for v in params)
    shape = np.shape(x)
    x32 = np.asarray(x, np.float32).ravel()
    if minmax is not None:
        x32 = normalise01(x32, minmax[0], minmax[1])
    u = x32.astype(np.float64)
    r = {"x": u.reshape(shape), "mean": None}
    with np.errstate(invalid="ignore"):
        if contrast != 1.0 or brightness != 0.0:
            m = float(np.sum(u)) / u.size
            r["mean"] = m
            u = (u - m) * contrast + m + brightness
        r["affine_raw"] = u.reshape(shape)
        if r["mean"] is not None:
            u = clamp01(u)
        r["affine"] = u.reshape(shape)
        if gamma != 1.0:
            u = 1.0 - np.power(1.0 - u, gamma) if invert else np.power(u, gamma)
        r["gamma"] = u.reshape(shape)
        if sigma != 0.0:
            u = u + sigma * normals(seed, step, sample, 0, u.size)
        r["noise"] = u.reshape(shape)
        if clip:
            u = clamp01(u)
    r["out"] = u.reshape(shape)
    return r


def vary(x, params, seed=0, step=0, first_sample=0, clip=True, minmax=None):
    """A batch: x float32 [B, ...], params [B,5], minmax [B,2] or None -> float64 of x's shape (not narrowed to float32)"""
    x = np.asarray(x, np.float32)
    return np.stack([stages(x[b], params[b], seed, step, first_sample + b, clip, None if minmax is None else minmax[b])["out"]
                     for b in range(x.shape[0])])
