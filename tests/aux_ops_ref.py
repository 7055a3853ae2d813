"""fp64 numpy / scipy references and the fixed inputs of the per-op tests of aux.hip and unet_eval_masks (tests/test_aux_ops_gpu.py), pinned to
scipy and to oracle/aux_ref.py by tests/test_aux_ops_cpu.py.  Imported like the other *_ref.py files.

The inputs are part of the reference: they are built so that every comparison is well-posed before a GPU is involved
(coordinates that fp32 and fp64 agree on exactly, rounded outputs whose fp64 value is far from a rounding boundary), and the
CPU test asserts each of those conditions."""
import functools

import numpy as np
from scipy import ndimage

from oracle import aux_ref

U24 = 2.0 ** -24           # unit roundoff of fp32


# ---- mirror pad ---------------------------------------------------------------------------------------------------------
MIRROR_CASES = [(5, 5), (5, 13), (6, 8), (37, 61)]            # (n, S): P = 0, P = n - 1 (the maximum), n odd / even
MIRROR_BIG = (17, 496, 500)                                   # (B, n, S): B * S * S > 16384 * 256, the grid-stride loop


def index_image(B, n):
    """1000 * row + col, shifted per image: every pixel of a batch names itself (exact in fp32 up to n = 1000)."""
    r = np.arange(n, dtype=np.float32)
    return np.stack([1000.0 * r[:, None] + r[None, :] + np.float32(0.25 * b) for b in range(B)]).astype(np.float32)


def mirror_pad(x, S, minmax=None):
    """x fp32 [B,n,n] -> [B,S,S]: aux_ref.mirror_index on both axes; with minmax [B,2]: (v - lo) / (hi - lo) in fp32."""
    idx = aux_ref.mirror_index(S, x.shape[-1])
    out = x[:, idx][:, :, idx]
    if minmax is not None:
        lo = minmax[:, 0].astype(np.float32)[:, None, None]; hi = minmax[:, 1].astype(np.float32)[:, None, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            out = (out - lo) / (hi - lo)
    return out.astype(np.float32)


# ---- separable Gaussian ---------------------------------------------------------------------------------------------------
GAUSS_CASES = [(9, 31, 3.0), (31, 9, 3.0), (5, 5, 0.1), (12, 40, 10.0)]     # r = 12 > H, r = 12 > W, r = 0, r = 40 = W
GAUSS_BIG = (1181, 1187, 3.0)                                               # 3 * H * W > 16384 * 256


def gaussian_taps32(sigma):
    """The fp32 taps data.elastic_transform uploads (data.gaussian_taps) and the radius."""
    w, r = aux_ref.gaussian_taps(sigma)
    return w.astype(np.float32), r


def gaussian_field(seed, B, H, W):
    """B different fields in [-1, 1), fp32 (what elastic_transform feeds the filter: 2 u - 1)."""
    return (np.random.RandomState(seed).rand(B, H, W) * 2 - 1).astype(np.float32)


def _correlate_zero(x, w, r, axis):
    """sum_k w[k + r] x[i + k] along axis, x zero outside the image, in fp64."""
    n = x.shape[axis]
    out = np.zeros_like(x)
    for k in range(-r, r + 1):
        lo, hi = max(0, -k), min(n, n - k)                    # output positions i with 0 <= i + k < n
        if lo >= hi:
            continue
        dst = [slice(None)] * x.ndim; src = [slice(None)] * x.ndim
        dst[axis] = slice(lo, hi); src[axis] = slice(lo + k, hi + k)
        out[tuple(dst)] += w[k + r] * x[tuple(src)]
    return out


def gaussian_filter(field, taps32, radius, scale):
    """field [B,H,W]: the two zero-extended correlations (rows, then columns) in fp64 with the fp32 taps cast to fp64, x scale."""
    w = taps32.astype(np.float64)
    t = _correlate_zero(field.astype(np.float64), w, radius, 1)
    return _correlate_zero(t, w, radius, 2) * float(scale)


def gaussian_bound(field, taps32, radius, scale):
    """Bound on |kernel - gaussian_filter| (u = 2^-24, m = 2 r + 1 taps, A = max|field| * sum|w|):
    pass 1 is a chain of at most m fmaf, each rounds a partial sum of magnitude <= A once: error <= m u A (to first order);
    pass 2 carries that error through sum|w| (<= m u A sum|w|) and adds m roundings of partial sums <= A sum|w|;
    the final multiply by scale rounds once more.  With sum|w| = 1 + O(m u): (2 m + 1) u A scale = (4 r + 3) u A scale to first
    order; gamma_k = k u / (1 - k u) with k = 4 r + 4 covers the higher-order terms and the taps' own sum."""
    k = 4 * radius + 4
    A = float(np.abs(field).max()) * float(np.abs(taps32.astype(np.float64)).sum()) ** 2
    return k * U24 / (1 - k * U24) * A * abs(float(scale))


# ---- bilinear warp ---------------------------------------------------------------------------------------------------------
WARP_CASES = [(13, 22), (22, 13), (1, 9), (7, 1), (2, 2)]
WARP_B = 2


def warp_case(H, W):
    """(img, dy, dx), each fp32 [2,H,W].  Displacements are multiples of 1/8 in [-3, 3]: row + dy is exact in fp32, so fp32 and
    fp64 agree on the coordinate and on which pixels fall outside.  The image is asymmetric (a random part plus a ramp that
    differs along rows and columns) and the two fields are independent draws.  Planted in plane 0, where the shape has the pixel:
    coordinates exactly 0, exactly H - 1 / W - 1 (inside: y0 clamped, fy = 1), -1/8 and H - 1 + 1/8 / W - 1 + 1/8 (outside)."""
    rs = np.random.RandomState(1 if H <= W else 2)
    B = WARP_B
    yy, xx = np.mgrid[0:H, 0:W]
    img = (rs.rand(B, H, W) * 200 + 3.0 * yy + 1.0 * xx).astype(np.float32)
    dy = (rs.randint(-24, 25, (B, H, W)) / 8.0).astype(np.float32)
    dx = (rs.randint(-24, 25, (B, H, W)) / 8.0).astype(np.float32)
    if H <= 2:                            # an extent of 1 or 2: coordinates in [-1/4, H - 1 + 1/4], 60 % of them moved inside
        c = rs.randint(-2, 8 * (H - 1) + 3, (B, H, W)) / 8.0
        dy = (np.where(rs.rand(B, H, W) < 0.6, np.clip(c, 0, H - 1), c) - yy).astype(np.float32)
    if W <= 2:
        c = rs.randint(-2, 8 * (W - 1) + 3, (B, H, W)) / 8.0
        dx = (np.where(rs.rand(B, H, W) < 0.6, np.clip(c, 0, W - 1), c) - xx).astype(np.float32)
    e = 0.125
    dy[0, 0, 0] = 0.0; dx[0, 0, 0] = 0.0                                        # (0, 0) exactly
    dy[0, H - 1, W - 1] = 0.0; dx[0, H - 1, W - 1] = 0.0                        # (H-1, W-1) exactly: both clamps, fy = fx = 1
    if W >= 5:
        dy[0, 0, 1] = -e; dx[0, 0, 1] = 0.0                                     # row -1/8: outside
        dy[0, H - 1, 2] = e; dx[0, H - 1, 2] = 0.0                              # row H-1+1/8: outside
        dy[0, H - 1, W - 2] = 0.0; dx[0, H - 1, W - 2] = 0.5                    # row H-1 exactly, column between two pixels
    if H >= 5:
        dy[0, 1, 0] = 0.0; dx[0, 1, 0] = -e                                     # column -1/8: outside
        dy[0, 2, W - 1] = 0.0; dx[0, 2, W - 1] = e                              # column W-1+1/8: outside
        dy[0, H - 2, W - 1] = 0.5; dx[0, H - 2, W - 1] = 0.0                    # column W-1 exactly, row between two pixels
    return img, dy, dx


def warp_coords(dy, dx):
    H, W = dy.shape[-2:]
    yy, xx = np.mgrid[0:H, 0:W]
    return yy + dy.astype(np.float64), xx + dx.astype(np.float64)


def warp_outside(dy, dx):
    """The pixels whose coordinate lies outside [0, H-1] x [0, W-1]: exactly 0 in the result."""
    H, W = dy.shape[-2:]
    cy, cx = warp_coords(dy, dx)
    return (cy < 0) | (cy > H - 1) | (cx < 0) | (cx > W - 1)


def warp_bilinear(img, dy, dx):
    """scipy.ndimage.map_coordinates(order=1, mode='constant', cval=0) in fp64, plane by plane."""
    cy, cx = warp_coords(dy, dx)
    return np.stack([ndimage.map_coordinates(img[b].astype(np.float64), [cy[b], cx[b]], order=1, mode="constant", cval=0.0)
                     for b in range(img.shape[0])])


def warp_bilinear_numpy(img, dy, dx):
    """The same in plain numpy (fp64): what the CPU test holds scipy's degenerate shapes (H = 1, W = 1) against."""
    B, H, W = img.shape
    cy, cx = warp_coords(dy, dx)
    out = np.zeros((B, H, W))
    inside = ~warp_outside(dy, dx)
    y0 = np.clip(np.floor(cy).astype(int), 0, max(H - 2, 0)); x0 = np.clip(np.floor(cx).astype(int), 0, max(W - 2, 0))
    y1 = np.minimum(y0 + 1, H - 1); x1 = np.minimum(x0 + 1, W - 1)
    fy = cy - y0; fx = cx - x0
    for b in range(B):
        im = img[b].astype(np.float64)
        v = (1 - fy[b]) * ((1 - fx[b]) * im[y0[b], x0[b]] + fx[b] * im[y0[b], x1[b]]) \
            + fy[b] * ((1 - fx[b]) * im[y1[b], x0[b]] + fx[b] * im[y1[b], x1[b]])
        out[b] = np.where(inside[b], v, 0.0)
    return out


def warp_bound(img):
    """4 * 2^-23 * max|img|: the coordinates, fy, fx, 1 - fy and 1 - fx are exact (multiples of 1/8), which leaves the five
    roundings of (1-fy) * ((1-fx) v00 + fx v01) + fy * ((1-fx) v10 + fx v11) on values <= max|img|."""
    return 4 * 2.0 ** -23 * float(np.abs(img).max())


# ---- reflect pad + rotation + centre crop -----------------------------------------------------------------------------------
ROT_CASES = [(22, 28, 8, 17.5), (22, 28, 8, 45.0), (23, 28, 8, -100.25), (20, 30, 8, 30.0), (2, 40, 4, 77.0), (36, 20, 6, 333.3),
             (22, 28, 8, 90.0)]                                  # (n, pad, S, deg)
ROT_B = 2                                                        # images per case
ROT_TOL = 2e-5                                                   # of the value range: the project's figure for the fp32 path
ROT_BATCH64 = (22, 28, 8)                                        # (n, pad, S) of the B = 64 call


def reflect_rotate_crop(img, deg, pad, S):
    """One image [n,n] (used as fp64): np.pad(img, pad, 'reflect') -> scipy.ndimage.rotate (cubic spline, reshape=True,
    mode='constant') -> the centre S x S.  oracle/aux_ref.reflect_rotate_crop with pad as a parameter of its own; the value
    BEFORE any conversion to an integer image."""
    p = np.pad(img.astype(np.float64), pad_width=pad, mode="reflect")
    rot = ndimage.rotate(p, deg)
    h, w = rot.shape
    t = h // 2 - S // 2; l = w // 2 - S // 2
    return rot[t:t + S, l:l + S]


def to_levels(t, levels):
    """scipy's conversion to an unsigned integer image: (type) min(t > 0 ? t + 0.5 : 0, levels)."""
    return np.floor(np.minimum(np.where(t > 0, t + 0.5, 0.0), float(levels)))


def half_level_distance(t, levels):
    """Distance of every value to the nearest rounding boundary k + 0.5, k = 0 .. levels - 1 (below 0.5 everything becomes 0,
    from levels - 0.5 on everything becomes levels)."""
    k = np.clip(np.round(t - 0.5), 0, levels - 1)
    return np.abs(t - (k + 0.5))


def level_margin(img, levels):
    """What the fp32 path may be off by: ROT_TOL of the larger of the level count and the image's value range."""
    return ROT_TOL * max(float(levels), float(np.ptp(img)))


def float_images(n, seed=0):
    """ROT_B asymmetric grey images in 0 .. 255 (fp32) for the float mode."""
    rs = np.random.RandomState(100 + seed)
    return (rs.rand(ROT_B, n, n) * 255).astype(np.float32)


def integer_images(n, seed):
    """ROT_B images of integer grey values 0 .. 255 (fp32): rotations by multiples of 90 degrees permute them exactly."""
    rs = np.random.RandomState(200 + seed)
    return rs.randint(0, 256, (ROT_B, n, n)).astype(np.float32)


def block_images(n, levels, seed):
    """ROT_B high-contrast block images (fp32): random 2 x 2 blocks of two values.
    levels = 255: the values 0 and 255, so the cubic spline overshoots above 255.5 and below 0 next to an edge and both clamps
    run, while pixels on an edge take every value in between.
    levels = 65535: the fp32 path is good to ROT_TOL of the value range, which for a 0 .. 65535 image is 1.3 levels: no value
    strictly between two levels is then provably on one side of its boundary.  The values are -1e7 and +1e7 instead: a pixel is
    either far below 0, far above 65535.5 (both clamps, and the clamp at 65535 and not at 255), or - for the seeds
    rotate_seed() accepts - never in between."""
    rs = np.random.RandomState(300 + seed)
    bs = 2 if n >= 8 else 1                                      # (blocks of one pixel in the 2 x 2 image)
    nb = (n + bs - 1) // bs
    bits = rs.rand(ROT_B, nb, nb) > 0.5
    up = np.kron(bits, np.ones((bs, bs), bool))[:, :n, :n]
    lo, hi = (0.0, 255.0) if levels == 255 else (-1e7, 1e7)
    return np.where(up, hi, lo).astype(np.float32)


def well_posed(img, t, levels):
    """t: fp64 values before rounding.  (far from every boundary, upper clamp runs, lower clamp runs)"""
    m = level_margin(img, levels)
    return bool((half_level_distance(t, levels) >= m).all()), bool((t > levels + 0.5).any()), bool((t < 0).any())


def clamps_expected(case, levels):
    """Every block image must run both clamps, but for one: the reflect pad of a 2 x 2 image of 0 / 255 is a pattern of
    period 2, whose spline interpolant stays inside 0 .. 255 (no overshoot at the Nyquist frequency)."""
    return not (ROT_CASES[case][0] < 8 and levels == 255)


@functools.lru_cache(maxsize=None)
def rotate_seed(case, levels):
    """The first seed whose block images make the integer comparison of ROT_CASES[case] well-posed (see well_posed); None if
    200 seeds do not hold one - tests/test_aux_ops_cpu.py asserts that there is one and restates the three conditions."""
    n, pad, S, deg = ROT_CASES[case]
    for seed in range(200):
        img = block_images(n, levels, seed)
        t = np.stack([reflect_rotate_crop(im, deg, pad, S) for im in img])
        far, up, down = well_posed(img, t, levels)
        if far and ((up and down) or not clamps_expected(case, levels)) and np.ptp(t) > 0:
            return seed
    return None
