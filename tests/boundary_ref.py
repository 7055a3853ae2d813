"""Boundary scores restated with numpy compares and Python integers: what tests/test_boundary_gpu.py compares unet_mask_boundary,
unet_surface_sums and functions.boundary_scores with, and what tests/test_boundary_cpu.py pins to scipy and to answers worked by hand.

The contour comes from shifted compares, d2 from brute force over all pairs of contour pixels, the order statistics from sorted(),
the sum from math.fsum of math.sqrt, the scores from Python floats and fractions.  Nothing here shares code with the library or
with functions.scores_from_surface."""
import functools
import math
from fractions import Fraction

import numpy as np


def region(mask, select=None):
    mask = np.asarray(mask)
    return mask != 0 if select is None else mask == select


def contour(reg, connectivity=4, edge="background"):
    """bool [H,W]: the pixels of the region with a neighbour outside it.  Past the image lies background, or nothing."""
    reg = np.asarray(reg, bool)
    H, W = reg.shape
    pad = np.pad(reg, 1, constant_values=edge != "background")          # 'ignore': a pixel past the image is never outside
    gap = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dy, dx) != (0, 0) and (connectivity == 8 or dy == 0 or dx == 0):
                gap |= ~pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return reg & gap


def directed_d2(ca, cb):
    """int64 [H,W]: at every pixel of contour ca the smallest squared distance to a pixel of contour cb, -1 elsewhere; all -1 when
    cb is empty.  Every pair is looked at."""
    out = np.full(ca.shape, -1, np.int64)
    ay, ax = (v.astype(np.int64) for v in np.nonzero(ca))
    by, bx = (v.astype(np.int64) for v in np.nonzero(cb))
    if len(by) == 0:
        return out
    for s in range(0, len(ay), 4096):
        y, x = ay[s:s + 4096], ax[s:s + 4096]
        out[y, x] = ((y[:, None] - by[None]) ** 2 + (x[:, None] - bx[None]) ** 2).min(axis=1)
    return out


def record(ca, cb, q_num, q_den, t2):
    """The ten words of one direction as Python numbers: [n, max_d2, lo, hi, rem, within x 4, sum], and the d2 plane."""
    plane = directed_d2(ca, cb)
    n = int(ca.sum())
    if n == 0 or not cb.any():
        return [n, 0, 0, 0, 0, 0, 0, 0, 0, 0.0], plane
    d = sorted(int(v) for v in plane[ca])
    j, rem = divmod((n - 1) * q_num, q_den)
    within = [sum(v <= t for v in d) for t in t2] + [0] * (4 - len(t2))
    return [n, d[-1], d[j], d[min(j + 1, n - 1)], rem] + within + [math.fsum(math.sqrt(v) for v in d)], plane


def fraction_of(percentile):
    q = Fraction(percentile) / 100
    return q.numerator, q.denominator


def t2_of(tolerances):
    return [math.floor(Fraction(t) ** 2) for t in tolerances]


def surface(pred, gt, tolerances=(1.0,), percentile=95, select=None, connectivity=4, edge="background"):
    """One image: {"bits": uint8 [H,W] (bit 0 the contour of pred, bit 1 of gt), "record": [2][10] Python numbers,
    "d2": the two int64 planes, "t2", "q"}"""
    cp, cg = (contour(region(m, select), connectivity, edge) for m in (pred, gt))
    q_num, q_den = fraction_of(percentile)
    t2 = t2_of(tolerances)
    pg, d_pg = record(cp, cg, q_num, q_den, t2)
    gp, d_gp = record(cg, cp, q_num, q_den, t2)
    return {"bits": cp.astype(np.uint8) | cg.astype(np.uint8) << 1, "record": [pg, gp], "d2": [d_pg, d_gp], "t2": t2, "q": (q_num, q_den)}


def directed_percentile(rec, q_den):
    lo, hi = math.sqrt(rec[2]), math.sqrt(rec[3])
    return lo + rec[4] / q_den * (hi - lo)


def scores(s, spacing=1.0):
    """The scores of one image from surface()'s result, as a dict of Python floats (lists per tolerance)."""
    pg, gp = s["record"]
    k, (q_num, q_den) = len(s["t2"]), s["q"]
    n_p, n_g = pg[0], gp[0]
    out = {"n_pred": n_p, "n_gt": n_g}
    if n_p == 0 or n_g == 0:
        both = n_p == 0 and n_g == 0
        for f in ("hausdorff", "hd_percentile", "assd"):
            out[f] = 0.0 if both else math.inf
        for f in ("nsd", "boundary_f1"):
            out[f] = [1.0 if both else 0.0] * k
        out["precision"] = [math.nan if n_p == 0 else 0.0] * k
        out["recall"] = [math.nan if n_g == 0 else 0.0] * k
        return out
    out["hausdorff"] = math.sqrt(max(pg[1], gp[1])) * spacing
    out["hd_percentile"] = max(directed_percentile(pg, q_den), directed_percentile(gp, q_den)) * spacing
    out["assd"] = (pg[9] + gp[9]) / (n_p + n_g) * spacing
    out["nsd"] = [(pg[5 + i] + gp[5 + i]) / (n_p + n_g) for i in range(k)]
    out["precision"] = [pg[5 + i] / n_p for i in range(k)]
    out["recall"] = [gp[5 + i] / n_g for i in range(k)]
    out["boundary_f1"] = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(out["precision"], out["recall"])]
    return out


# ---- the named cases ------------------------------------------------------------------------------------------------------

SIZES = [(1, 1), (1, 9), (9, 1), (3, 3), (5, 7), (6, 63), (6, 64), (6, 65), (3, 257)]


def random_pair(H, W, seed=0):
    """Two uint8 masks of one size that mostly agree"""
    rs = np.random.RandomState(6000 + 131 * H + W + seed)
    a = rs.rand(H, W) < rs.uniform(0.3, 0.8)
    b = a ^ (rs.rand(H, W) < 0.15)
    return a.astype(np.uint8), b.astype(np.uint8)


def pixels(H, W, *yx):
    m = np.zeros((H, W), np.uint8)
    for y, x in yx:
        m[y, x] = 1
    return m


def corners_case():
    """70 x 300, one pixel in each of two opposite corners: d2 = 69^2 + 299^2 in both directions"""
    return pixels(70, 300, (0, 0)), pixels(70, 300, (69, 299))


def strip_case(H):
    """H x 1500, row 0: the contour of pred is 4, 25, 1030^2 and 1449^2 away from the one pixel of gt: 1030^2 is just above 2^20
    and 1449^2 just above 2^21, so neighbouring order statistics differ in the top radix digit"""
    assert 1 << 21 > 1030 ** 2 > 1 << 20 and 1449 ** 2 > 1 << 21 > 1448 ** 2
    return pixels(H, 1500, (0, 11), (0, 430), (0, 1455), (0, 1458)), pixels(H, 1500, (0, 1460))


def equal_case():
    """Every d2 of pred -> gt is 9 (n = 2); gt -> pred has n = 1"""
    return pixels(3, 11, (1, 2), (1, 8)), pixels(3, 11, (1, 5))


def square_case():
    """A 5 x 5 square against the same square shifted by 2 columns, in 11 x 13"""
    a, b = np.zeros((11, 13), np.uint8), np.zeros((11, 13), np.uint8)
    a[3:8, 3:8] = 1
    b[3:8, 5:10] = 1
    return a, b


def batch_case(H=9, W=14):
    """B = 3: an empty, a full and an ordinary image"""
    a, b = random_pair(H, W, 5)
    return np.stack([np.zeros_like(a), np.ones_like(a), a]), np.stack([b, np.ones_like(a), b])


def cells_pair():
    import instances_ref
    gt, pred = instances_ref.cells_case(4, 12, 64, 80)
    return (pred > 0).astype(np.uint8), (gt > 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def named_cases():
    """[(name, pred [H,W], gt [H,W])]"""
    out = [("random %dx%d" % hw, *random_pair(*hw)) for hw in SIZES]
    out += [("corners", *corners_case()), ("strip 1", *strip_case(1)), ("strip 2", *strip_case(2)), ("equal", *equal_case()),
            ("square", *square_case()), ("line", pixels(5, 9, *[(2, x) for x in range(1, 8)]), pixels(5, 9, *[(3, x) for x in range(9)])),
            ("full", np.ones((4, 6), np.uint8), np.ones((4, 6), np.uint8)),
            ("empty both", np.zeros((4, 6), np.uint8), np.zeros((4, 6), np.uint8)),
            ("empty pred", np.zeros((4, 6), np.uint8), random_pair(4, 6)[1]), ("empty gt", random_pair(4, 6)[0], np.zeros((4, 6), np.uint8))]
    return out
