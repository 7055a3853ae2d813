"""numpy/scipy restatement of the reference's label preprocessing and weighted crop distribution (imported like
instances_ref): what data.preprocess_gt / binary_target / crop_distribution and the two entry points behind them
(unet_carve_borders, unet_crop_counts) are held to, and the seeded id maps the tests feed them.  Pinned to the reference's own
outputs (tests/golden/prepare_golden.npz) and to hand-worked answers by tests/test_prepare_cpu.py.

  carve_literal(ids, reach)   the reference's loop restated: per id, a (2 reach + 1)^2 maximum filter of the cell's 0/255 image
                              (zero outside the image), the ring it gained added to mask_global; gt = max(0, ids - mask_global)
  carve_fast(ids, reach)      the same numbers without a loop over ids: the (2 reach + 1)^2 shifted planes of the zero-padded id
                              map, own id and background blanked, sorted per pixel, distinct values counted
  crop_counts(mask, ..)       window counts from a summed-area table
  crop_probabilities(c, ..)   the reference's expression with scipy.stats.norm.pdf, per image

Ids outside [0, 2^24) are background everywhere and are counted (the entry point's status word).
"""
import numpy as np
from scipy import ndimage
from scipy.stats import norm

ID_LIMIT = 1 << 24


def clean(ids):
    """(int64 id map with out-of-range ids (NaN included) set to 0, how many there were)"""
    a = np.asarray(ids)
    if a.dtype.kind == "f":
        ok = (a >= 0) & (a < ID_LIMIT)                      # NaN fails both
        a = np.where(ok, a, 0).astype(np.int64)
    else:
        a = a.astype(np.int64)
        ok = (a >= 0) & (a < ID_LIMIT)
        a = np.where(ok, a, 0)
    return a, int((~ok).sum())


def outputs(ids, n):
    """(gt int64, mask_global int64, gt_bin uint8) from the cleaned ids and the count n of foreign ids per window"""
    edges = 255 * n
    gt = np.maximum(0, ids - edges)
    return gt, edges, np.where(gt > 0, 255, 0).astype(np.uint8)


def foreign_literal(ids, reach):
    size = 2 * reach + 1
    n = np.zeros(ids.shape, np.int64)
    for c in np.unique(ids):
        if c == 0:
            continue
        cell = ids == c
        n += ndimage.maximum_filter(cell.astype(np.uint8), size=size, mode="constant", cval=0).astype(bool) & ~cell
    return n


def foreign_fast(ids, reach, rows=128):
    H, W = ids.shape
    pad = np.pad(ids, reach).astype(np.int32)                # ids are below 2^24: half the bytes to stack and sort
    n = np.zeros((H, W), np.int64)
    for y0 in range(0, H, rows):                             # in bands of rows: the stack of planes stays small
        y1 = min(H, y0 + rows)
        own = pad[reach + y0:reach + y1, reach:reach + W]
        planes = np.stack([pad[y0 + dy:y1 + dy, dx:dx + W] for dy in range(2 * reach + 1) for dx in range(2 * reach + 1)], axis=-1)
        planes = np.where(planes == own[..., None], 0, planes).reshape((y1 - y0) * W, -1)
        busy = planes.any(axis=1)                            # pixels with a foreign id in reach; the others keep n = 0
        s = np.sort(planes[busy], axis=1)
        band = np.zeros((y1 - y0) * W, np.int64)
        band[busy] = (s[:, 0] != 0).astype(np.int64) + ((s[:, 1:] != s[:, :-1]) & (s[:, 1:] != 0)).sum(axis=1)
        n[y0:y1] = band.reshape(y1 - y0, W)
    return n


def carve_literal(ids, reach=4):
    """One image [H,W]: gt, mask_global, gt_bin, number of out-of-range pixels."""
    a, bad = clean(ids)
    return outputs(a, foreign_literal(a, reach)) + (bad,)


def carve_fast(ids, reach=4):
    a, bad = clean(ids)
    return outputs(a, foreign_fast(a, reach)) + (bad,)


def carve_batch(ids, reach=4):
    """[B,H,W] -> gt [B,H,W] float32, edges float32, bin uint8, status [B] (the entry point's outputs)"""
    per = [carve_fast(i, reach) for i in ids]
    return (np.stack([p[0] for p in per]).astype(np.float32), np.stack([p[1] for p in per]).astype(np.float32),
            np.stack([p[2] for p in per]), np.array([p[3] for p in per], np.int64))


def crop_pairs(H, W, crop, skip=10):
    return [(ii, jj) for ii in range(0, H - crop, skip) for jj in range(0, W - crop, skip)]


def crop_counts(mask, crop, skip=10):
    """One image [H,W]: int64 [ny, nx], the non-zero pixels of every window, from a summed-area table."""
    fg = np.asarray(mask) != 0
    H, W = fg.shape
    sat = np.zeros((H + 1, W + 1), np.int64)
    sat[1:, 1:] = fg.cumsum(0).cumsum(1)
    ii = np.arange(0, H - crop, skip)[:, None]
    jj = np.arange(0, W - crop, skip)[None, :]
    return sat[ii + crop, jj + crop] - sat[ii, jj + crop] - sat[ii + crop, jj] + sat[ii, jj]


def crop_probabilities(counts, crop):
    """One image: float64 [ny * nx] as data.py:70-82 forms it from the mean of each {0,255} window."""
    p = []
    for c in np.asarray(counts).ravel():
        x = ((255.0 * float(c)) / (crop * crop)) / 255
        p.append(0 if x < 0.1 or x > 0.9 else 10 * norm.pdf(x, loc=0.5, scale=0.05))
    if np.sum(p) == 0:
        return np.ones((len(p),)) / len(p)
    return p / np.sum(p)


# ---- seeded inputs --------------------------------------------------------------------------------------------------------

KINDS = ["discs", "discs_hi", "speckle", "zeros", "one", "two_piece", "edges"]


def _paint_discs(rs, H, W, ids):
    out = np.zeros((H, W), np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    rmax = max(1.5, min(H, W) / 5)
    for c in ids:
        cy, cx, r = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(0.5 * rmax, rmax)
        out[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = c      # a later disc overwrites: cells touch, some end up in pieces
    return out


def ids_case(kind, seed, H, W):
    """One seeded id map [H,W] int64 of a kind:
    discs      overlapping discs, ids 1..n              discs_hi   the same with ids 200 + 37 k (crossing 255 and 510)
    speckle    each pixel foreground with probability 0.4, every one with an id of its own (the most distinct ids a window holds)
    zeros / one   no cell / one id everywhere
    two_piece  stripes of ONE id two columns apart (pieces closer than the reach, which must not carve each other), and a
               second id in the lowest quarter
    edges      cells cut by every image edge and corner"""
    rs = np.random.RandomState(11000 + seed)
    n = int(np.clip(H * W // 150, 2, 60))
    if kind == "discs":
        return _paint_discs(rs, H, W, range(1, n + 1))
    if kind == "discs_hi":
        return _paint_discs(rs, H, W, [200 + 37 * k for k in range(n)])
    if kind == "speckle":
        return np.where(rs.rand(H, W) < 0.4, 1 + np.arange(H * W).reshape(H, W), 0)
    if kind == "zeros":
        return np.zeros((H, W), np.int64)
    if kind == "one":
        return np.full((H, W), 5, np.int64)
    if kind == "two_piece":
        out = np.zeros((H, W), np.int64)
        out[:, ::3] = 3
        out[3 * H // 4 + 1:, 1::3] = 9
        return out
    assert kind == "edges"
    out = np.zeros((H, W), np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    r = min(H, W) / 4 + 1
    centres = [(0, W / 2), (H - 1, W / 3), (H / 2, 0), (2 * H / 3, W - 1), (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for k, (cy, cx) in enumerate(centres):
        out[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = 300 * (k + 1)
    return out


def ids_batch(kind, seed, B, H, W):
    return np.stack([ids_case(kind, seed * 7 + b, H, W) for b in range(B)])
