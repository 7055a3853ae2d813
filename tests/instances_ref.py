"""numpy/scipy restatement of the instance labelling and of the Cell Tracking Challenge SEG measure (imported like
weighted_map_ref): what functions.label_cells / functions.seg_measure and the two entry points behind them are held to, and
the seeded masks and id maps the tests feed them.

  label(mask)             scipy.ndimage.label with the cross structure (4-connectivity): raster numbering by first pixel
  overlaps(gt, pred, ..)  np.bincount areas, np.unique on gt * (np_max + 1) + pred for the pair counts, then the rule
                          2 |g n p| > |g| (strict) -> match, inter; pixels with an id outside its range are counted apart
  seg(gts, preds)         J = inter / (area_gt + area_pred[match] - inter) in float64 per present ground-truth id, 0 unmatched
"""
import numpy as np
from scipy import ndimage

CROSS = ndimage.generate_binary_structure(2, 1)


def label(mask):
    """(labels int32 [H,W], n) of one mask, foreground = value != 0."""
    lab, n = ndimage.label(np.asarray(mask) != 0, CROSS)
    return lab.astype(np.int32), int(n)


def overlaps(gt, pred, ng_max=None, np_max=None):
    """One image.  Returns area_gt [ng_max+1], area_pred [np_max+1], match [ng_max+1], inter [ng_max+1] (int64), the number
    of pixels with an id out of range, and the number of distinct (g, p) pairs with g, p >= 1."""
    gt, pred = np.asarray(gt).astype(np.int64).ravel(), np.asarray(pred).astype(np.int64).ravel()
    ng_max = int(gt.max()) if ng_max is None else ng_max
    np_max = int(pred.max()) if np_max is None else np_max
    ok = (gt >= 0) & (gt <= ng_max) & (pred >= 0) & (pred <= np_max)
    g, p = gt[ok], pred[ok]
    area_gt = np.bincount(g, minlength=ng_max + 1)
    area_pred = np.bincount(p, minlength=np_max + 1)
    both = (g > 0) & (p > 0)
    pairs, counts = np.unique(g[both] * (np_max + 1) + p[both], return_counts=True)
    match = np.zeros(ng_max + 1, np.int64)
    inter = np.zeros(ng_max + 1, np.int64)
    for key, c in zip(pairs, counts):
        gi, pi = divmod(int(key), np_max + 1)
        if 2 * c > area_gt[gi]:
            assert match[gi] == 0
            match[gi], inter[gi] = pi, c
    return area_gt, area_pred, match, inter, int((~ok).sum()), len(pairs)


def jaccards(area_gt, area_pred, match, inter):
    """float64 J per present ground-truth id (area > 0) of one image, in increasing id order."""
    out = []
    for g in range(1, len(area_gt)):
        if area_gt[g] == 0:
            continue
        if match[g] == 0:
            out.append(0.0)
        else:
            out.append(int(inter[g]) / (int(area_gt[g]) + int(area_pred[match[g]]) - int(inter[g])))
    return np.array(out, np.float64)


def seg(gts, preds):
    """SEG of a batch of id maps [B,H,W]: dict with seg, per_image [B], jaccard (list of B arrays), jaccard_sum, n_gt,
    n_matched, n_pred."""
    js, n_matched, n_pred = [], 0, 0
    for gt, pred in zip(gts, preds):
        area_gt, area_pred, match, inter, bad, _ = overlaps(gt, pred)
        assert bad == 0
        js.append(jaccards(area_gt, area_pred, match, inter))
        n_matched += int((match[1:] > 0).sum())
        n_pred += int((area_pred[1:] > 0).sum())
    every = np.concatenate(js) if js else np.zeros(0)
    return {"seg": every.mean() if len(every) else np.float64(np.nan), "jaccard_sum": float(every.sum()), "n_gt": len(every),
            "n_matched": n_matched, "n_pred": n_pred, "jaccard": js,
            "per_image": np.array([j.mean() if len(j) else np.nan for j in js], np.float64)}


# ---- seeded inputs --------------------------------------------------------------------------------------------------------

def discs(rs, H, W, n):
    m = np.zeros((H, W), bool)
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(n):
        cy, cx, r = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(0.5, max(1.0, min(H, W) / 6))
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return m


def serpentine(H, W):
    """One one-pixel-wide path through the whole image: every even row, joined alternately at its right and left end.  It
    crosses every tile border and is one component whose unions form the longest chains the image allows."""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = True
    return m


def comb(H, W):
    """Teeth in the columns x % 4 == 0 that join only in the last row (one component, first pixel (0, 0), joined far below),
    and between them free teeth in the columns x % 4 == 2 that stop two rows short: in raster order the joined comb is 1 and
    the free teeth 2, 3, ... although each of the comb's own teeth starts in row 0 too."""
    m = np.zeros((H, W), bool)
    m[:, 0::4] = True
    m[H - 1, :] = True
    if H > 2:
        m[:H - 2, 2::4] = True
    return m


def mask_batch(kind, seed, H, W):
    """A seeded batch [B,H,W] (B 1-4) of one kind, uint8."""
    rs = np.random.RandomState(7000 + seed)
    B = int(rs.randint(1, 5))
    out = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        if kind == "discs":
            out[b] = discs(rs, H, W, rs.randint(1, 25))
        elif kind.startswith("speckle"):
            out[b] = rs.rand(H, W) < float(kind[7:])
        elif kind == "ones":
            out[b] = 1
        elif kind == "serpentine":
            out[b] = serpentine(H, W) if b % 2 == 0 else serpentine(W, H).T
        elif kind == "comb":
            out[b] = comb(H, W) if b % 2 == 0 else comb(H, W)[:, ::-1]
        else:
            assert kind == "zeros"
    return out


def cells_case(seed, n, H, W, stride=1):
    """A ground-truth id map and a predicted one of an H x W image with about n cells.
    gt: n discs painted in turn (a later one overwrites), ids stride, 2 stride, ...; so ids need not be consecutive, some may
    have no pixel left, and a cell cut in two by a later one is not connected.
    pred: the cells shifted by a few pixels; every fifth one shrunk to a third of its radius (covers 1/9 of the cell: no
    match), every seventh dropped; a few extra discs; then labelled, so cells that touch merge into one prediction."""
    rs = np.random.RandomState(9000 + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    gt = np.zeros((H, W), np.int32)
    fg = np.zeros((H, W), bool)
    dy, dx = rs.randint(-2, 3, 2)
    rmax = max(3.0, 0.33 * np.sqrt(H * W / n))
    for i in range(1, n + 1):
        cy, cx, r = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(0.5 * rmax, rmax)
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        gt[d2 < r * r] = i * stride
        if i % 7 == 0:
            continue
        rp = r / 3 if i % 5 == 0 else r - 1
        fg |= (yy - cy - dy) ** 2 + (xx - cx - dx) ** 2 < rp * rp
    fg |= discs(rs, H, W, 3)
    return gt, label(fg)[0]
