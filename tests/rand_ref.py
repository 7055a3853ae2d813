"""numpy restatement of the nearest-cell growth, of the foreground-restricted pair table and of the Rand / information scores
(imported like instances_ref): what functions.grow_cells / pair_table / rand_scores / rand_from_pairs and the two entry points
behind them (unet_grow_labels, unet_partition_pairs) are held to, and the seeded id maps the tests feed them.  Pinned by
tests/test_rand_cpu.py: grow to the all-pairs definition grow_brute, scores to hand-worked answers.

  grow(labels, max_dist2)        the two-pass integer algorithm: per column the row distance g and the id of the nearest labelled
                                 pixel (above and below at the same g: the smaller id), then per row an [W, W] matrix of the keys
                                 ((x - x')^2 + g(x')^2) << 24 | id(x') and its minimum; with a limit, a minimum beyond it is dropped
  grow_brute(labels, max_dist2)  the definition: for every background pixel the [n_labelled] squared distances, those within the
                                 limit, their minimum, and the smallest id among the labelled pixels at it (small images only)
  pairs(pred, gt)                np.unique of the packed (b, g, p) over the pixels with gt >= 1
  scores(pred, gt, alpha)        the scores from those pairs, in Python integers, fractions and math.fsum
"""
import fractions
import itertools
import math

import numpy as np

import instances_ref
import prepare_ref

ID_BITS = 24
ID_MAX = (1 << ID_BITS) - 1
FAR = 1 << 18                                   # a row distance no image has; FAR^2 << 24 = 2^60 still fits int64
DISTANCES = (None, 0, 1, 1.5, 2, 4, 7.3)        # max_distance of the GPU tests


def dist2(max_distance):
    """floor(max_distance^2) as functions.grow_cells forms it; None stays None."""
    return None if max_distance is None else int(math.floor(float(max_distance) ** 2))


def columns(lab):
    """(g, id) int64 [H,W]: row distance to the nearest labelled pixel of the pixel's column and its id (the smaller id when the
    one above and the one below are equally far); g = FAR, id = 0 where the column has none."""
    H, W = lab.shape
    out = []
    for rows in (range(H), range(H - 1, -1, -1)):
        g, i = np.full(W, FAR, np.int64), np.zeros(W, np.int64)
        G, I = np.empty((H, W), np.int64), np.empty((H, W), np.int64)
        for y in rows:
            m = lab[y] > 0
            g = np.where(m, 0, np.minimum(g + 1, FAR))
            i = np.where(m, lab[y], i)
            G[y], I[y] = g, i
        out.append((G, I))
    (gd, idn), (gu, iup) = out
    up = (gu < gd) | ((gu == gd) & (iup < idn))
    return np.where(up, gu, gd), np.where(up, iup, idn)


def nearest(lab):
    """(d2, id) int64 [H,W] of one id map: squared distance to the nearest labelled pixel and the smallest id at that distance
    (d2 >= FAR^2 and id = 0 in an image without labels).  The row pass of the two-pass algorithm, a band of rows at a time."""
    lab = np.asarray(lab).astype(np.int64)
    H, W = lab.shape
    g, i = columns(lab)
    x = np.arange(W, dtype=np.int64)
    dx2 = (x[:, None] - x[None, :]) ** 2                                  # [x, x']
    key = np.empty((H, W), np.int64)
    band = max(1, (1 << 22) // (W * W))
    for y0 in range(0, H, band):
        k = ((dx2[None] + (g[y0:y0 + band] ** 2)[:, None, :]) << ID_BITS) | i[y0:y0 + band, None, :]
        key[y0:y0 + band] = k.min(axis=2)
    return key >> ID_BITS, key & ID_MAX


def limit(lab, near, max_dist2):
    """The grown map from nearest()'s answer: labelled pixels keep their id; the nearest id where d2 <= max_dist2 (None: any)."""
    d2, i = near
    lab = np.asarray(lab)
    ok = (i > 0) if max_dist2 is None else (i > 0) & (d2 <= max_dist2)
    return np.where(lab != 0, lab, np.where(ok, i, 0)).astype(np.int32)


def grow(labels, max_dist2=None):
    """One id map [H,W] -> int32 [H,W]."""
    return limit(labels, nearest(labels), max_dist2)


def grow_batch(labels, max_dist2s):
    """[B,H,W] -> {max_dist2: int32 [B,H,W]}: one nearest() per image serves every limit."""
    near = [nearest(l) for l in labels]
    return {m: np.stack([limit(l, n, m) for l, n in zip(labels, near)]) for m in max_dist2s}


def grow_brute(labels, max_dist2=None):
    lab = np.asarray(labels).astype(np.int64)
    out = lab.copy()
    ys, xs = np.nonzero(lab)
    ids = lab[ys, xs]
    if len(ids):
        for y, x in zip(*np.nonzero(lab == 0)):
            d = (ys - y) ** 2 + (xs - x) ** 2
            if max_dist2 is not None:
                keep = d <= max_dist2
                if not keep.any():
                    continue
                out[y, x] = ids[keep][d[keep] == d[keep].min()].min()
            else:
                out[y, x] = ids[d == d.min()].min()
    return out.astype(np.int32)


# ---- pairs and scores -------------------------------------------------------------------------------------------------------

def pairs(pred, gt):
    """[B,H,W] id maps -> int64 (b, g, p, n) over the pixels with gt >= 1, sorted by (b, g, p)."""
    pred, gt = np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64)
    b = np.broadcast_to(np.arange(gt.shape[0])[:, None, None], gt.shape)
    fg = gt >= 1
    key, n = np.unique((b[fg] << 48) | (gt[fg] << 24) | pred[fg], return_counts=True)
    return key >> 48, (key >> 24) & ID_MAX, key & ID_MAX, n.astype(np.int64)


SCORES = ("rand_split", "rand_merge", "v_rand", "rand_error", "info_split", "info_merge", "v_info", "voi_split", "voi_merge")
INTS = ("N", "S_pair", "S_pred", "S_gt", "c")


def scores_of_table(table, alpha=0.5):
    """One image: table = {(g, p): n}.  dict of the nine float scores, the five Python integers, and H_pred, H_gt."""
    nan = math.nan
    a, bp, c = {}, {}, 0
    for (g, p), n in table.items():
        a[g] = a.get(g, 0) + n
        if p == 0:
            c += n
        else:
            bp[p] = bp.get(p, 0) + n
    N = sum(a.values())
    S_pair = sum(n * n for (g, p), n in table.items() if p) + c
    S_pred = sum(v * v for v in bp.values()) + c
    S_gt = sum(v * v for v in a.values())
    r = {"N": N, "S_pair": S_pair, "S_pred": S_pred, "S_gt": S_gt, "c": c}
    if N == 0:
        r.update({k: nan for k in SCORES}, H_pred=nan, H_gt=nan)
        return r
    q = lambda num, den: float(fractions.Fraction(num) / den) if den else nan
    al = fractions.Fraction(float(alpha))
    den = al * S_pred + (1 - al) * S_gt
    r.update(rand_split=q(S_pair, S_gt), rand_merge=q(S_pair, S_pred), v_rand=q(S_pair, den), rand_error=q(den - S_pair, den))
    ln = lambda v: v * math.log(v)
    T = ln(N)
    xp = [ln(n) for (g, p), n in table.items() if p]
    xb = [ln(v) for v in bp.values()]
    xa = [ln(v) for v in a.values()]
    H_pred = math.fsum([T] + [-v for v in xb]) / N
    H_gt = math.fsum([T] + [-v for v in xa]) / N
    H_joint = math.fsum([T] + [-v for v in xp]) / N
    I = math.fsum([T] + xp + [-v for v in xa + xb]) / N
    f = lambda num, den: num / den if den else nan
    r.update(info_split=f(I, H_pred), info_merge=f(I, H_gt), v_info=f(I, (1 - alpha) * H_pred + alpha * H_gt),
             voi_split=math.fsum(xa + [-v for v in xp]) / N, voi_merge=math.fsum(xb + [-v for v in xp]) / N,
             H_pred=H_pred, H_gt=H_gt, H_joint=H_joint, I=I)
    return r


def scores(pred, gt, alpha=0.5):
    """[B,H,W] id maps -> dict: float64 [B] per score, int64 [B] per integer, H_pred / H_gt [B], and the two means."""
    B = len(gt)
    b, g, p, n = pairs(pred, gt)
    per = [scores_of_table({(int(gi), int(pi)): int(ni) for gi, pi, ni in zip(g[b == i], p[b == i], n[b == i])}, alpha) for i in range(B)]
    out = {k: np.array([r[k] for r in per], np.float64) for k in SCORES + ("H_pred", "H_gt")}
    out.update({k: np.array([r[k] for r in per], np.int64) for k in INTS})
    for k in ("rand_error", "v_info"):
        v = out[k][~np.isnan(out[k])]
        out[k + "_mean"] = v.mean() if len(v) else np.float64(np.nan)
    return out


def check_scores(got, want):
    """functions.RandScores against rand_scores: integers and Rand scores exactly, information scores to 1e-12 relative."""
    for k in INTS:
        assert getattr(got, k).dtype == np.int64 and np.array_equal(getattr(got, k), want[k]), k
    for k in SCORES[:4]:
        assert getattr(got, k).dtype == np.float64 and np.array_equal(getattr(got, k), want[k], equal_nan=True), k
    for k in SCORES[4:]:
        g, w = getattr(got, k), want[k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), k
        assert np.allclose(g, w, rtol=1e-12, atol=0, equal_nan=True), (k, g, w)
    for k in ("rand_error_mean", "v_info_mean"):
        assert np.allclose(getattr(got, k), want[k], rtol=1e-12, atol=0, equal_nan=True), k


# ---- seeded id maps ---------------------------------------------------------------------------------------------------------

def tie_maps(H, W, ids=(9, 4, 7, 2), half=(1, 2, 5)):
    """Every order of four ids on the corners of squares of side 2 h, h in `half`, with a lone pair beside and below where they
    fit: the centre and the mid-edges of a square are equally far from two or four labelled pixels, within one column (left and
    right edge), between columns (top and bottom edge) or both (centre).  [24,H,W] int32; images too small for a layout leave it out."""
    out = []
    for perm in itertools.permutations(ids):
        m = np.zeros((H, W), np.int32)
        y0 = x0 = 0
        for h in half:
            s = 2 * h
            if y0 >= H or x0 >= W:
                break
            if y0 + s < H and x0 + s < W:
                m[y0, x0], m[y0, x0 + s], m[y0 + s, x0], m[y0 + s, x0 + s] = perm
            elif x0 + s < W:
                m[y0, x0], m[y0, x0 + s] = perm[:2]                # one row: ties between columns only
            elif y0 + s < H:
                m[y0, x0], m[y0 + s, x0] = perm[:2]                # one column
            x0 += s + 3
            y0 += s + 2
        out.append(m)
    return np.stack(out)


def id_cases(H, W, seed):
    """[(name, int32 [B,H,W])], B 1-4: the kinds of id map at which the growth kernels can go wrong."""
    rs = np.random.RandomState(4000 + 31 * H + W + seed)
    out = []
    discs = instances_ref.mask_batch("discs", seed + H, H, W)
    lab = np.stack([instances_ref.label(m)[0] for m in discs]).astype(np.int64)
    out.append(("discs, ids 3 apart", np.where(lab > 0, 3 * lab + 5, 0)))
    top = np.where(lab == 1, ID_MAX, np.where(lab == 2, ID_MAX - 1, lab))
    out.append(("discs, the largest ids", top[:, ::-1, ::-1]))
    for k, (dens, nid) in enumerate(((0.004, 3), (0.02, 3), (0.02, ID_MAX), (0.3, 500), (0.8, ID_MAX))):
        m = instances_ref.mask_batch("speckle%g" % dens, seed + W + k, H, W)
        out.append(("speckle %g, ids up to %d" % (dens, nid), m * rs.randint(1, nid + 1, m.shape)))
    mixed = np.zeros((3, H, W), np.int64)
    mixed[1] = 7
    mixed[2] = lab[0]
    out.append(("all zero, all labelled, discs", mixed))
    lone = np.zeros((4, H, W), np.int64)
    for k, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        lone[k, y, x] = 5 + k
    out.append(("one pixel in a corner", lone))
    edge = np.zeros((4, H, W), np.int64)
    edge[0, H - 1, :] = rs.randint(1, 4, W) * (rs.rand(W) < 0.5)          # the last row only
    edge[1, :, W - 1] = rs.randint(1, 4, H) * (rs.rand(H) < 0.5)          # the last column only
    edge[2, H // 2, W // 2] = 11                                          # discs of the limit around one pixel ...
    edge[3, H // 2, W // 2], edge[3, H - 1, 0] = 11, 3                    # ... and around two
    out.append(("last row, last column, lone centre", edge))
    t = tie_maps(H, W)
    k = rs.randint(0, 21)
    out.append(("ties %d-%d" % (k, k + 3), t[k:k + 4]))
    if H * W > 40000:                           # the numpy row pass costs H W^2 per image: fewer images of each kind
        keep = {"discs, ids 3 apart": slice(0, 2), "speckle 0.004, ids up to 3": slice(0, 1), "speckle 0.3, ids up to 500": slice(0, 1),
                "speckle 0.8, ids up to %d" % ID_MAX: slice(0, 1), "all zero, all labelled, discs": slice(0, 3),
                "one pixel in a corner": slice(3, 4), "last row, last column, lone centre": slice(0, 4, 3)}
        out = [(name, a[keep[name]]) for name, a in out if name in keep] + [out[-1][:1] + (out[-1][1][:2],)]
    return [(name, np.ascontiguousarray(a).astype(np.int32)) for name, a in out]


# ---- seeded pairs of id maps for the pair table and the scores ----------------------------------------------------------------

CASES = ((1, 9, 128, 128), (2, 37, 256, 256), (3, 99, 388, 388))          # seed, cells, H, W of instances_ref.cells_case
E2E = ((33, 20, 96, 96), (4, 9, 96, 96), (2, 20, 128, 128), (29, 9, 128, 128))     # seed, cells, H, W: images where many cells touch


def seeded_pairs():
    """The id maps of the GPU score tests: cells_case at the three sizes (B = 2 each), gt against pred, against a shifted gt and
    against an eroded one."""
    out = []
    for seed, n, H, W in CASES:
        two = [instances_ref.cells_case(s, n, H, W, stride=1 + seed % 2) for s in (seed, seed + 10)]
        gt, pred = (np.stack([t[k] for t in two]) for k in (0, 1))
        out.append(("cells %d" % H, pred, gt))
        out.append(("shifted %d" % H, np.roll(gt, (2, -3), (1, 2)), gt))
        out.append(("eroded %d" % H, np.where(prepare_ref.carve_batch(gt, 2)[2] > 0, gt, 0), gt))
    return out


def speckle_pairs():
    """Hundreds of ids on either side, B = 3, the second image's ground truth all background."""
    rs = np.random.RandomState(77)
    gt = rs.randint(0, 300, (3, 70, 90)).astype(np.int32) * (rs.rand(3, 70, 90) < 0.7)
    pred = rs.randint(0, 400, (3, 70, 90)).astype(np.int32) * (rs.rand(3, 70, 90) < 0.8)
    gt[1] = 0
    return pred.astype(np.int32), gt.astype(np.int32)


def carved_prediction(gt):
    """What a perfect network would predict: the instances of the carved training target (label_cells(binary_target(gt) > 0))."""
    return np.stack([instances_ref.label(prepare_ref.carve_fast(g)[2])[0] for g in gt])
