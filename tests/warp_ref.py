"""numpy/scipy restatement of the topology-preserving warp behind the ISBI 2012 warping error (Jain et al. 2010; imported like
rand_ref): what functions.warp_labels / functions.warping_error and the unet_warp_* entry points are held to, and the seeded
inputs the tests feed them.

  simple_table()          the 256 codes of the 8 neighbours (clockwise from NW, bits 0..7), from the component definition with
                          scipy.ndimage.label: exactly one 4-connected foreground component that holds a 4-neighbour of the
                          pixel, exactly one 8-connected background component
  may_mask(gt, reach, mask)   interior AND user mask AND (exact squared distance to the other class of gt <= floor(reach^2))
  warp(gt, pred, may)     passes 0..3 of the pixels with (y & 1) * 2 + (x & 1) == s, all simple candidates of a pass at once;
                          sweeps until one flips nothing
  warp_sequential(...)    the same sweeps, one pixel at a time in raster order inside every pass
  scores(pred, gt, ...)   every field of functions.WarpScores
"""
import math

import numpy as np
from scipy import ndimage

import instances_ref

# the 8 neighbours clockwise from NW: bit k of a code is the neighbour at (dy, dx) = NEIGHBOURS[k]
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1))
CROSS = ndimage.generate_binary_structure(2, 1)
FULL = ndimage.generate_binary_structure(2, 2)
REACHES = (None, 0, 1, 2.5, 5)


def code_patch(code):
    """The 3 x 3 neighbourhood of a code as a bool array, the centre False."""
    p = np.zeros((3, 3), bool)
    for k, (dy, dx) in enumerate(NEIGHBOURS):
        p[1 + dy, 1 + dx] = bool(code >> k & 1)
    return p


def is_simple(code, fg_structure=CROSS, bg_structure=FULL):
    """The component definition: foreground connected by fg_structure, background by bg_structure, the centre in neither."""
    fg = code_patch(code)
    bg = ~fg
    bg[1, 1] = False
    lab, _ = ndimage.label(fg, fg_structure)
    if fg_structure is CROSS:
        touching = {int(lab[y, x]) for y, x in ((0, 1), (1, 2), (2, 1), (1, 0)) if lab[y, x]}
        n_bg = ndimage.label(bg, bg_structure)[1]
        return len(touching) == 1 and n_bg == 1
    # the roles swapped: foreground 8-connected (every neighbour touches the centre), background 4-connected and counted
    # only where it holds a 4-neighbour of the centre
    n_fg = ndimage.label(fg, fg_structure)[1]
    labb, _ = ndimage.label(bg, bg_structure)
    touching = {int(labb[y, x]) for y, x in ((0, 1), (1, 2), (2, 1), (1, 0)) if labb[y, x]}
    return n_fg == 1 and len(touching) == 1


_TABLE = None


def simple_table():
    global _TABLE
    if _TABLE is None:
        _TABLE = np.array([is_simple(c) for c in range(256)], bool)
    return _TABLE


def codes(L):
    """The neighbour code of every interior pixel of a bool image, 0 on the border (which never flips)."""
    H, W = L.shape
    c = np.zeros((H, W), np.int32)
    if H < 3 or W < 3:
        return c
    for k, (dy, dx) in enumerate(NEIGHBOURS):
        c[1:-1, 1:-1] |= L[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx].astype(np.int32) << k
    return c


def interior(H, W):
    m = np.zeros((H, W), bool)
    m[1:-1, 1:-1] = True
    return m


def dist2(reach):
    return int(math.floor(float(reach) ** 2))


def may_mask(gt, reach=None, mask=None):
    """One image: the pixels that may flip."""
    g = np.asarray(gt) != 0
    may = interior(*g.shape)
    if mask is not None:
        may &= np.asarray(mask) != 0
    if reach is not None:
        if g.all() or not g.any():
            return np.zeros_like(may)
        # distance_transform_edt: the distance of every non-zero pixel to the nearest zero pixel
        d = np.where(g, ndimage.distance_transform_edt(g), ndimage.distance_transform_edt(~g))
        may &= np.rint(d * d).astype(np.int64) <= dist2(reach)
    return may


def classes(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy & 1) * 2 + (xx & 1)


def warp(gt, pred, may, max_sweeps=None):
    """One image, foreground 4-connected.  Returns (L bool, flips per pixel int32, sweeps counting the final empty one, flips per
    sweep as a list)."""
    L, T, may = np.asarray(gt) != 0, np.asarray(pred) != 0, np.asarray(may) != 0
    L = L.copy()
    H, W = L.shape
    may = may & interior(H, W)
    cls, table = classes(H, W), simple_table()
    count = np.zeros((H, W), np.int32)
    per_sweep = []
    while max_sweeps is None or len(per_sweep) < max_sweeps:
        n = 0
        for s in range(4):
            flip = may & (L != T) & (cls == s) & table[codes(L)]
            L[flip] = T[flip]
            count += flip
            n += int(flip.sum())
        per_sweep.append(n)
        if n == 0:
            break
    return L, count, len(per_sweep), per_sweep


def warp_sequential(gt, pred, may):
    """The same sweeps with the candidates of a pass taken one by one in raster order, each tested in the image as it is then."""
    L, T, may = np.asarray(gt) != 0, np.asarray(pred) != 0, np.asarray(may) != 0
    L = L.copy()
    H, W = L.shape
    may = may & interior(H, W)
    cls, table = classes(H, W), simple_table()
    sweeps = 0
    while True:
        n = 0
        sweeps += 1
        for s in range(4):
            for y, x in zip(*np.nonzero(may & (L != T) & (cls == s))):
                c = 0
                for k, (dy, dx) in enumerate(NEIGHBOURS):
                    c |= int(L[y + dy, x + dx]) << k
                if table[c]:
                    L[y, x] = T[y, x]
                    n += 1
        if n == 0:
            return L, sweeps


def warp_batch(gt, pred, reach=None, mask=None, connectivity=4):
    """[B,H,W] inputs (foreground = value != 0) -> dict of what the device op returns: warped int32 {0,1}, mismatch_map bool,
    and int64 [B] mismatch, mismatch_before, flips; sweeps = the maximum over the batch; may, count (flips per pixel)."""
    gt, pred = np.asarray(gt) != 0, np.asarray(pred) != 0
    B, H, W = gt.shape
    out = {k: [] for k in ("warped", "mismatch_map", "mismatch", "mismatch_before", "flips", "sweeps", "may", "count")}
    for b in range(B):
        may = may_mask(gt[b], reach, None if mask is None else mask[b])
        g, p = (~gt[b], ~pred[b]) if connectivity == 8 else (gt[b], pred[b])
        L, count, sweeps, _ = warp(g, p, may)
        out["mismatch_map"].append(L != p)
        if connectivity == 8:
            L = ~L
        out["warped"].append(L.astype(np.int32))
        out["mismatch"].append(int((L != pred[b]).sum()))
        out["mismatch_before"].append(int((gt[b] != pred[b]).sum()))
        out["flips"].append(int(count.sum()))
        out["sweeps"].append(sweeps)
        out["may"].append(may)
        out["count"].append(count)
    r = {k: np.stack(v) if k in ("warped", "mismatch_map", "may", "count") else np.array(v, np.int64) for k, v in out.items()}
    r["sweeps"] = int(r["sweeps"].max())
    return r


def scores(pred, gt, reach=None, mask=None, connectivity=4):
    """Every field of functions.WarpScores for [B,H,W] inputs, as a dict."""
    r = warp_batch(gt, pred, reach, mask, connectivity)
    H, W = r["warped"].shape[1:]
    r["warping_error"] = r["mismatch"] / np.float64(H * W)
    r["warping_error_mean"] = np.float64(r["warping_error"].mean())
    r["error_regions"] = np.array([ndimage.label(m, CROSS)[1] for m in r["mismatch_map"]], np.int64)
    return r


def components(L):
    """(4-connected foreground components, 8-connected background components) of a bool image."""
    L = np.asarray(L) != 0
    return int(ndimage.label(L, CROSS)[1]), int(ndimage.label(~L, FULL)[1])


# ---- seeded inputs --------------------------------------------------------------------------------------------------------

def shifted(m, dy, dx):
    """m moved by (dy, dx), background coming in at the edges."""
    H, W = m.shape
    out = np.zeros_like(m)
    out[max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)] = m[max(0, -dy):H + min(0, -dy), max(0, -dx):W + min(0, -dx)]
    return out


def disturbed(rs, m, speckle=0.01):
    """A prediction for the mask m: shifted by up to 2 pixels, dilated or eroded once, and speckled."""
    m = np.asarray(m) != 0
    dy, dx = (int(v) for v in rs.randint(-2, 3, 2))
    p = shifted(m, dy, dx)
    if min(m.shape) >= 3:
        p = ndimage.binary_dilation(p, CROSS) if rs.rand() < 0.5 else ndimage.binary_erosion(p, FULL)
    return p ^ (rs.rand(*m.shape) < speckle)


def corridor(H=9, W=400):
    """A 2-pixel gt stub at the left end of the middle row against a line through the whole row: the stub grows by one pixel
    per pass of the right class, two pixels per sweep."""
    gt, pred = np.zeros((H, W), bool), np.zeros((H, W), bool)
    gt[H // 2, 1:3] = True
    pred[H // 2, 1:W - 1] = True
    return gt, pred


def cells_pair(seed, n, H, W):
    """A cell image (instances_ref.cells_case's ground truth) against a shifted, dilated and speckled copy."""
    g = instances_ref.cells_case(seed, n, H, W)[0] > 0
    rs = np.random.RandomState(4200 + seed)
    p = ndimage.binary_dilation(shifted(g, 3, -2), FULL, iterations=2) ^ (rs.rand(H, W) < 0.002)
    return g, p


def size_cases(H, W, seed=0):
    """[(name, gt uint8 [B,H,W], pred uint8 [B,H,W])] at one size: discs, serpentine, comb and cells against disturbed copies
    (B 1-4 as instances_ref.mask_batch draws it), and a batch of four that holds an all-background image, an all-foreground
    image and gt == pred next to a busy one."""
    rs = np.random.RandomState(31000 + 131 * H + W + seed)
    out = []
    for kind in ("discs", "serpentine", "comb"):
        g = instances_ref.mask_batch(kind, seed + H + W, H, W) != 0
        p = np.stack([disturbed(rs, m, 0.02 if kind == "discs" else 0.005) for m in g])
        out.append((kind, g.astype(np.uint8), p.astype(np.uint8)))
    n = max(1, H * W // 400)
    g4 = np.zeros((4, H, W), bool)
    p4 = np.zeros((4, H, W), bool)
    g4[0] = instances_ref.cells_case(seed + 1, n, H, W)[0] > 0
    p4[0] = disturbed(rs, g4[0], 0.01)
    p4[1] = instances_ref.discs(rs, H, W, 5)                 # all-background gt against discs
    g4[2] = True                                             # all-foreground gt against discs
    p4[2] = instances_ref.discs(rs, H, W, 5)
    g4[3] = p4[3] = instances_ref.discs(rs, H, W, 7)         # nothing to do
    out.append(("mixed", g4.astype(np.uint8), p4.astype(np.uint8)))
    return out
