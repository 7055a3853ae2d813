"""Plain numpy/scipy restatement of the reference's weighted_map (functions.py:7-78), one image at a time, by the
reference's own method: label the 4-connected cells, one exact Euclidean distance transform per component, keep the
two least distances per pixel, w = w_c + w0 * exp(-(d1 + d2)^2 / (2 sig2)) on background in float64, stored as float32.

The one liberty taken: each component's distance transform is computed on its bounding box grown by REACH pixels, and
every pixel outside that box counts as infinitely far.  Such a pixel is more than REACH = 73 px from the component, so
(d1 + d2) > 73 there and 20 * exp(-(d1 + d2)^2 / 50) < 1e-44: it differs from the reference by less than the smallest
float32 subnormal.  It keeps speckle labels with thousands of components affordable on a CPU."""
import math
import os

import numpy as np
from scipy import ndimage

REACH = 73
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)


def components(gt):
    """(label image, count) of the 4-connected foreground, what cv.connectedComponents(connectivity=4) partitions."""
    return ndimage.label(np.asarray(gt) != 0, structure=CROSS)


def distances(gt):
    """(d1, d2, n): float32 distances to the nearest and second-nearest component (inf = none within REACH)."""
    lab, n = components(gt)
    H, W = lab.shape
    d1 = np.full((H, W), np.inf, np.float32)
    d2 = np.full((H, W), np.inf, np.float32)
    for k, sl in enumerate(ndimage.find_objects(lab), start=1):
        y0, y1 = max(sl[0].start - REACH, 0), min(sl[0].stop + REACH, H)
        x0, x1 = max(sl[1].start - REACH, 0), min(sl[1].stop + REACH, W)
        dk = ndimage.distance_transform_edt(lab[y0:y1, x0:x1] != k).astype(np.float32)
        a, b = d1[y0:y1, x0:x1], d2[y0:y1, x0:x1]
        b[...] = np.where(dk < a, a, np.minimum(b, dk))
        a[...] = np.minimum(a, dk)
    return d1, d2, n


def weighted_map(gt, w0=20, sig2=25):
    """gt: [H,W] {0,1} array, integer or float -> float32 [H,W] (the reference's result for that dtype)."""
    gt = np.asarray(gt)
    n1 = int(np.count_nonzero(gt == 1))
    n0 = gt.size - n1
    if n1 == 0 or n0 == 0:
        raise IndexError("one-class image")
    wc_bg = np.float32(n1) / np.float32(n0)                 # counts[1].float() / counts[0].float()
    if not np.issubdtype(gt.dtype, np.floating):
        wc_bg = np.float32(np.trunc(wc_bg))                 # stored in torch.empty_like(gt): integer labels truncate
    d1, d2, n = distances(gt)
    if n == 1:
        d2 = np.zeros_like(d1)
    s = d1.astype(np.float64) + d2.astype(np.float64)
    wd = w0 * np.exp(-np.square(s) / (2 * sig2))
    w = np.where(gt != 0, 1.0, np.float64(wc_bg) + wd)
    return w.astype(np.float32), n


def weighted_map_batch(gt_batch, w0=20, sig2=25):
    out = [weighted_map(g, w0, sig2) for g in np.asarray(gt_batch)]
    return np.stack([w for w, _ in out]), np.array([n for _, n in out])


def golden_cases(golden_dir):
    """(name, labels [B,n,n] in the dtype the reference was given, reference weights) of weighted_map_golden.npz."""
    g = np.load(os.path.join(golden_dir, "weighted_map_golden.npz"))
    for name in g["names"]:
        shape = tuple(int(v) for v in g[name + "_shape"])
        lab = np.unpackbits(g[name + "_bits"])[:int(np.prod(shape))].reshape(shape)
        dt = np.int64 if str(g[name + "_dtype"]) == "int64" else np.float32
        yield str(name), lab.astype(dt), g[name + "_w"]


def reach_of(sig2):
    """The device op's reach (wmap.hip's header): R = ceil(sqrt(2 sig2 * 104)); beyond it exp(-s^2 / (2 sig2)) < e^-104 < 2^-150."""
    return int(math.ceil(math.sqrt(2.0 * float(np.float32(sig2)) * 104.0)))


def check_against_restatement(lab, w, n_objects, w0=20, sig2=25, reach=REACH, counts=None):
    """lab numpy [B,H,W]; w, n_objects (and counts, the foreground pixels per image): the device op's results.  Counts exact,
    cells exactly 1, background with no component within `reach` exactly w_c, elsewhere |dw| <= 1e-5 max(1, |w_ref|).
    The restatement is exact for any reach on images of up to REACH + 1 = 74 pixels a side (every grown box is the image)."""
    w_ref, n_ref = weighted_map_batch(lab, w0, sig2)
    assert np.array_equal(n_objects, n_ref)
    if counts is not None:
        assert np.array_equal(counts, (lab != 0).reshape(lab.shape[0], -1).sum(axis=1))
    for b in range(lab.shape[0]):
        fg = lab[b] != 0
        assert np.all(w[b][fg] == 1.0)
        d1, _, _ = distances(lab[b])
        far = ~fg & (d1 > reach)
        if far.any():
            n1 = np.float32(fg.sum()); wc = n1 / np.float32(fg.size - fg.sum())
            if not np.issubdtype(lab.dtype, np.floating):
                wc = np.float32(np.trunc(wc))
            assert np.all(w[b][far] == wc)
    assert np.all(np.abs(w - w_ref) <= 1e-5 * np.maximum(1.0, np.abs(w_ref)))


def visible_border(lab, w_ref):
    """[B,H,W] bool: background pixels of images whose class term is exactly 0 (integer labels, fewer cells than background)
    where the reference's weight, there the border term alone, is at least 2^-100."""
    lab = np.asarray(lab)
    out = np.zeros(lab.shape, bool)
    if np.issubdtype(lab.dtype, np.floating):
        return out
    for b in range(lab.shape[0]):
        fg = lab[b] != 0
        if fg.sum() < fg.size - fg.sum():
            out[b] = ~fg & (w_ref[b] >= 2.0 ** -100)
    return out


# ---- seeded label batches of tests/test_weighted_map_ops_gpu.py (proved well-posed by tests/test_weighted_map_cpu.py) ------
# (B, H, W) at the default parameters: the smallest image; one past the 32-pixel labelling tile and the 64-wide column block;
# one past the 256 pixels of a row block; exact multiples of all three
THRESHOLD_SHAPES = [(1, 1, 2), (2, 33, 65), (1, 5, 257), (3, 64, 32), (2, 31, 256)]
# (w0, sig2) -> reach; 1020 is the longest the op admits (at most 1024)
PARAMS = [(20, 2), (10, 25), (3, 200), (20, 5000)]
REACHES = [21, 73, 204, 1020]
PARAM_CASES = ["blobs+far", "speckle+single", "tall-single", "tall-speckle"]


def param_dtype(name, w0, sig2):
    """int64 and float32 labels alternate over the cases and the parameters."""
    return (np.int64, np.float32)[(PARAM_CASES.index(name) + PARAMS.index((w0, sig2))) % 2]


def blobs(rs, H, W, count):
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), bool)
    for _ in range(count):
        cy, cx, r = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(0.5, max(1.0, min(H, W) / 6))
        lab |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return lab


def both_classes(lab, rs):
    if lab.all():
        lab.flat[rs.randint(lab.size)] = False
    if not lab.any():
        lab.flat[rs.randint(lab.size)] = True
    return lab


def threshold_labels(B, H, W, dtype):
    """Image b is speckle for odd b and discs for even b; every image has both classes."""
    rs = np.random.RandomState(H * 1000 + W)
    out = np.zeros((B, H, W), bool)
    for b in range(B):
        out[b] = both_classes(rs.rand(H, W) < 0.3 if b % 2 else blobs(rs, H, W, 6), rs)
    return out.astype(dtype)


def param_labels(name, dtype):
    """Images of at most 74 x 74.  'blobs+far' [2,40,70]: discs; two components 50 px and more apart (beyond the reach of 21
    at sig2 = 2).  'speckle+single' [2,40,70]: speckle; exactly one component.  'tall-single', 'tall-speckle' [1,74,9]."""
    rs = np.random.RandomState(PARAM_CASES.index(name) + 77)
    if name == "blobs+far":
        far = np.zeros((40, 70), bool)
        far[4:8, 3:9] = True
        far[30:37, 59:66] = True
        lab = np.stack([both_classes(blobs(rs, 40, 70, 8), rs), far])
    elif name == "speckle+single":
        one = np.zeros((40, 70), bool)
        one[10:19, 20:41] = True
        one[19:30, 28:31] = True
        lab = np.stack([rs.rand(40, 70) < 0.3, one])
    elif name == "tall-single":
        one = np.zeros((74, 9), bool)
        one[50:60, 2:7] = True
        lab = one[None]
    else:
        lab = (rs.rand(1, 74, 9) < 0.25)
    return lab.astype(dtype)
