"""Plain numpy/scipy restatement of the reference's weighted_map (functions.py:7-78), one image at a time, by the
reference's own method: label the 4-connected cells, one exact Euclidean distance transform per component, keep the
two least distances per pixel, w = w_c + w0 * exp(-(d1 + d2)^2 / (2 sig2)) on background in float64, stored as float32.

The one liberty taken: each component's distance transform is computed on its bounding box grown by REACH pixels, and
every pixel outside that box counts as infinitely far.  Such a pixel is more than REACH = 73 px from the component, so
(d1 + d2) > 73 there and 20 * exp(-(d1 + d2)^2 / 50) < 1e-44: it differs from the reference by less than the smallest
float32 subnormal.  It keeps speckle labels with thousands of components affordable on a CPU."""
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
