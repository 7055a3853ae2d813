"""Generates tests/golden/weighted_map_golden.npz by running the REFERENCE's own weighted_map (functions.py:7-78).

    python tests/golden/make_golden_weighted_map.py <path to a checkout of the reference>

OpenCV is not installed, so the reference's `import cv2 as cv` is served by a small stand-in module with the two calls
weighted_map makes, written on scipy:
  - cv.connectedComponents(img, connectivity=4) labels the 4-connected components of the non-zero pixels 1..n, the
    background 0, and returns (n + 1, labels).  scipy.ndimage.label(img != 0, structure=<4-neighbour cross>) forms the
    same partition (numbered in the same raster order, which weighted_map does not depend on: it sorts the maps).
  - cv.distanceTransform(src, cv.DIST_L2, maskSize=0) is the exact Euclidean distance (maskSize 0 = DIST_MASK_PRECISE)
    of every pixel to the nearest zero pixel of src, as float32.  scipy.ndimage.distance_transform_edt(src != 0) is the
    exact Euclidean distance to the nearest zero element; cast to float32 it is the same number (sqrt of an integer).
Nothing of the reference is stored: the fixture holds the labels (bit-packed) and the reference's outputs."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import aux_ref  # noqa: E402

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)


def cv2_stand_in():
    cv = types.ModuleType("cv2")
    cv.DIST_L2 = 2

    def connectedComponents(img, connectivity=8):
        lab, n = ndimage.label(np.asarray(img) != 0, structure=CROSS if connectivity == 4 else np.ones((3, 3), bool))
        return n + 1, lab.astype(np.int32)

    def distanceTransform(src, distanceType, maskSize=3):
        assert distanceType == cv.DIST_L2 and maskSize == 0
        return ndimage.distance_transform_edt(np.asarray(src) != 0).astype(np.float32)

    cv.connectedComponents = connectedComponents
    cv.distanceTransform = distanceTransform
    return cv


def reference_weighted_map(ref_dir):
    sys.modules["cv2"] = cv2_stand_in()
    spec = importlib.util.spec_from_file_location("reference_functions", os.path.join(ref_dir, "functions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.weighted_map


def disc(n, cy, cx, r):
    yy, xx = np.mgrid[0:n, 0:n]
    return (yy - cy) ** 2 + (xx - cx) ** 2 < r * r


def cases():
    """name -> {0,1} uint8 labels [B,n,n] (the reference needs square images) and the dtype they are handed over in."""
    c = {}
    cells = np.stack([aux_ref.cells(s, 256)[1] // 255 for s in (3, 4)])
    c["cells_i64"] = (cells, "int64")
    c["cells_f32"] = (cells, "float32")
    c["single"] = (disc(64, 30, 34, 11)[None], "int64")
    diag = np.zeros((48, 48), np.uint8)
    i = np.arange(48)
    diag[i, i] = 1                                  # 48 components under 4-connectivity
    diag[i[:40], 47 - i[:40]] = 1                   # the anti-diagonal meets it in one 2x2 block at the centre
    c["diagonal"] = (diag[None], "int64")
    ring = (disc(80, 40, 40, 25) & ~disc(80, 40, 40, 15)).astype(np.uint8)
    ring[70:76, 5:12] = 1
    c["ring"] = (ring[None], "float32")
    edge = np.zeros((64, 64), np.uint8)
    edge[0:5, 10:30] = 1; edge[20:40, 0:3] = 1; edge[60:64, 40:64] = 1; edge[0:64, 62:64] = 1; edge[30:34, 30:34] = 1
    edge[7:11, 12:20] = 1; edge[24:30, 5:9] = 1     # 2-3 px from the edge objects: strong border weights between them
    c["edge"] = (edge[None], "int64")
    far = np.zeros((200, 200), np.uint8)
    far[10:16, 10:16] = 1; far[180:190, 170:190] = 1
    c["far"] = (far[None], "int64")
    rs = np.random.RandomState(7)
    c["speckle96"] = ((rs.rand(1, 96, 96) < 0.35).astype(np.uint8), "int64")
    blobs = np.stack([disc(64, *rs.randint(8, 56, 2), rs.randint(4, 12)) | disc(64, *rs.randint(8, 56, 2), rs.randint(4, 12))
                      | (rs.rand(64, 64) < 0.02) for _ in range(3)]).astype(np.uint8)
    c["batch3"] = (blobs, "int64")
    return c


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    weighted_map = reference_weighted_map(sys.argv[1])
    out = {}
    for name, (lab, dt) in cases().items():
        t = torch.from_numpy(lab.astype(np.int64 if dt == "int64" else np.float32))
        w = weighted_map(t).numpy().astype(np.float32)
        out[name + "_shape"] = np.array(lab.shape)
        out[name + "_bits"] = np.packbits(lab.reshape(-1))
        out[name + "_dtype"] = np.array(dt)
        out[name + "_w"] = w
        print("%-10s %-16s %-7s w in [%.4g, %.4g]" % (name, lab.shape, dt, w.min(), w.max()))
    path = os.path.join(HERE, "weighted_map_golden.npz")
    np.savez_compressed(path, names=np.array(list(cases().keys())), **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
