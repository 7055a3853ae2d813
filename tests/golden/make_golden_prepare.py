"""Generates tests/golden/prepare_golden.npz by EXECUTING the reference's own preprocess_gt (data.py:195-221) and the
statements of ImageDataset that build and use the weighted crop distribution (data.py:63-82, :98-103, :115).

    python tests/golden/make_golden_prepare.py <path to a checkout of the reference>

data.py cannot be imported (it reads files with OpenCV and imports downloaders), so the function and the statements are taken
from the file's AST and executed in namespaces holding exactly the names they use:
  - preprocess_gt, the whole function;
  - from ImageDataset.__init__, the body of the loop over the target files after the file read: preprocess_gt, cv.threshold,
    the list of pairs and the loop over the windows that fills target_weighted_crop_distribution;
  - from ImageDataset.__getitem__, the statements from `crop_id = ...` to the clamping of y, and `rot_deg = ...`, with
    np.random seeded, so that the draws and the generator's state after them are reproducible.
OpenCV is not installed: `cv` is a stand-in with the three calls made, written on scipy:
  - cv.getStructuringElement(cv.MORPH_RECT, (5, 5)) is a 5 x 5 array of ones;
  - cv.dilate(src, kernel, iterations=k) is the maximum over the kernel's footprint, k times; OpenCV's default border for
    dilate contributes nothing to the maximum: scipy.ndimage.grey_dilation(mode='constant', cval=-inf);
  - cv.threshold(src, t, maxval, cv.THRESH_BINARY) returns (t, maxval where src > t else 0) in src's type.
Nothing of the reference is stored: the fixture holds the input id maps and the reference's numeric outputs."""
import ast
import os
import sys
import types

import numpy as np
from scipy import ndimage
from scipy.stats import norm

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import prepare_ref as ref  # noqa: E402


def cv2_stand_in():
    cv = types.ModuleType("cv2")
    cv.MORPH_RECT = 0
    cv.THRESH_BINARY = 0

    def getStructuringElement(shape, ksize):
        assert shape == cv.MORPH_RECT
        return np.ones((ksize[1], ksize[0]), np.uint8)

    def dilate(src, kernel, iterations=1):
        out = np.asarray(src)
        for _ in range(iterations):
            out = ndimage.grey_dilation(out, footprint=kernel.astype(bool), mode="constant", cval=-np.inf)
        return out

    def threshold(src, thresh, maxval, kind):
        assert kind == cv.THRESH_BINARY
        return thresh, np.where(src > thresh, maxval, 0).astype(src.dtype)

    cv.getStructuringElement, cv.dilate, cv.threshold = getStructuringElement, dilate, threshold
    return cv


def target_id(st):
    t = st.targets[0] if isinstance(st, ast.Assign) else None
    return getattr(t, "id", None)


def reference_code(ref_dir):
    tree = ast.parse(open(os.path.join(ref_dir, "data.py")).read())
    pre = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "preprocess_gt"][0]
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ImageDataset"][0]
    init = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__"][0]
    loop = [n for n in ast.walk(init) if isinstance(n, ast.For) and getattr(n.target, "id", "") == "filename"
            and "preprocess_gt" in ast.dump(n)][0]
    first = [i for i, st in enumerate(loop.body) if "preprocess_gt" in ast.dump(st)][0]
    get = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__getitem__"][0]
    lo = [i for i, st in enumerate(get.body) if target_id(st) == "crop_id"][0]
    hi = [i for i, st in enumerate(get.body) if target_id(st) == "y"][-1]
    rot = [st for st in get.body if target_id(st) == "rot_deg"]
    comp = lambda body, what: compile(ast.Module(body, []), "reference:data.py:" + what, "exec")
    return comp([pre], "preprocess_gt"), comp(loop.body[first:], "__init__"), comp(get.body[lo:hi + 1] + rot, "__getitem__")


CASES = [  # name, kind, seed, H, W, crops
    ("discs", "discs", 1, 96, 120, (36, 60)),
    ("discs_hi", "discs_hi", 2, 96, 120, (36, 60)),
    ("speckle", "speckle", 3, 40, 52, (36, 39)),
    ("edges", "edges", 4, 64, 64, (36, 60)),
    ("two_piece", "two_piece", 5, 41, 41, (36, 40)),
    ("zeros", "zeros", 6, 40, 52, (36, 39)),
]
DRAW_SEEDS = (0, 1, 2)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    pre_code, init_code, get_code = reference_code(sys.argv[1])
    cv = cv2_stand_in()
    fns = {"np": np, "cv": cv}
    exec(pre_code, fns)
    preprocess_gt = fns["preprocess_gt"]
    out = {"names": np.array([c[0] for c in CASES]), "draw_seeds": np.array(DRAW_SEEDS)}
    for name, kind, seed, H, W, crops in CASES:
        img = ref.ids_case(kind, seed, H, W).astype(np.uint16 if kind != "speckle" else np.int32)   # man_seg images are uint16
        gt, mask_global = preprocess_gt(img)
        out[name + "_ids"] = img
        out[name + "_gt"] = gt
        out[name + "_mask_global"] = mask_global
        out[name + "_crops"] = np.array(crops)
        for crop in crops:
            me = types.SimpleNamespace(pairs=None, crop=crop, skip=10, target=[], target_weighted_crop_distribution=[])
            ns = {"np": np, "cv": cv, "norm": norm, "preprocess_gt": preprocess_gt, "self": me, "crop": crop, "img": img}
            exec(init_code, ns)
            out["%s_bin" % name] = me.target[0]
            out["%s_pairs%d" % (name, crop)] = np.array(me.pairs)
            out["%s_p%d" % (name, crop)] = np.asarray(me.target_weighted_crop_distribution[0], np.float64)
            if name == "discs" and crop == crops[0]:
                for s in DRAW_SEEDS:
                    np.random.seed(s)
                    g = {"np": np, "self": me, "idx": 0, "target": me.target[0]}
                    exec(get_code, g)
                    st = np.random.get_state()
                    out["draw%d" % s] = np.array([g["x"], g["y"], g["rot_deg"]])
                    out["draw%d_keys" % s] = st[1]
                    out["draw%d_pos" % s] = np.array([st[2], st[3]])
                    out["draw%d_gauss" % s] = np.array(st[4])
                    print("seed", s, "->", g["x"], g["y"], g["rot_deg"])
        p = out["%s_p%d" % (name, crops[0])]
        print("%-10s %-9s gt max %5d, edges max %5d, p(crop %d): %d of %d windows non-zero" %
              (name, img.shape, gt.max(), mask_global.max(), crops[0], (p > 0).sum(), len(p)))
    out["meta"] = np.array(repr(dict(numpy=np.__version__, scipy=__import__("scipy").__version__)))
    path = os.path.join(HERE, "prepare_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
