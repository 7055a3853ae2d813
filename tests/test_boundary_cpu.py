"""Boundary scores without a GPU: the C ABI and the Python surface are there; tests/boundary_ref.py (what the GPU tests compare the
device with) agrees with scipy.ndimage (binary_erosion for the contour, distance_transform_edt for d2) and numpy.percentile on
random masks and gives the answers worked by hand below; functions.scores_from_surface, which is pure numpy, forms the scores of
hand-made records, empty contours included."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy import ndimage

import boundary_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_mask_boundary", "unet_surface_sums_scratch_bytes", "unet_surface_sums")
STRUCTURES = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}


def masks():
    """Some 60 random masks up to 24 x 24 in pairs, and the named cases"""
    rs = np.random.RandomState(11)
    out = []
    for k in range(30):
        H, W = rs.randint(1, 25, 2)
        a = rs.rand(H, W) < rs.uniform(0.1, 0.9)
        out.append(("random %d" % k, a.astype(np.uint8), (a ^ (rs.rand(H, W) < 0.2)).astype(np.uint8)))
    return out + [c for c in ref.named_cases() if c[1].size <= 2000]


def sums_of(s):
    """boundary_ref.surface's result as a functions.SurfaceSums of arrays"""
    import functions
    rec = np.zeros((2, 10), np.int64)
    for d in range(2):
        rec[d, :9] = s["record"][d][:9]
        rec[d, 9:] = np.array([s["record"][d][9]], np.float64).view(np.int64)
    return functions.SurfaceSums(rec, None, None, tuple(s["t2"]), *s["q"])


# ---- ABI and Python surface -------------------------------------------------------------------------------------------------

def test_abi_declares_and_exports_the_new_entry_points():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and name in _hip._SIGS and hasattr(L, name), name
    assert L.unet_abi_version() == 4
    assert len(_hip._SIGS["unet_mask_boundary"][1]) == 10 and len(_hip._SIGS["unet_surface_sums"][1]) == 20
    assert len(_hip._SIGS["unet_surface_sums_scratch_bytes"][1]) == 3
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1, -3, 4), (0, 0, 0)):
        assert L.unet_surface_sums_scratch_bytes(*dims) == 0
    for B, H, W in ((1, 1, 1), (3, 5, 7), (2, 300, 257)):
        assert L.unet_surface_sums_scratch_bytes(B, H, W) >= B * H * W * 17         # a byte of contour bits and four int32 planes


def test_python_surface():
    import functions
    a, b = torch.ones(4, 4, dtype=torch.uint8), torch.ones(4, 4, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="mask_boundary"):
        functions.mask_boundary(a)
    with pytest.raises(NotImplementedError, match="mask_boundary"):
        functions.mask_boundary(a.numpy())
    for fn, name in ((functions.surface_sums, "surface_sums"), (functions.boundary_scores, "surface_sums")):
        with pytest.raises(NotImplementedError, match=name):
            fn(a, b)
        with pytest.raises(NotImplementedError, match=name):
            fn(a[None].float(), b[None].long())
        with pytest.raises(ValueError, match="shape"):
            fn(a, torch.ones(4, 5, dtype=torch.uint8))
        with pytest.raises(ValueError, match="shape"):
            fn(a, a[None])
        with pytest.raises(ValueError, match=r"\[H,W\]"):
            fn(a[0], a[0])
        with pytest.raises(ValueError, match=r"\[H,W\]"):
            fn(a[None, None], a[None, None])
        with pytest.raises(ValueError, match="real dtype"):
            fn(a.to(torch.complex64), a)
        with pytest.raises(ValueError, match="at most 4"):
            fn(a, b, tolerances=(1, 2, 3, 4, 5))
        for t in (-1, -0.5, math.inf, math.nan, "1", None, True):
            with pytest.raises(ValueError, match="tolerance"):
                fn(a, b, tolerances=(1.0, t))
        for p in (-1, 100.5, math.nan, math.inf, "95", None, True):
            with pytest.raises(ValueError, match="percentile"):
                fn(a, b, percentile=p)
        for c in (0, 6, 4.5, True, "4"):
            with pytest.raises(ValueError, match="connectivity"):
                fn(a, b, connectivity=c)
        for e in ("edge", 0, None):
            with pytest.raises(ValueError, match="edge"):
                fn(a, b, edge=e)
        for k in (-1, 1.0, True, 1 << 31):
            with pytest.raises(ValueError, match="select"):
                fn(a, b, select=k)
        big = torch.ones(1, 1, dtype=torch.uint8).expand(functions.SHAPE_EDGE + 1, 1)
        with pytest.raises(ValueError, match="at most %d" % functions.SHAPE_EDGE):
            fn(big, big)
        with pytest.raises(ValueError, match="at most %d" % functions.SHAPE_EDGE):
            fn(big.T, big.T)
    for s in (0, -1.0, math.inf, math.nan, True, "1"):
        with pytest.raises(ValueError, match="spacing"):
            functions.boundary_scores(a, b, spacing=s)
        with pytest.raises(ValueError, match="spacing"):
            functions.scores_from_surface(functions.SurfaceSums(np.zeros((2, 10), np.int64), None, None, (), 19, 20), spacing=s)
    with pytest.raises(ValueError, match="connectivity"):
        functions.mask_boundary(a, connectivity=6)
    with pytest.raises(ValueError, match="edge"):
        functions.mask_boundary(a, edge="both")
    with pytest.raises(ValueError, match="select"):
        functions.mask_boundary(a, select=-2)
    with pytest.raises(ValueError, match=r"\[H,W\]"):
        functions.mask_boundary(a[0])
    with pytest.raises(ValueError, match="record"):
        functions.scores_from_surface(functions.SurfaceSums(np.zeros((2, 9), np.int64), None, None, (), 19, 20))
    assert functions.SurfaceSums._fields == ("record", "d2_pred", "d2_gt", "t2", "q_num", "q_den")
    assert functions.BoundaryScores._fields == ("hausdorff", "hd_percentile", "assd", "nsd", "precision", "recall", "boundary_f1", "n_pred", "n_gt")


def test_percentile_and_tolerance_fractions():
    import functions
    f = functions._percentile_fraction
    assert f("t", 95) == (19, 20) and f("t", 95.0) == (19, 20) and f("t", 0) == (0, 1) and f("t", 100) == (1, 1) and f("t", 50) == (1, 2)
    assert f("t", Fraction(300, 7)) == (3, 7) and f("t", 99.9) == (999, 1000) and f("t", 12.5) == (1, 8)
    num, den = f("t", 100 / 3)                                                     # no short decimal form: the nearest fraction
    assert den < functions.SURFACE_Q_DEN and abs(Fraction(num, den) - Fraction(1, 3)) < Fraction(1, 10 ** 9)
    assert ref.fraction_of(95) == (19, 20) and ref.fraction_of(Fraction(300, 7)) == (3, 7)
    assert ref.t2_of((1.0, 1.5, 2, math.sqrt(2), Fraction(7, 2), 0)) == [1, 2, 4, 2, 12, 0]      # sqrt(2) as a double is above the root


# ---- boundary_ref against scipy and numpy -----------------------------------------------------------------------------------

def test_contour_is_mask_minus_its_erosion():
    n = 0
    for name, p, g in masks():
        for m in (p, g):
            for conn, structure in STRUCTURES.items():
                reg = m != 0
                want = reg & ~ndimage.binary_erosion(reg, structure, border_value=0)
                assert np.array_equal(ref.contour(reg, conn, "background"), want), (name, conn)
                inner = reg & ~ndimage.binary_erosion(reg, structure, border_value=1)
                assert np.array_equal(ref.contour(reg, conn, "ignore"), inner), (name, conn, "ignore")
                n += 1
    assert n >= 180
    lab = np.array([[0, 2, 2, 2], [1, 2, 2, 2], [1, 2, 2, 2]])
    assert np.array_equal(ref.contour(ref.region(lab, 2), 4, "ignore"), [[0, 1, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]])
    assert np.array_equal(ref.contour(ref.region(lab, 1)), [[0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]])


def test_d2_and_percentile_against_scipy_and_numpy():
    n = 0
    for name, p, g in masks():
        for conn in (4, 8):
            for pct in (0, 50, 95, 100, Fraction(300, 7)):
                s = ref.surface(p, g, (1.0, 2.5), pct, None, conn, "background")
                cp, cg = (s["bits"] & 1).astype(bool), (s["bits"] & 2).astype(bool)
                for (ca, cb), rec, plane in zip(((cp, cg), (cg, cp)), s["record"], s["d2"]):
                    assert rec[0] == ca.sum()
                    if not ca.any() or not cb.any():
                        assert rec[1:] == [0] * 8 + [0.0] and (plane == -1).all()
                        continue
                    edt = ndimage.distance_transform_edt(~cb)
                    assert np.array_equal(plane[ca], np.round(edt[ca] ** 2).astype(np.int64)) and (plane[~ca] == -1).all(), (name, conn)
                    d = np.sqrt(plane[ca].astype(np.float64))
                    want = np.percentile(d, float(100 * Fraction(*s["q"])), method="linear")
                    assert abs(ref.directed_percentile(rec, s["q"][1]) - want) <= 1e-12 * max(1.0, want), (name, conn, pct)
                    assert rec[1] == plane.max() and rec[5:9] == [(plane[ca] <= 1).sum(), (plane[ca] <= 6).sum(), 0, 0]
                    assert abs(rec[9] - d.sum()) <= 1e-12 * rec[9]
                    n += 1
    assert n >= 400


# ---- boundary_ref against answers worked by hand ----------------------------------------------------------------------------

def test_identical_masks_and_single_pixels():
    a = ref.random_pair(9, 14)[0]
    s = ref.surface(a, a, (0, 1))
    n = int(ref.contour(a != 0).sum())
    assert s["record"][0] == s["record"][1] == [n, 0, 0, 0, (n - 1) * 19 % 20, n, n, 0, 0, 0.0]
    sc = ref.scores(s)
    assert (sc["hausdorff"], sc["hd_percentile"], sc["assd"]) == (0.0, 0.0, 0.0) and sc["nsd"] == sc["boundary_f1"] == [1.0, 1.0]
    for dy, dx in ((0, 0), (0, 3), (2, 0), (3, 4), (-2, 5)):
        p, g = ref.pixels(9, 12, (4, 3)), ref.pixels(9, 12, (4 + dy, 3 + dx))
        for edge in ("background", "ignore"):
            s = ref.surface(p, g, (4.9, 5.0), 95, None, 4, edge)
            d2 = dy * dy + dx * dx
            w = [int(d2 <= 24), int(d2 <= 25)]
            assert s["record"][0] == s["record"][1] == [1, d2, d2, d2, 0] + w + [0, 0, math.sqrt(d2)]
            sc = ref.scores(s, spacing=0.5)
            assert sc["hausdorff"] == sc["hd_percentile"] == sc["assd"] == math.sqrt(d2) * 0.5 and sc["nsd"] == [float(v) for v in w]


def test_square_shifted_by_two():
    """A 5 x 5 square has 16 contour pixels (the 3 x 3 inside is not contour) with either connectivity.  Against the square two
    columns to the right: the left column of the one (5 pixels) is 2 away from the other's left column; its top and bottom rows
    hold, beside the corner, x = 4 (1 away from the other's corner at x = 5) and x = 5, 6, 7 (on the other's row: 0); its right
    column at x = 7 is 2 away horizontally from column 9 and column 5, but its end pixels are on the other's top and bottom rows
    (0), and the three between are min(2, distance to the top row 1, 2, 1) = 1, 2, 1 away."""
    p, g = ref.square_case()
    for conn in (4, 8):
        s = ref.surface(p, g, (0, 1, 2), 50, None, conn)
        assert np.array_equal((s["bits"] & 1)[3:8, 3:8], [[1, 1, 1, 1, 1], [1, 0, 0, 0, 1], [1, 0, 0, 0, 1], [1, 0, 0, 0, 1], [1, 1, 1, 1, 1]])
        d = sorted([4] * 5 + [1] * 2 + [0] * 6 + [1, 4, 1])
        assert sorted(s["d2"][0][s["d2"][0] >= 0].tolist()) == d
        j, rem = divmod(15, 2)
        assert s["record"][0] == [16, 4, d[j], d[j + 1], rem, 6, 10, 16, 0, 6 * 2.0 + 4 * 1.0]
        assert s["record"][1] == s["record"][0]                                    # the mirror image
        sc = ref.scores(s)
        assert sc["hausdorff"] == 2.0 and sc["assd"] == 1.0 and sc["nsd"] == [6 / 16, 10 / 16, 1.0] and sc["hd_percentile"] == 1.0


def test_line_full_and_empty():
    name, p, g = [c for c in ref.named_cases() if c[0] == "line"][0]
    for conn in (4, 8):
        for edge in ("background", "ignore"):
            s = ref.surface(p, g, (1,), 100, None, conn, edge)
            assert np.array_equal(s["bits"] & 1, p) and np.array_equal(s["bits"] >> 1, g)      # one pixel wide: all of it is contour
            assert s["record"][0][:5] == [7, 1, 1, 1, 0] and s["record"][1][:5] == [9, 2, 2, 2, 0]
    full = np.ones((4, 6), np.uint8)
    s = ref.surface(full, full, (1,), 95, None, 4, "background")
    assert s["record"][0][0] == 16 and np.array_equal(s["bits"] & 1, [[1] * 6, [1, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 1], [1] * 6])
    s = ref.surface(full, full, (1,), 95, None, 8, "ignore")                       # nothing is outside: no contour
    assert s["record"] == [[0] * 9 + [0.0]] * 2 and not s["bits"].any()
    sc = ref.scores(s)
    assert (sc["hausdorff"], sc["hd_percentile"], sc["assd"], sc["nsd"], sc["boundary_f1"]) == (0.0, 0.0, 0.0, [1.0], [1.0])
    assert math.isnan(sc["precision"][0]) and math.isnan(sc["recall"][0])
    some = ref.random_pair(4, 6)[0]
    sc = ref.scores(ref.surface(np.zeros_like(some), some, (1, 2)))
    assert (sc["hausdorff"], sc["hd_percentile"], sc["assd"]) == (math.inf,) * 3 and sc["nsd"] == sc["boundary_f1"] == [0.0, 0.0]
    assert all(math.isnan(v) for v in sc["precision"]) and sc["recall"] == [0.0, 0.0] and sc["n_pred"] == 0 and sc["n_gt"] > 0


def test_strips_cross_radix_digits():
    for H in (1, 2):
        p, g = ref.strip_case(H)
        s = ref.surface(p, g, (), 50)
        assert s["record"][0][:5] == [4, 1449 ** 2, 25, 1030 ** 2, 1] and s["record"][1][:5] == [1, 4, 4, 4, 0]
        s = ref.surface(p, g, (), 95)
        assert s["record"][0][2:5] == [1030 ** 2, 1449 ** 2, 17] and (1030 ** 2) >> 20 == 1 and (1449 ** 2) >> 20 == 2
    p, g = ref.corners_case()
    assert ref.surface(p, g)["record"][0][1] == ref.surface(p, g)["record"][1][1] == 69 ** 2 + 299 ** 2


# ---- functions.scores_from_surface ------------------------------------------------------------------------------------------

def check_scores(got, want, k):
    for f in ("hausdorff", "hd_percentile", "assd"):
        assert getattr(got, f) == want[f] or abs(getattr(got, f) - want[f]) <= 1e-15 * want[f], f
    for f in ("nsd", "precision", "recall", "boundary_f1"):
        assert getattr(got, f).shape == (k,) and np.array_equal(getattr(got, f), np.array(want[f], np.float64), equal_nan=True), f
    assert got.n_pred == want["n_pred"] and got.n_gt == want["n_gt"]


def test_scores_from_surface_on_records():
    import functions
    n = 0
    for name, p, g in masks():
        for spacing in (1.0, 0.25):
            s = ref.surface(p, g, (1.0, 2.0, 3.5), 95)
            got = functions.scores_from_surface(sums_of(s), spacing=spacing)
            check_scores(got, ref.scores(s, spacing), 3)
            n += 1
    assert n >= 80
    p, g = ref.batch_case()                                                        # a batch: empty, full, ordinary
    each = [ref.surface(a, b, (1.0,), 50) for a, b in zip(p, g)]
    rec = np.stack([sums_of(s).record for s in each])
    got = functions.scores_from_surface(functions.SurfaceSums(torch.from_numpy(rec), None, None, (1,), 1, 2))
    assert got.hausdorff.shape == (3,) and got.nsd.shape == (3, 1) and got.n_pred.tolist() == [0, each[1]["record"][0][0], each[2]["record"][0][0]]
    for b in range(3):
        check_scores(functions.BoundaryScores(*(t[b] for t in got)), ref.scores(each[b]), 1)
    assert got.hausdorff[0] == math.inf and got.hausdorff[1] == 0.0 and 0 < got.hausdorff[2] < math.inf
    none = functions.scores_from_surface(functions.SurfaceSums(np.zeros((2, 10), np.int64), None, None, (), 19, 20))      # no tolerance
    assert none.nsd.shape == (0,) and none.hausdorff == 0.0 and none.n_pred == 0
