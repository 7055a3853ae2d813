"""Per-cell measurements without a GPU: the C ABI and the Python surface are there; tests/measure_ref.py (what the GPU tests
compare the device with) gives the answers worked by hand below and those of scipy.ndimage; functions.props_from_sums, which is
pure numpy, gives the closed forms of rectangles, diagonals and single pixels and keeps its second moments within the rounding
of an independent float64 computation centred on the centroid."""
import os
import re

import numpy as np
import pytest
import torch

import instances_ref
import measure_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_cell_sums_scratch_bytes", "unet_cell_sums", "unet_remap_labels")


def table(labels, image=None, n_max=None):
    """measure_ref.sums as a functions.CellSums"""
    import functions
    return functions.CellSums(**ref.sums(labels, image, n_max))


def props(labels, image=None, n_max=None):
    import functions
    return functions.props_from_sums(table(labels, image, n_max))


def test_abi_declares_and_exports_the_new_entry_points():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(L, name), name
    assert L.unet_abi_version() == 4
    assert L.unet_cell_sums_scratch_bytes(2, 9) == 2 * 10 * 128         # one 128-byte record per (image, id)
    assert L.unet_cell_sums_scratch_bytes(0, 9) == 0 and L.unet_cell_sums_scratch_bytes(1, -1) == 0
    assert L.unet_cell_sums_scratch_bytes(1, 1 << 24) == 0


def test_python_surface():
    import functions
    import tester
    lab = torch.ones(4, 4, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="device"):
        functions.cell_sums(lab)
    with pytest.raises(NotImplementedError, match="device"):
        functions.cell_props(lab)
    with pytest.raises(NotImplementedError, match="device"):
        functions.select_cells(lab, torch.ones(2, dtype=torch.bool))
    with pytest.raises(ValueError, match="int32 or int64"):
        functions.cell_sums(lab.float())
    with pytest.raises(ValueError, match="shape"):
        functions.cell_sums(torch.ones(4, dtype=torch.int32))
    assert functions.CellSums._fields == ref.FIELDS
    assert "measure" in tester.segment.__code__.co_varnames


# ---- measure_ref against hand-worked answers and scipy ----------------------------------------------------------------------

def test_the_hand_worked_map():
    """[[2 2 0 0 0]
        [2 5 5 0 0]
        [0 0 0 0 0]]   id 2: (0,0) (0,1) (1,0), on the frame; id 5: (1,1) (1,2), inside; the two touch along two edges."""
    m = ref.hand_case()
    img = np.arange(15, dtype=np.int32).reshape(3, 5) * 100           # v = 100 (5 y + x)
    s = ref.sums(m, img, n_max=6)
    assert s["area"].tolist() == [10, 0, 3, 0, 0, 2, 0]
    assert s["present"].tolist() == [True, False, True, False, False, True, False]
    assert s["bbox"].tolist() == [[0, 0, 3, 5], [0] * 4, [0, 0, 2, 2], [0] * 4, [0] * 4, [1, 1, 2, 3], [0] * 4]
    #                      sum y, sum x, sum y^2, sum x^2, sum xy
    assert s["moments"][2].tolist() == [1, 1, 1, 1, 0]
    assert s["moments"][5].tolist() == [2, 3, 2, 5, 3]
    assert s["moments"][0].tolist() == [15 - 1 - 2, 30 - 1 - 3, 25 - 1 - 2, 90 - 1 - 5, 30 - 0 - 3]
    # id 2: frame sides: (0,0) top and left, (0,1) top, (1,0) left = 4; open: (0,1) right, (1,0) below = 2; contact with 5: (0,1)
    # below, (1,0) right = 2.  The perimeter of the L-shaped triomino is 8
    assert (s["frame"][2], s["open"][2], s["contact"][2]) == (4, 2, 2)
    # id 5: no frame; contact with 2: (1,1) above and left = 2; open: (1,1) below, (1,2) above, below, right = 4.  A domino has 6
    assert (s["frame"][5], s["open"][5], s["contact"][5]) == (0, 4, 2)
    # the background: frame sides top 3, bottom 5, right 3, left 1 = 12 (the 16 of the image minus the 4 of id 2); its contact is
    # every open edge of the cells seen from the other side; it has no open edge by definition
    assert (s["frame"][0], s["open"][0], s["contact"][0]) == (12, 0, 2 + 4)
    assert s["v_sum"].tolist() == [10500 - 600 - 1300, 0, 600, 0, 0, 1300, 0]
    assert s["v_sum2"][5] == 600 ** 2 + 700 ** 2 and s["v_sum2"][2] == 100 ** 2 + 500 ** 2
    assert (s["v_min"][2], s["v_max"][2], s["v_min"][5], s["v_max"][5], s["v_min"][0], s["v_max"][0]) == (0, 500, 600, 700, 200, 1400)
    assert s["v_min"][1] == 0 and s["v_max"][1] == 0
    # every edge of the image is counted: frame sides in all = 2 (H + W), and contact is symmetric
    assert s["frame"].sum() == 16 and s["open"].sum() == s["contact"][0]


@pytest.mark.parametrize("seed,H,W", [(0, 37, 53), (1, 64, 64), (2, 5, 17)])
def test_against_scipy(seed, H, W):
    gt, pred = instances_ref.cells_case(seed, 7, H, W, stride=3)
    n_max = int(gt.max()) + 2
    for img in (ref.int_image(seed, (H, W)), np.random.RandomState(seed).rand(H, W).astype(np.float32) * 255 - 20):
        s = ref.sums(gt, img, n_max)
        want = ref.scipy_route(gt, img, n_max)
        p = props(gt, img, n_max)
        for k in range(1, n_max + 1):
            assert s["area"][k] == want["area"][k - 1]
            if not s["present"][k]:
                assert want["bbox"][k - 1] is None and np.isnan(p.area[k]) and np.isnan(p.centroid[k]).all() and np.isnan(p.mean[k])
                continue
            sl = want["bbox"][k - 1]
            assert s["bbox"][k].tolist() == [sl[0].start, sl[1].start, sl[0].stop, sl[1].stop]
            assert s["v_min"][k] == want["v_min"][k - 1] and s["v_max"][k] == want["v_max"][k - 1]
            if img.dtype.kind == "i":
                assert s["v_sum"][k] == want["v_sum"][k - 1] and s["v_sum2"][k] == want["v_sum2"][k - 1]       # below 2^53: exact in scipy too
            else:
                sabs, ssq = ref.abs_sums(gt, img, n_max)
                assert abs(s["v_sum"][k] - want["v_sum"][k - 1]) <= s["area"][k] * 2.0 ** -52 * sabs[k]
                assert abs(s["v_sum2"][k] - want["v_sum2"][k - 1]) <= s["area"][k] * 2.0 ** -52 * ssq[k]
            assert np.allclose(p.centroid[k], want["centroid"][k - 1], rtol=0, atol=1e-9)
            assert abs(p.mean[k] - want["v_sum"][k - 1] / want["area"][k - 1]) <= 1e-9 * 255


def test_edges_are_symmetric_and_cover_the_frame():
    for H, W in ((5, 17), (64, 64), (37, 30)):
        gt, pred = instances_ref.cells_case(H, 9, H, W)
        for m in (gt, pred, np.zeros((H, W), np.int32), ref.every_pixel_its_own(H, W)):
            s = ref.sums(m)
            assert s["frame"].sum() == 2 * (H + W)
            assert s["open"][1:].sum() + s["contact"][1:].sum() - s["contact"][0] == 2 * count_inner_edges(m)
            assert (s["frame"] + s["open"] + s["contact"])[s["present"]].min() >= 4


def count_inner_edges(m):
    """edges between two different non-zero ids"""
    m = m.astype(np.int64)
    return int(((m[:, 1:] != m[:, :-1]) & (m[:, 1:] > 0) & (m[:, :-1] > 0)).sum() + ((m[1:] != m[:-1]) & (m[1:] > 0) & (m[:-1] > 0)).sum())


def test_select_ref():
    m = ref.hand_case()
    keep = np.array([True, True, False, True, True, True, True])
    assert np.array_equal(ref.select(m, keep), np.where(m == 5, 5, 0))
    assert np.array_equal(ref.select(m, keep, renumber=True), np.where(m == 5, 4, 0))           # 1, 3, 4, 5 kept: 5 is the fourth
    both = np.stack([keep, ~keep])
    got = ref.select(np.stack([m, m]), both, renumber=True)
    assert np.array_equal(got[0], np.where(m == 5, 4, 0)) and np.array_equal(got[1], np.where(m == 2, 1, 0))


# ---- props_from_sums against closed forms -----------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,y0,x0", [(3, 8, 0, 0), (8, 3, 5, 2), (1, 9, 4, 4), (6, 6, 1, 30000), (40, 7, 32000, 32700)])
def test_a_rectangle(h, w, y0, x0):
    """h x w point masses: variances (h^2 - 1) / 12 and (w^2 - 1) / 12, hence the axes; far from the origin too (by its table,
    written down in closed form: no image of that size is made)."""
    import functions
    ys, xs = np.arange(y0, y0 + h, dtype=object), np.arange(x0, x0 + w, dtype=object)
    mom = [w * ys.sum(), h * xs.sum(), w * (ys * ys).sum(), h * (xs * xs).sum(), ys.sum() * xs.sum()]
    z = np.zeros(2, np.int64)
    s = functions.CellSums(area=np.array([0, h * w]), bbox=np.array([[0] * 4, [y0, x0, y0 + h, x0 + w]], np.int32),
                           moments=np.array([[0] * 5, [int(v) for v in mom]], np.int64), frame=z, open=z + [0, 2 * (h + w)], contact=z,
                           v_sum=None, v_sum2=None, v_min=None, v_max=None, present=np.array([False, True]))
    p = functions.props_from_sums(s)
    vy, vx = (h * h - 1) / 12, (w * w - 1) / 12
    tol = 4 * h * w * 2.0 ** -52 * (h * h + w * w)
    assert abs(p.moments_central[1, 0] - vy) <= tol and abs(p.moments_central[1, 1] - vx) <= tol and abs(p.moments_central[1, 2]) <= tol
    assert np.isclose(p.axis_major[1], 4 * np.sqrt(max(vy, vx)), rtol=1e-12) and np.isclose(p.axis_minor[1], 4 * np.sqrt(min(vy, vx)), rtol=1e-12, atol=1e-12)
    assert np.allclose(p.centroid[1], [y0 + (h - 1) / 2, x0 + (w - 1) / 2], rtol=0, atol=1e-9)
    assert p.extent[1] == 1.0 and p.perimeter[1] == 2 * (h + w) and p.contact_fraction[1] == 0 and not p.touches_frame[1]
    assert np.isclose(p.equivalent_diameter[1], np.sqrt(4 * h * w / np.pi))
    if h != w:
        assert np.isclose(p.eccentricity[1], np.sqrt(1 - min(vy, vx) / max(vy, vx)), rtol=1e-12)
        assert np.isclose(p.orientation[1], np.pi / 2 if h > w else 0.0, atol=1e-12)            # tall: along y; wide: along x
    assert p.mean is None and p.std is None and p.min is None and p.max is None
    assert all(np.isnan(getattr(p, f)[0]).all() for f in p._fields if f not in ("bbox", "touches_frame", "mean", "std", "min", "max"))
    assert not p.touches_frame[0]


def test_diagonals_single_pixels_and_absent_ids():
    n = 9
    m = np.zeros((n + 2, n + 3), np.int32)
    for k in range(n):
        m[1 + k, 2 + k] = 1                                               # along y = x (down and to the right)
        m[1 + k, n + 1 - k] = m[1 + k, n + 1 - k] or 2                    # along y = -x; the crossing pixel stays id 1
    m[0, 0] = 4
    p = props(m, n_max=5)
    assert np.isclose(p.eccentricity[1], 1.0, atol=1e-7) and np.isclose(p.orientation[1], np.pi / 4, atol=1e-12)
    assert p.axis_minor[1] <= 1e-6 and np.isclose(p.axis_major[1], 4 * np.sqrt(2 * (n * n - 1) / 12))
    assert np.isclose(p.orientation[2], -np.pi / 4, atol=1e-12) and np.isclose(p.eccentricity[2], 1.0, atol=1e-7)     # a line with a gap
    assert p.axis_major[4] == 0 and p.axis_minor[4] == 0 and p.eccentricity[4] == 0 and p.area[4] == 1 and p.extent[4] == 1
    assert p.touches_frame[4] and not p.touches_frame[1] and p.perimeter[4] == 4 and p.equivalent_diameter[4] == np.sqrt(4 / np.pi)
    for k in (3, 5):
        assert all(np.isnan(getattr(p, f)[k]).all() for f in p._fields if f not in ("bbox", "touches_frame", "mean", "std", "min", "max"))
        assert not p.touches_frame[k] and p.bbox[k].tolist() == [0, 0, 0, 0]
    two = np.array([[1, 2, 2]], np.int32)                                 # two touching cells: contact on both sides
    q = props(two)
    assert q.contact_fraction[1] == 1 / 4 and q.contact_fraction[2] == 1 / 6 and q.touches_frame[1]


def test_intensity_properties():
    m = ref.hand_case()
    img = np.arange(15, dtype=np.int32).reshape(3, 5) * 100
    p = props(m, img, n_max=5)
    assert p.mean[5] == 650 and p.std[5] == 50 and p.min[5] == 600 and p.max[5] == 700
    assert p.mean[2] == 200 and np.isclose(p.std[2], np.std([0, 100, 500]))
    assert np.isnan(p.mean[1]) and np.isnan(p.std[3]) and np.isnan(p.min[4]) and np.isnan(p.max[4])
    f = props(m, img.astype(np.float32) / 8, n_max=5)
    assert f.mean[5] == 650 / 8 and np.isclose(f.std[5], 50 / 8) and f.min[5] == 75 and f.max[5] == 87.5
    big = np.full((3, 5), 65535, np.int32)                                # no cancellation in the integer variance
    assert props(m, big).std[0] == 0 and props(m, big).mean[2] == 65535


@pytest.mark.parametrize("offset", [0, 32000])
def test_second_moments_within_the_rounding_of_a_centred_sum(offset):
    """|mu / area - the float64 sum of (y - cy)^2 / area| <= 4 area 2^-52 (h^2 + w^2), h, w the box sides: both are sums of area
    non-negative terms of at most h^2 + w^2, each carrying at most area 2^-53 times their sum; the 4 allows for the division and
    the subtraction.  With the cells pushed to the far corner of the largest image the bound is the same: the table is
    re-centred in integers first.  (The far cells' tables are formed from the near ones' by the shift, exactly.)"""
    import functions
    gt, pred = instances_ref.cells_case(11, 12, 90, 120, stride=2)
    n_max = int(gt.max())
    s = ref.sums(gt, n_max=n_max)
    if offset:
        a, o = s["area"], offset
        sy, sx, syy, sxx, sxy = s["moments"].T
        s["moments"] = np.stack([sy + a * o, sx + a * o, syy + 2 * o * sy + a * o * o, sxx + 2 * o * sx + a * o * o,
                                 sxy + o * sx + o * sy + a * o * o], axis=1)
        s["bbox"] = np.where(s["present"][:, None], s["bbox"] + o, 0).astype(np.int32)
    p = functions.props_from_sums(functions.CellSums(**s))
    checked = 0
    for k in range(1, n_max + 1):
        ys, xs = np.nonzero(gt == k)
        if len(ys) == 0:
            continue
        ys, xs = ys.astype(np.float64), xs.astype(np.float64)
        cy, cx = ys.mean(), xs.mean()
        want = np.array([((ys - cy) ** 2).sum(), ((xs - cx) ** 2).sum(), ((ys - cy) * (xs - cx)).sum()]) / len(ys)
        h, w = ys.max() - ys.min() + 1, xs.max() - xs.min() + 1
        bound = 4 * len(ys) * 2.0 ** -52 * (h * h + w * w)
        delta = np.abs(p.moments_central[k] - want)
        assert (delta <= bound).all(), (k, delta, bound)
        assert np.allclose(p.centroid[k], [cy + offset, cx + offset], rtol=0, atol=1e-8)
        checked += 1
    assert checked >= 8
