"""Per-cell convex hulls and neighbours without a GPU: the C ABI and the Python surface are there; tests/hull_ref.py (what the
GPU tests compare the device with) gives the answers worked by hand below and those of scipy.spatial.ConvexHull; the tie rule
of the width and an input on which a 64-bit comparison picks another edge are pinned; functions.hull_props and
functions.neighbour_counts, which are pure numpy, give the closed forms."""
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy.spatial import ConvexHull

import hull_ref as ref
import instances_ref
import measure_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_cell_hulls_scratch_bytes", "unet_cell_hulls", "unet_cell_contacts_scratch_bytes", "unet_cell_contacts")


def one(mask):
    """(vertices, area2, feret_max2, (c, l2)) of a single cell given as a mask"""
    v = ref.hull(ref.corners(mask))
    return (v,) + ref.measure(v)


def tables(labels, n_max=None):
    """hull_ref.hulls and measure_ref.sums as functions.CellHulls and functions.CellSums"""
    import functions
    h = ref.hulls(labels, n_max)
    hulls = functions.CellHulls(h["n_vertices"], h["area2"], h["feret_max2"], h["width"][..., 0], h["width"][..., 1], h["offset"], h["vertices"])
    return hulls, functions.CellSums(**measure_ref.sums(labels, None, n_max))


def cases():
    """Every single-cell mask of this file, named"""
    rs = np.random.RandomState(3)
    out = [("pixel", np.ones((1, 1), bool)), ("disc", ref.disc()), ("disc pair", ref.disc_pair() > 0), ("strip", ref.strip_case() > 0)]
    out += [("rect %dx%d" % hw, np.ones(hw, bool)) for hw in ((1, 7), (7, 1), (3, 5), (6, 6), (40, 9))]
    out += [("random %d" % k, rs.rand(rs.randint(1, 24), rs.randint(1, 24)) < rs.uniform(0.05, 0.95)) for k in range(60)]
    out += [("cell %d" % k, instances_ref.cells_case(k, 1, 40, 44)[0] > 0) for k in range(5)]
    return [(n, m) for n, m in out if m.any()]


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
    assert len(_hip._SIGS["unet_cell_hulls"][1]) == 17 and len(_hip._SIGS["unet_cell_contacts"][1]) == 13
    for levels in (0, -1, -(1 << 40)):
        assert L.unet_cell_hulls_scratch_bytes(levels) == 0
    for levels in (1, 2, 1000, 1 << 33):
        assert L.unet_cell_hulls_scratch_bytes(levels) >= 8 * levels               # two 32-bit tables
    assert L.unet_cell_contacts_scratch_bytes(0, 64) == 0 and L.unet_cell_contacts_scratch_bytes(2, 0) == 0
    assert L.unet_cell_contacts_scratch_bytes(2, 64) >= 64 * 12                    # a 64-bit key and a 32-bit counter per slot


def test_python_surface():
    import functions
    lab = torch.ones(4, 4, dtype=torch.int32)
    for fn in (functions.cell_hulls, functions.cell_neighbours):
        with pytest.raises(NotImplementedError, match="device"):
            fn(lab)
        with pytest.raises(NotImplementedError, match="device"):
            fn(lab[None].long())
        with pytest.raises(ValueError, match="int32 or int64"):
            fn(lab.float())
        with pytest.raises(ValueError, match="int32 or int64"):
            fn(lab.bool())
        with pytest.raises(ValueError, match="shape"):
            fn(torch.ones(4, dtype=torch.int32))
        with pytest.raises(ValueError, match="shape"):
            fn(torch.ones(1, 1, 4, 4, dtype=torch.int32))
    assert functions.CellHulls._fields == ("n_vertices", "area2", "feret_max2", "width_cross", "width_len2", "offset", "vertices")
    assert functions.HullProps._fields == ("convex_area", "solidity", "feret_max", "feret_min", "convex_perimeter", "n_vertices")
    assert functions.Neighbours._fields == ("b", "i", "j", "sides")
    assert functions.CellSums._fields == measure_ref.FIELDS                        # unchanged


# ---- hull_ref against hand-worked answers -----------------------------------------------------------------------------------

def test_single_pixel_and_rectangles():
    v, a2, f2, w = one(np.ones((1, 1), bool))
    assert v == [(0, 0), (0, 1), (1, 1), (1, 0)] and (a2, f2, w) == (2, 2, (1, 1))
    for h, wd in ((1, 2), (2, 1), (3, 5), (5, 3), (4, 4), (1, 65), (17, 5)):
        m = np.zeros((h + 2, wd + 3), bool)
        m[1:1 + h, 2:2 + wd] = True
        v, a2, f2, (c, l2) = one(m)
        assert v == [(2, 1), (2, 1 + h), (2 + wd, 1 + h), (2 + wd, 1)]
        assert a2 == 2 * h * wd and f2 == h * h + wd * wd                          # solidity exactly 1
        assert c * c == min(h, wd) ** 2 * l2 and l2 == max(h, wd) ** 2             # the calliper lies on a long side
        if h == wd:
            assert (c, l2) == (h * h, h * h)


def test_l_shape_and_staircase():
    """X . .      the hull cuts the corner off along (1,0)-(3,2): area 9 - 2 = 7; the cut edge has l2 = 8 and the far vertex
       X . .      (0,3) at cross 8, so width^2 = 64 / 8 = 8 < 9 = the square of every axis-parallel width.
       X X X"""
    m = np.array([[1, 0, 0], [1, 0, 0], [1, 1, 1]], bool)
    v, a2, f2, w = one(m)
    assert v == [(0, 0), (0, 3), (3, 3), (3, 2), (1, 0)] and (a2, f2, w) == (14, 18, (8, 8))
    """X . .      a hexagon: the 3 x 3 square less two right triangles of legs 2: area 5; the two diagonal edges have l2 = 8 and
       . X .      the far vertices at cross 4: width^2 = 2 (sqrt 2 across the diagonal), the same (c, l2) for both.
       . . X"""
    v, a2, f2, w = one(np.eye(3, dtype=bool))
    assert v == [(0, 0), (0, 1), (2, 3), (3, 3), (3, 2), (1, 0)] and (a2, f2, w) == (10, 18, (4, 8))
    v, a2, f2, w = one(np.eye(3, dtype=bool)[::-1])                                # the other diagonal
    assert v == [(2, 0), (0, 2), (0, 3), (1, 3), (3, 1), (3, 0)] and (a2, f2, w) == (10, 18, (4, 8))


def test_discs():
    """The two figures of solidity the op is for: one disc of r = 12 is convex up to its staircase, two of them 22 apart under one
    id are not."""
    d = ref.disc(12)
    v, a2, f2, w = one(d)
    assert d.sum() == 441 and a2 == 946 and len(v) == 24 and f2 == 25 * 25 + 1
    p = ref.disc_pair(12, 22)
    v, a2, f2, w = one(p > 0)
    assert (p > 0).sum() == 871 and a2 == 2046 and f2 == 47 * 47 + 1
    assert round(2 * 441 / 946, 3) == 0.932 and round(2 * 871 / 2046, 3) == 0.851
    h = ref.hulls(p, n_max=3)                                                      # rows 0, 2 and 3 are absent
    assert h["n_vertices"].tolist() == [0, len(v), 0, 0] and h["area2"].tolist() == [0, 2046, 0, 0]
    assert h["offset"].tolist() == [0, 0, 26, 26, 26] and h["vertices"].shape == (52, 2)
    assert [tuple(x) for x in h["vertices"][:len(v)].tolist()] == v and not h["vertices"][len(v):].any()
    assert v[0] == (min(x for x, y in v if y == 1), 1) and v[-1] == (max(x for x, y in v if y == 1), 1)


def test_against_scipy():
    n = 0
    for name, m in cases():
        pts = np.array(ref.corners(m))
        v, a2, f2, w = one(m)
        sp = ConvexHull(pts)
        assert len(sp.vertices) == len(v) and set(map(tuple, pts[sp.vertices].tolist())) == set(v), name
        assert abs(sp.volume - a2 / 2) <= 1e-9 * a2, name                          # scipy's "volume" of a 2-d hull is its area
        d = pts[sp.vertices]
        assert f2 == int(((d[:, None, :] - d[None, :, :]) ** 2).sum(-1).max()), name
        n += 1
    assert n >= 60


# ---- the width: ties and 128 bits -------------------------------------------------------------------------------------------

def test_width_tie_takes_the_shorter_edge():
    """A trapezoid of height 3: its parallel sides (length 2 above, 6 below) both have width 3 = c / sqrt(l2) with (c, l2) = (6, 4)
    and (18, 36); the rule takes the smaller l2, whichever of the two comes first around the hull."""
    m = np.array([[0, 0, 1, 1, 0, 0], [0, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1]], bool)
    for mask in (m, m[::-1]):
        v, a2, f2, w = one(mask)
        ws = ref.widths(v)
        assert (6, 4) in ws and (18, 36) in ws and min(c * c / l2 for c, l2 in ws) == 9.0
        assert w == (6, 4)
    assert ref.widths(one(m)[0]).index((18, 36)) < ref.widths(one(m)[0]).index((6, 4))      # met in both orders
    assert ref.widths(one(m[::-1])[0]).index((6, 4)) < ref.widths(one(m[::-1])[0]).index((18, 36))


def test_strip_needs_more_than_64_bits():
    """The strip's long edges have c^2 l2 above 2^64: with the products wrapped at 64 bits the comparison picks another edge, so a
    kernel that compared in 64 bits fails test_hull_gpu's strip case."""
    m = ref.strip_case()
    assert m.shape == (6, 30000) and (m > 0).sum() == 4
    v = ref.hull(ref.corners(m > 0))
    exact, wrapped = ref.measure(v)[2], ref.measure(v, ref.less_wrapped64)[2]
    assert exact != wrapped
    assert exact[0] ** 2 * wrapped[1] < wrapped[0] ** 2 * exact[1]                 # Python integers: the exact one is narrower
    assert max(c * c * l2 for c, l2 in ref.widths(v)) >= 1 << 64
    assert all(exact[0] ** 2 * l2 <= c * c * exact[1] for c, l2 in ref.widths(v))


# ---- invariants -------------------------------------------------------------------------------------------------------------

def test_solidity_is_at_most_one():
    for name, m in cases():
        v, a2, f2, (c, l2) = one(m)
        assert 2 * int(m.sum()) <= a2 and len(v) >= 4 and c > 0 and l2 > 0, name
        assert c * c <= f2 * l2, name                                              # the smallest width is no larger than the largest


def test_contacts_sum_to_the_contact_of_cell_sums():
    """For every id >= 1 the sides of the pairs that hold it add up to CellSums.contact of measure_ref."""
    maps = [measure_ref.hand_case(), ref.block_map(1, 37, 300), ref.block_map(2, 65, 63), ref.sparse_ids(17, 5), measure_ref.every_pixel_its_own(9, 7),
            instances_ref.cells_case(3, 9, 64, 64, stride=3)[0], np.zeros((4, 4), np.int32), np.full((3, 3), 2, np.int32)]
    total = 0
    for m in maps:
        b, i, j, n = ref.contacts(m)
        assert (i >= 1).all() and (i < j).all() and (n >= 1).all() and (b == 0).all()
        want = measure_ref.sums(m)["contact"]
        got = np.zeros_like(want)
        np.add.at(got, i, n)
        np.add.at(got, j, n)
        assert np.array_equal(got[1:], want[1:])
        total += int(n.sum())
    assert total > 500
    b, i, j, n = ref.contacts(measure_ref.hand_case())
    assert (b.tolist(), i.tolist(), j.tolist(), n.tolist()) == ([0], [2], [5], [2])
    two = ref.contacts(np.stack([np.zeros((3, 5), np.int32), measure_ref.hand_case()]))
    assert [a.tolist() for a in two] == [[1], [2], [5], [2]]                       # the image index is the first column


# ---- functions.hull_props and functions.neighbour_counts --------------------------------------------------------------------

def test_hull_props_closed_forms():
    import functions
    m = np.zeros((12, 20), np.int32)
    m[1:4, 2:7] = 1                                                                # 3 x 5 rectangle
    m[6, 9] = 3                                                                    # one pixel
    m[8:11, 12:15][np.eye(3, dtype=bool)] = 4                                      # the staircase
    m[5:8, 0:3][np.array([[1, 0, 0], [1, 0, 0], [1, 1, 1]], bool)] = 6             # the L
    hulls, sums = tables(m, n_max=7)
    p = functions.hull_props(hulls, sums)
    assert all(getattr(p, f).dtype == np.float64 and getattr(p, f).shape == (8,) for f in p._fields[:-1]) and p.n_vertices.dtype == np.int32
    assert p.n_vertices.tolist() == [0, 4, 0, 4, 6, 0, 5, 0]
    for f in p._fields[:-1]:
        assert np.isnan(getattr(p, f)[[0, 2, 5, 7]]).all() and np.isfinite(getattr(p, f)[[1, 3, 4, 6]]).all(), f
    assert p.convex_area[[1, 3, 4, 6]].tolist() == [15.0, 1.0, 5.0, 7.0]
    assert p.solidity[[1, 3, 4, 6]].tolist() == [1.0, 1.0, 3 / 5, 5 / 7]
    assert p.feret_max[[1, 3, 4, 6]].tolist() == [math.sqrt(34), math.sqrt(2), math.sqrt(18), math.sqrt(18)]
    assert p.feret_min[[1, 3, 4, 6]].tolist() == [3.0, 1.0, 4 / math.sqrt(8), 8 / math.sqrt(8)]
    want = [16.0, 4.0, 4 + 2 * math.sqrt(8), 8 + math.sqrt(8)]
    assert np.allclose(p.convex_perimeter[[1, 3, 4, 6]], want, rtol=1e-15, atol=0)
    both = np.stack([m, m[::-1].copy()])                                           # a batch: the second image upside down
    hb = ref.hulls(both, 7)
    sb = functions.CellSums(**measure_ref.sums_batch(both, None, 7))
    pb = functions.hull_props(functions.CellHulls(hb["n_vertices"], hb["area2"], hb["feret_max2"], hb["width"][..., 0], hb["width"][..., 1],
                                                  hb["offset"], hb["vertices"]), sb)
    assert pb.solidity.shape == (2, 8) and np.array_equal(pb.solidity[0], p.solidity, equal_nan=True)
    assert np.allclose(pb.convex_perimeter[1], p.convex_perimeter, rtol=1e-15, atol=0, equal_nan=True)
    assert np.array_equal(pb.feret_min[1], p.feret_min, equal_nan=True)


def test_hull_props_on_random_cells_and_torch_tables():
    import functions
    m = ref.block_map(7, 37, 60)
    hulls, sums = tables(m, n_max=int(m.max()) + 2)
    p = functions.hull_props(hulls, sums)
    on = hulls.n_vertices > 0
    assert on.sum() >= 10 and not on[0] and np.array_equal(on[1:], sums.present[1:])
    assert (p.solidity[on] <= 1.0).all() and (p.solidity[on] > 0).all() and (p.feret_min[on] <= p.feret_max[on]).all()
    assert (p.convex_perimeter[on] >= 2 * p.feret_max[on]).all() and (p.convex_perimeter[on] <= math.pi * p.feret_max[on] + 1e-9).all()
    for i in np.nonzero(on)[0]:
        v = ref.hull(ref.corners(m == i))
        per = sum(math.hypot(v[k][0] - v[k - 1][0], v[k][1] - v[k - 1][1]) for k in range(len(v)))
        assert abs(p.convex_perimeter[i] - per) <= 1e-12 * per
    as_torch = functions.CellHulls(*(torch.from_numpy(np.ascontiguousarray(t)) for t in hulls))
    q = functions.hull_props(as_torch, functions.CellSums(*(None if t is None else torch.from_numpy(t) for t in sums)))
    for f in p._fields:
        assert np.array_equal(getattr(p, f), getattr(q, f), equal_nan=True), f


def test_neighbour_counts():
    import functions
    m = np.array([[1, 1, 2, 0, 7],
                  [3, 3, 2, 0, 7],
                  [3, 4, 4, 0, 0]], np.int32)
    nb = functions.Neighbours(*ref.contacts(np.stack([m, np.zeros_like(m)])))
    assert list(zip(nb.b.tolist(), nb.i.tolist(), nb.j.tolist(), nb.sides.tolist())) == [
        (0, 1, 2, 1), (0, 1, 3, 2), (0, 2, 3, 1), (0, 2, 4, 1), (0, 3, 4, 2)]
    c = functions.neighbour_counts(nb, 2, 8)
    assert c.dtype == np.int64 and c.shape == (2, 9) and c[0].tolist() == [0, 2, 3, 3, 2, 0, 0, 0, 0] and not c[1].any()
