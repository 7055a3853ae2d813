"""The numpy restatement of the topology-preserving warp (tests/warp_ref.py), which tests/test_warp_gpu.py holds the device op to,
pinned on the CPU: the table of simple neighbourhoods against the component definition, the parallel passes against a raster-order
sequential warp, the invariants of the result, hand-worked cases, and that the inputs of the GPU tests exercise the code."""
import numpy as np
import pytest
from scipy import ndimage

import instances_ref
import warp_ref as ref

P_MAX, LAUNCHES = 16, 8                                      # the defaults of functions.warp_labels


def disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def all_cases():
    """(name, gt bool [H,W], pred bool [H,W]) of every kind the GPU tests use, at sizes the sequential form can afford."""
    out = []
    for H, W in ((3, 3), (5, 7), (33, 31), (63, 65)):
        for name, g, p in ref.size_cases(H, W):
            out += [("%s %dx%d[%d]" % (name, H, W, b), g[b] != 0, p[b] != 0) for b in range(len(g))]
    out.append(("corridor", *ref.corridor(9, 120)))
    out.append(("cells 128", *ref.cells_pair(1, 9, 128, 128)))
    return out


def test_the_table_of_simple_neighbourhoods():
    """116 of the 256 codes; complementing all 8 neighbours and swapping the two connectivities maps the table onto itself,
    which is why connectivity 8 needs no second table."""
    t = ref.simple_table()
    assert t.shape == (256,) and int(t.sum()) == 116
    swapped = np.array([ref.is_simple(c ^ 255, ref.FULL, ref.CROSS) for c in range(256)])
    assert np.array_equal(t, swapped)
    assert not t[0] and not t[255]                           # an isolated pixel and an interior pixel
    assert t[0b00000010] and not t[0b00100010]               # the end of a line; the middle of a vertical line
    assert not t[0b00000001]                                 # only a diagonal neighbour: no 4-neighbour in the component


@pytest.mark.parametrize("reach", (None, 2.5))
def test_parallel_passes_equal_the_sequential_warp(reach):
    for name, g, p in all_cases():
        may = ref.may_mask(g, reach)
        L, count, sweeps, _ = ref.warp(g, p, may)
        Ls, sweeps_s = ref.warp_sequential(g, p, may)
        assert np.array_equal(L, Ls) and sweeps == sweeps_s, name


@pytest.mark.parametrize("reach", ref.REACHES)
def test_invariants_of_the_warp(reach):
    """Topology kept, flips only inside may and at most once per pixel, and nothing left to do."""
    table = ref.simple_table()
    cases = all_cases() + [("cells 256", *ref.cells_pair(2, 37, 256, 256))]
    for name, g, p in cases:
        may = ref.may_mask(g, reach)
        L, count, sweeps, per_sweep = ref.warp(g, p, may)
        assert ref.components(L) == ref.components(g), name
        assert not ((L != g) & ~may).any(), name
        assert count.max(initial=0) <= 1 and np.array_equal(count > 0, L != g), name
        assert not (may & (L != p) & table[ref.codes(L)]).any(), name
        assert per_sweep[-1] == 0 and all(n > 0 for n in per_sweep[:-1]) and sum(per_sweep) == count.sum(), name
        assert sweeps <= int((may & (g != p)).sum()) + 1, name


def test_connectivity_8_is_the_warp_of_the_complements():
    g, p = ref.cells_pair(1, 9, 128, 128)
    r8 = ref.warp_batch(g[None], p[None], connectivity=8)
    L = ref.warp(~g, ~p, ref.may_mask(g))[0]
    assert np.array_equal(r8["warped"][0], (~L).astype(np.int32))
    fg8, bg4 = ndimage.label(r8["warped"][0], ref.FULL)[1], ndimage.label(r8["warped"][0] == 0, ref.CROSS)[1]
    assert (fg8, bg4) == (ndimage.label(g, ref.FULL)[1], ndimage.label(~g, ref.CROSS)[1])
    assert r8["mismatch"][0] == (r8["warped"][0] != p).sum() and r8["mismatch_map"][0].sum() == r8["mismatch"][0]


def test_a_hole_in_the_prediction_stays():
    g = disc(21, 23, 10, 11, 6)
    p = g.copy()
    p[10, 11] = False
    r = ref.scores(p[None], g[None])
    assert r["mismatch"].tolist() == [1] and r["mismatch_before"].tolist() == [1] and r["flips"].tolist() == [0]
    assert r["sweeps"] == 1 and r["error_regions"].tolist() == [1] and r["warping_error"][0] == 1 / (21 * 23)


def test_a_shifted_disc_warps_onto_itself():
    g = disc(31, 33, 15, 14, 7)
    p = ref.shifted(g, 0, 2)
    r = ref.scores(p[None], g[None])
    assert r["mismatch"].tolist() == [0] and r["flips"].tolist() == [int((g != p).sum())] and r["error_regions"].tolist() == [0]
    assert np.array_equal(r["warped"][0], p.astype(np.int32))
    near = ref.scores(p[None], g[None], reach=1)
    assert 0 < near["mismatch"][0] < near["mismatch_before"][0]


def test_a_merged_blob_keeps_two_cells():
    g = disc(25, 41, 12, 11, 6) | disc(25, 41, 12, 29, 6)
    p = g.copy()
    p[10:15, 11:30] = True                                   # a bridge between the two
    r = ref.scores(p[None], g[None])
    assert ref.components(r["warped"][0]) == ref.components(g) == (2, 1)
    assert r["mismatch"][0] > 0 and r["error_regions"][0] >= 1
    assert (r["mismatch_map"][0] & ~(p & ~g)).sum() == 0     # what is left lies on the bridge


def test_one_class_with_a_reach_has_nothing_to_flip():
    p = disc(17, 19, 8, 9, 4)
    for g in (np.zeros((17, 19), bool), np.ones((17, 19), bool)):
        assert not ref.may_mask(g, 5).any()
        r = ref.scores(p[None], g[None], reach=5)
        assert r["flips"].tolist() == [0] and r["sweeps"] == 1 and r["mismatch"].tolist() == [int((g != p).sum())]
        assert ref.scores(p[None], g[None])["flips"][0] == 0 or not g.any()


def test_the_reach_is_the_exact_squared_distance():
    g = np.zeros((21, 23), bool)
    g[10, 11] = True
    yy, xx = np.mgrid[0:21, 0:23]
    d2 = (yy - 10) ** 2 + (xx - 11) ** 2
    for reach in (0, 1, 2.5, 5):
        want = (d2 <= ref.dist2(reach)) & (d2 > 0) & ref.interior(21, 23)
        if ref.dist2(reach) >= 1:
            want[10, 11] = True                              # the pixel itself: its nearest background is at d^2 = 1
        assert np.array_equal(ref.may_mask(g, reach), want), reach


def test_the_inputs_of_the_gpu_tests_exercise_the_code():
    """On the restatement alone: the cases flip, leave a mismatch, and between them need more sweeps than one launch of 16
    passes holds and more launches than one round of the wrapper enqueues."""
    sweeps = {}
    for H, W in ((33, 31), (63, 65), (129, 97), (257, 255)):
        for name, g, p in ref.size_cases(H, W):
            r = ref.warp_batch(g, p)
            assert r["flips"].sum() > 0 and ((0 < r["mismatch"]) & (r["mismatch"] < r["mismatch_before"])).any(), (name, H, W)
            if name == "mixed":
                assert r["flips"][0] > 0 and r["flips"][3] == 0 and r["mismatch_before"][3] == 0
            sweeps[(name, H, W)] = r["sweeps"]
    assert max(sweeps.values()) > P_MAX // 4, sweeps
    g, p = ref.corridor(9, 400)
    L, count, n, _ = ref.warp(g, p, ref.may_mask(g))
    assert n == 200 and not (L != p).any() and n > LAUNCHES * P_MAX // 4
    g, p = ref.cells_pair(3, 99, 388, 388)
    r = ref.scores(p[None], g[None], reach=5)
    assert r["flips"][0] > 0 and 0 < r["mismatch"][0] < r["mismatch_before"][0] and r["error_regions"][0] > 1


def test_inputs_are_what_instances_ref_makes():
    assert np.array_equal(ref.size_cases(33, 31)[1][1][0] != 0, instances_ref.mask_batch("serpentine", 64, 33, 31)[0] != 0)
