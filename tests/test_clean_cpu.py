"""The numpy restatement of the mask clean-up (tests/clean_ref.py), which tests/test_clean_gpu.py holds the device op to, pinned
on the CPU: the fill against scipy.ndimage.binary_fill_holes with the dual structure, the labels against ndimage.label, the areas
against np.bincount, hand-worked cases, and that the inputs of the GPU tests exercise the code.  And the new surface: entry
points declared, in the ctypes table and in the library, refusing bad arguments on the host; the Python signatures."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import clean_ref as ref
import shape_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_label_components_conn_scratch_bytes", "unet_label_components_conn", "unet_clean_mask_scratch_bytes", "unet_clean_mask")


# ---- the surface ----------------------------------------------------------------------------------------------------------------

def test_abi_declares_and_exports_the_new_entry_points():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(L, name), name
    assert L.unet_abi_version() == 4
    assert len(_hip._SIGS["unet_label_components_conn"][1]) == 11 and len(_hip._SIGS["unet_clean_mask"][1]) == 15
    assert L.unet_clean_mask_scratch_bytes(2, 33, 31) >= 2 * 33 * 31 * 13       # parent, label, attributes, the filled plane
    assert L.unet_label_components_conn_scratch_bytes(2, 33, 31) >= 2 * 33 * 31 * 4
    assert L.unet_clean_mask_scratch_bytes(2, 0, 31) == 0 and L.unet_label_components_conn_scratch_bytes(0, 3, 3) == 0


def test_library_refuses_bad_arguments_before_any_launch():
    """ARG_CHECK answers on the host: no device is needed to be refused."""
    import ctypes as C
    import _hip
    _hip.build()
    L = _hip.lib()
    q = C.c_void_p(4096)                                     # never dereferenced: every call below is refused first

    def clean(mask=q, dtype=0, B=1, H=8, W=8, conn=4, fill=1, hole=-1, small=0, border=0, out=q, action=q, info=q, scratch=q):
        return L.unet_clean_mask(mask, dtype, B, H, W, conn, fill, hole, small, border, out, action, info, scratch, None)

    def label(mask=q, dtype=0, B=1, H=8, W=8, conn=8, phase=1, labels=q, n=q, scratch=q):
        return L.unet_label_components_conn(mask, dtype, B, H, W, conn, phase, labels, n, scratch, None)

    for kw in ({"dtype": 4}, {"dtype": -1}):
        assert clean(**kw) == -2 and b"dtype" in L.unet_last_error()
        assert label(**kw) == -2 and b"dtype" in L.unet_last_error()
    for conn in (0, 6, 12, -4):
        assert clean(conn=conn) == -2 and b"connectivity" in L.unet_last_error()
        assert label(conn=conn) == -2 and b"connectivity" in L.unet_last_error()
    assert clean(hole=-2) == -2 and b"max_hole_area" in L.unet_last_error()
    assert clean(small=-1) == -2 and b"min_area" in L.unet_last_error()
    for phase in (-1, 2):
        assert label(phase=phase) == -2 and b"phase" in L.unet_last_error()
    for name in ("mask", "out", "info", "scratch"):
        assert clean(**{name: None}) == -2
    for name in ("mask", "labels", "n", "scratch"):
        assert label(**{name: None}) == -2
    for kw in ({"B": 0}, {"H": 0}, {"W": -1}):
        assert clean(**kw) == -2 and label(**kw) == -2
    for kw in ({"H": 70000, "W": 1}, {"H": 65535, "W": 65535}, {"B": 70000}):
        assert clean(**kw) == -2 and b"too large" in L.unet_last_error()
        assert label(**kw) == -2 and b"too large" in L.unet_last_error()


def test_python_surface():
    import torch
    import functions
    import tester
    sig = inspect.signature(functions.clean_mask)
    assert list(sig.parameters) == ["mask", "fill_holes", "max_hole_area", "min_area", "drop_border", "connectivity", "return_info",
                                    "return_action"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [True, None, 0, False, 4, False, False]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters.values())[1:])
    assert functions.CleanInfo._fields == ref.INFO
    sig = inspect.signature(functions.label_cells)
    assert list(sig.parameters) == ["mask", "connectivity"] and sig.parameters["connectivity"].default == 4
    sig = inspect.signature(functions.fill_holes)
    assert list(sig.parameters) == ["mask", "max_area", "connectivity"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [None, 4]
    sig = inspect.signature(functions.remove_small)
    assert list(sig.parameters) == ["mask", "min_area", "connectivity"] and sig.parameters["connectivity"].default == 4
    seg = list(inspect.signature(tester.segment).parameters)
    assert seg[:7] == ["unet", "images", "tile_size", "max_batch", "normalise", "return_probs", "return_instances"]
    assert seg[7:] == ["views", "clean", "shape_split", "split", "measure", "watershed", "connectivity"]
    P = inspect.Parameter
    assert [p.kind for p in inspect.signature(tester.segment).parameters.values()] == [P.POSITIONAL_OR_KEYWORD] * 11 + [P.KEYWORD_ONLY] * 3
    assert [p.default for p in inspect.signature(tester.segment).parameters.values()] == [
        P.empty, P.empty, None, 16, True, False, False, None, None, None, None, False, None, None]
    assert inspect.signature(tester.segment).parameters["clean"].default is None

    m = torch.zeros(2, 5, 7, dtype=torch.uint8)
    for host in (m, m.numpy()):
        for call in (functions.clean_mask, functions.fill_holes, lambda t: functions.remove_small(t, 3)):
            with pytest.raises(NotImplementedError):
                call(host)
    with pytest.raises(NotImplementedError):
        functions.label_cells(m, connectivity=8)
    for conn in (0, 6, "8", None):                           # bad values are refused before the device is looked at
        with pytest.raises(ValueError, match="connectivity"):
            functions.clean_mask(m, connectivity=conn)
        with pytest.raises(ValueError, match="connectivity"):
            functions.label_cells(m, connectivity=conn)
        with pytest.raises(ValueError, match="connectivity"):
            functions.fill_holes(m, connectivity=conn)
    for bad in (-1, 2.5, "3", True):
        with pytest.raises(ValueError, match="max_hole_area"):
            functions.clean_mask(m, max_hole_area=bad)
        with pytest.raises(ValueError, match="min_area"):
            functions.clean_mask(m, min_area=bad)
        with pytest.raises(ValueError, match="min_area"):
            functions.remove_small(m, bad)
    with pytest.raises(ValueError, match="min_area"):
        functions.clean_mask(m, min_area=None)
    with pytest.raises(ValueError, match=r"\[H,W\]"):
        functions.clean_mask(m[0, 0])
    for bad in ("yes", 1, {"h": 2}, {"return_info": True}, {"min_area": -1}, {"connectivity": 6}, {"max_hole_area": 1.5}):
        with pytest.raises(ValueError, match="clean"):
            tester._parse_clean(bad, 2)
    assert tester._parse_clean(None, 2) is None and tester._parse_clean(True, 2) == {}
    assert tester._parse_clean({"min_area": 5}, 2) == {"min_area": 5}
    for fills in (True, {"min_area": 5}, {"fill_holes": True}):
        with pytest.raises(ValueError, match="class"):
            tester._parse_clean(fills, 3)
    assert tester._parse_clean({"fill_holes": False, "min_area": 5, "drop_border": True}, 3)["min_area"] == 5


# ---- the restatement against scipy ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gpu_inputs():
    """(name, mask [H,W]) of every seeded image the GPU tests clean."""
    out = []
    for H, W in ref.SIZES + [ref.BIG]:
        for name, m in ref.size_cases(H, W):
            out += [("%s %dx%d[%d]" % (name, H, W, b), m[b]) for b in range(len(m))]
    return out


def test_the_fill_is_binary_fill_holes_with_the_dual_structure():
    """65 x 66 speckle, 20 seeds, and every GPU input: foreground connectivity c <-> binary_fill_holes(structure = the dual)."""
    masks = [ref.speckle(65, 66, s, p) for s in range(20) for p in (0.45, 0.6)] + [m for _, m in gpu_inputs()]
    filled = 0
    for m in masks:
        for conn, S in ((4, ref.FULL), (8, ref.CROSS)):
            got = ref.clean(m, connectivity=conn)
            want = ndimage.binary_fill_holes(m != 0, structure=S)
            assert np.array_equal(got["out"] != 0, want) and np.array_equal(got["action"] == 2, want & (m == 0))
            assert got["info"][1] == (want & (m == 0)).sum() and got["info"][2:6].sum() == 0
            filled += int(got["info"][1])
    assert filled > 1000


def test_labels_are_ndimage_label_in_raster_order_and_areas_bincount():
    for name, m in gpu_inputs():
        for conn, S in ((4, ref.CROSS), (8, ref.FULL)):
            for phase in (0, 1):
                lab, n = ref.label(m, conn, phase)
                want, nw = ndimage.label((m != 0) == bool(phase), S)
                assert n == nw and np.array_equal(lab, want)
                firsts = [int(np.flatnonzero(lab.ravel() == i)[0]) for i in range(1, min(n, 50) + 1)]
                assert firsts == sorted(firsts), (name, conn, phase)     # numbered by first pixel, for the full structure as well
            # the areas the actions rest on, counted another way: remove_small_objects' rule on np.bincount
            got = ref.clean(m, fill_holes=False, min_area=5, connectivity=conn)
            lab, n = ndimage.label(m != 0, S)
            area = np.bincount(lab.ravel())
            assert np.array_equal(got["action"] == 3, (area[lab] < 5) & (lab > 0)) and np.array_equal(got["out"] != 0, (area[lab] >= 5) & (lab > 0))
            assert got["info"][2] == (area[1:] < 5).sum() and got["info"][6] == (area[1:] >= 5).sum()
            # clear_border's rule
            got = ref.clean(m, fill_holes=False, drop_border=True, connectivity=conn)
            edge = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
            assert np.array_equal(got["action"] == 4, np.isin(lab, edge[edge > 0]))
            # small holes: remove_small_holes' rule, the hole's own pixels counted
            got = ref.clean(m, max_hole_area=6, connectivity=conn)
            blab, nb = ndimage.label(m == 0, ref.structure(ref.dual(conn)))
            barea = np.bincount(blab.ravel(), minlength=nb + 1)
            bedge = np.unique(np.concatenate([blab[0], blab[-1], blab[:, 0], blab[:, -1]]))
            want = (blab > 0) & ~np.isin(blab, bedge) & (barea[blab] <= 6)
            assert np.array_equal(got["action"] == 2, want)


def test_the_gpu_inputs_exercise_the_code():
    """Conditions on the inputs, under the restatement alone, so that a weak input cannot hide a failure."""
    busy = 0
    for name, m in gpu_inputs():
        if not name.startswith("busy") or not m.any() or m.all():
            continue                                         # the empty and the full image of the batch of four
        busy += 1
        y, x = ref.POCKET
        for conn in (4, 8):
            all_holes, some = ref.clean(m, connectivity=conn), ref.clean(m, max_hole_area=6, connectivity=conn)
            assert some["info"][0] >= 1, name                                        # a hole that is filled
            assert all_holes["info"][0] > some["info"][0], name                      # a hole too large for max_hole_area = 6
            assert ref.clean(m, max_hole_area=0, connectivity=conn)["info"][0] == 0
            assert m[y, x] == 0 and all_holes["action"][y, x] == 0 and m[y - 2, x] and m[y + 2, x] and m[y, x + 2], name   # the pocket
            before = ref.clean(m, fill_holes=False, connectivity=conn)["info"][6]
            assert all_holes["info"][6] < before and m[6, 6] and all_holes["action"][5, 6] == 2, name    # the island joins the ring
            full = ref.clean(m, min_area=5, drop_border=True, connectivity=conn)["info"]
            assert full[2] >= 1 and full[4] >= 1 and full[6] >= 1, name              # a small, a border and a kept cell
            assert all_holes["action"][6, 6] == 1
        for kw in ({}, {"min_area": 5}):
            differs = (ref.clean(m, connectivity=4, **kw)["action"] != ref.clean(m, connectivity=8, **kw)["action"]).any()
            assert differs, name                                                     # the connectivity matters
    assert busy == 8 * (len(ref.SIZES) - 2 + 1)              # 1 + 2 + 3 + 2 images at every size from 31 x 33 on, ref.BIG included


# ---- hand-worked cases --------------------------------------------------------------------------------------------------------

def info(m, **kw):
    return dict(zip(ref.INFO, ref.clean(m, **kw)["info"].tolist()))


def test_checkerboard():
    m = ref.checkerboard()
    assert ref.label(m, 4)[1] == 2048 and ref.label(m, 8)[1] == 1
    i4, i8 = info(m, connectivity=4), info(m, connectivity=8)
    assert (i4["holes_filled"], i4["cells_kept"]) == (0, 2048)
    assert (i8["holes_filled"], i8["pixels_filled"], i8["cells_kept"]) == (1922, 1922, 1)
    lab, area, is_hole = ref.holes(m, 8)
    assert set(area[is_hole]) == {1}


def test_diagonals_cross_a_tile_corner():
    for anti in (False, True):
        m = ref.diagonal(64, anti)
        assert ref.label(m, 4)[1] == 64 and ref.label(m, 8)[1] == 1
        assert m[31, 32 if anti else 31] and m[32, 31 if anti else 32]       # the pair across the corner of the four 32 x 32 tiles
        assert np.array_equal(ref.label(m, 8)[0], m.astype(np.int32))


def test_diamond():
    m = ref.diamond()
    i4, i8 = info(m, connectivity=4), info(m, connectivity=8)
    assert (i4["cells_kept"], i4["holes_filled"]) == (80, 0)
    assert (i8["cells_kept"], i8["holes_filled"], i8["pixels_filled"]) == (1, 1, 761)


def test_nested_squares():
    m = ref.nested()
    i = info(m)
    assert (i["holes_filled"], i["pixels_filled"], i["cells_kept"]) == (2, 380, 1)
    assert (ref.clean(m)["out"] != 0).sum() == 1024
    i = info(m, max_hole_area=64)
    assert (i["holes_filled"], i["pixels_filled"], i["cells_kept"]) == (1, 60, 2)
    i = info(m, min_area=1025)
    assert (i["cells_small"], i["pixels_small"], i["cells_kept"]) == (1, 1024, 0) and not ref.clean(m, min_area=1025)["out"].any()
    i = info(m, min_area=1024)
    assert (i["cells_small"], i["cells_kept"]) == (0, 1)
    i = info(m, fill_holes=False, min_area=5)
    assert (i["cells_small"], i["pixels_small"], i["cells_kept"], i["holes_filled"]) == (1, 4, 2, 0)


def test_a_pocket_that_reaches_the_frame_diagonally():
    m = ref.diagonal_pocket()
    assert info(m, connectivity=4)["holes_filled"] == 0
    i = info(m, connectivity=8)
    assert (i["holes_filled"], i["pixels_filled"]) == (1, 9)


def test_two_squares_on_a_diagonal_and_the_border():
    m = ref.two_squares()
    i = info(m, drop_border=True, connectivity=4)
    assert (i["cells_border"], i["pixels_border"], i["cells_kept"]) == (1, 9, 1)
    i = info(m, drop_border=True, connectivity=8)
    assert (i["cells_border"], i["pixels_border"], i["cells_kept"]) == (1, 18, 0)


def test_the_ring_shaped_cell():
    """What the GPU test of shape_seeds rests on: under the shape restatement the ring has several seeds, the filled ring one."""
    m = ref.ring_cell()
    assert info(m)["holes_filled"] == 1
    assert shape_ref.seeds(m, 2.0)[1] > 1 and shape_ref.seeds(ref.clean(m)["out"], 2.0)[1] == 1
