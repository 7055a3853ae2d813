"""The numpy restatement with a connectivity (tests/conn_ref.py), which tests/test_conn_gpu.py holds the 8-connected sweeps to,
pinned on the CPU.  At connectivity 4 it equals split_ref.grow, flood_ref.flood, shape_ref.reconstruct and shape_ref.seeds bit
for bit on their own cases.  At connectivity 8 the growth is held to a per-seed distance by masked binary dilation with the full
3 x 3 structure, the reconstruction to a synchronous grey dilation, the flood to the level loop over the growth, and all of them
to hand-worked answers.  Every input of the device tests is shown to differ between 4 and 8.  And the surface: the four _conn
entries declared, in the ctypes table and in the library; the pinned Python signatures unchanged; a bad connectivity refused."""
import os
import re

import numpy as np
import pytest

import conn_ref as ref
import flood_ref
import shape_ref
import split_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"unet_geodesic_sweeps_conn": 10, "unet_flood_sweeps_conn": 10, "unet_flood_assign_conn": 9, "unet_reconstruct_sweeps_conn": 9}
SMALL = [s for s in ref.GROW_SIZES if s[0] * s[1] <= 65 * 63]


def images(cases):
    for name, s, m in cases:
        for b in range(len(s)):
            yield "%s[%d]" % (name, b), s[b], m[b]


# ---- connectivity 4: the existing restatements, bit for bit ---------------------------------------------------------------------

@pytest.mark.parametrize("H,W", ref.GROW_SIZES)
def test_growth_at_4_is_split_ref(H, W):
    for name, s, m in images(split_ref.size_cases(H, W)):
        for steps in split_ref.STEPS:
            got, want = ref.grow(s, m, steps, 4), split_ref.grow(s, m, steps)
            for k in want:
                assert np.array_equal(got[k], want[k]), (name, steps, k)
        assert np.array_equal(ref.keep_orphans(got["out"], s, m, 4), split_ref.keep_orphans(want["out"], s, m)), name


@pytest.mark.parametrize("H,W", SMALL)
def test_flood_at_4_is_flood_ref(H, W):
    for name, s, im, m in flood_ref.size_cases(H, W):
        for top in (None, 2):
            got = ref.flood_batch(s, im, m, max_level=top, connectivity=4)
            want = flood_ref.flood_batch(s, im, m, max_level=top)
            for k in want:
                assert np.array_equal(got[k], want[k]), (name, top, k)


@pytest.mark.parametrize("H,W", ref.RECON_SIZES)
def test_reconstruction_at_4_is_shape_ref(H, W):
    for with_mask in (True, False):
        marker, under, mask = shape_ref.recon_case(H, W, 2, with_mask=with_mask)
        got, want = ref.reconstruct_batch(marker, under, mask, 4), shape_ref.reconstruct_batch(marker, under, mask)
        for k in want:
            assert np.array_equal(got[k], want[k]), (with_mask, k)
    marker[0, 0, 0], under[0, H - 1, W - 1] = -1, shape_ref.TOP + 1          # values out of range count as 0 and are counted
    got, want = ref.reconstruct(marker[0], under[0], None, 4), shape_ref.reconstruct(marker[0], under[0])
    assert got["status"] == want["status"] == 2 and np.array_equal(got["out"], want["out"])


def test_seeds_at_4_are_shape_ref():
    for name, masks in shape_ref.size_cases(65, 66):
        for m in masks:
            for h, r, edge in ((0, 0, "ignore"), (2, 0, "ignore"), (2, 4, "background"), (0.5, 0, "background")):
                ids, n = ref.seeds(m, h, r, edge, 4)
                want, wn = shape_ref.seeds(m, h, r, edge)
                assert n == wn and np.array_equal(ids, want), (name, h, r, edge)


# ---- connectivity 8: pinned by other means ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SMALL)
def test_growth_at_8_is_the_dilation_distance(H, W):
    for name, s, m in images(split_ref.size_cases(H, W)):
        got = ref.grow(s, m, None, 8)
        ids, dist = ref.dilation_distance(s, m, 8)
        assert np.array_equal(got["out"], ids) and np.array_equal(got["dist"], dist), name
        for steps in (0, 1, 5):
            cut = ref.grow(s, m, steps, 8)
            keep = (dist >= 0) & (dist <= steps)
            assert np.array_equal(cut["out"], np.where(keep, ids, 0)) and np.array_equal(cut["dist"], np.where(keep, dist, -1)), (name, steps)


@pytest.mark.parametrize("H,W", ref.RECON_SIZES)
def test_reconstruction_at_8_is_the_grey_dilation(H, W):
    for with_mask in (True, False):
        marker, under, mask = shape_ref.recon_case(H, W, 2, with_mask=with_mask)
        for b in range(2):
            region = np.ones((H, W), bool) if mask is None else mask[b] != 0
            got = ref.reconstruct(marker[b], under[b], None if mask is None else mask[b], 8)
            R = ref.dilation_fixed_point(marker[b], under[b], region, 8)
            assert np.array_equal(got["out"], np.where(region, R, 0)), (with_mask, b)
            assert got["raised"] == int((region & (R > np.minimum(marker[b], under[b]))).sum())


def test_flood_at_8_is_the_level_loop():
    n = 0
    for name, s, im, m in flood_ref.small_cases() + [("random %d" % k,) + c for k, c in enumerate(flood_ref.random_small(20))]:
        got = ref.flood(s, im, m, connectivity=8)
        out, level = ref.level_loop(s, im, m, connectivity=8)
        assert np.array_equal(got["out"], out) and np.array_equal(got["pass_level"], level), name
        n += 1
    assert n >= 30


def test_constant_flood_at_8_is_the_growth():
    for H, W in ((33, 31), (65, 63)):
        s, m = split_ref.busy(H, W)
        f, g = ref.flood(s, np.full((H, W), 3, np.int32), m, connectivity=8), ref.grow(s, m, None, 8)
        assert np.array_equal(f["out"], g["out"])
        reached = g["dist"] > 0
        assert np.array_equal(f["dist"][reached], g["dist"][reached]) and (f["pass_level"][reached] == 3).all()


def test_the_diagonal_discs():
    m = ref.diagonal_discs()
    assert [ref.seeds(m, h, connectivity=8)[1] for h in ref.DISC_HS] == [2, 2, 2, 2]
    assert [ref.seeds(m, h, connectivity=4)[1] for h in ref.DISC_HS] == [9, 3, 2, 2]
    assert [shape_ref.seeds(m, h)[1] for h in ref.DISC_HS] == [9, 3, 2, 2]


def test_the_diagonal_corridor():
    for mirror in (False, True):
        s, m = ref.eye_corridor(mirror=mirror)
        r8, r4 = ref.grow(s[0], m[0], None, 8), ref.grow(s[0], m[0], None, 4)
        flip = (lambda x: 129 - x) if mirror else (lambda x: x)
        assert r8["unreached"] == 0 and r8["max_dist"] == 64
        assert r8["out"][64, flip(64)] == 2 and r8["out"][65, flip(65)] == 1
        assert r4["unreached"] == 128 and r4["max_dist"] == 0


def test_the_checkerboard():
    s, m = ref.checkerboard()
    assert s.shape == (1, 65, 67)
    r8, r4 = ref.grow(s[0], m[0], None, 8), ref.grow(s[0], m[0], None, 4)
    assert r8["unreached"] == 0 and r8["max_dist"] == 66
    assert r4["unreached"] == 2177 == int(m.sum()) - 1


def test_the_membrane():
    s, im = ref.membrane()
    f4, f8 = ref.flood(s, im, connectivity=4), ref.flood(s, im, connectivity=8)
    far = np.add.outer(np.arange(8), np.arange(8)) > 7
    assert (f4["pass_level"][far] == 9).all() and (f8["pass_level"][far] == 0).all()
    assert (f4["out"] == 4).all() and (f8["out"] == 4).all()
    assert (f8["pass_level"][im == 9] == 9).all()            # the membrane itself is as high as it is


def test_a_diagonal_tie_goes_to_the_smaller_id():
    s, m = ref.diagonal_tie()
    assert ref.grow(s, m, None, 8)["out"].tolist() == [[7, 7, 3], [7, 3, 3], [3, 3, 3]]
    assert ref.grow(s, m, None, 8)["dist"].tolist() == [[0, 1, 2], [1, 1, 1], [2, 1, 0]]
    f = ref.flood(s, np.zeros((3, 3), np.int32), connectivity=8)
    assert f["out"].tolist() == [[7, 7, 3], [7, 3, 3], [3, 3, 3]]


def test_the_corner_pairs():
    s, m = ref.corner_pairs()
    assert s.shape == (8, 129, 129) and (m.sum(axis=(1, 2)) == 2).all() and ((s > 0).sum(axis=(1, 2)) == 1).all()
    r8, r4 = ref.grow_batch(s, m, None, 8), ref.grow_batch(s, m, None, 4)
    assert (r8["unreached"] == 0).all() and (r8["max_dist"] == 1).all() and (r4["unreached"] == 1).all()
    for b in range(8):                                       # the two pixels lie in different tile rows and columns
        (y0, y1), (x0, x1) = np.nonzero(m[b])
        assert y0 // 64 != y1 // 64 and x0 // 64 != x1 // 64


# ---- the inputs of the device tests differ between 4 and 8 ----------------------------------------------------------------------

def test_busy_images_differ():
    assert [int((ref.grow(*split_ref.busy(H, W), None, 4)["out"] != ref.grow(*split_ref.busy(H, W), None, 8)["out"]).sum())
            for H, W in ((33, 31), (65, 63), (129, 97))] == [230, 207, 2455]


@pytest.mark.parametrize("H,W", ref.GROW_SIZES)
def test_growth_inputs_differ(H, W):
    differ = 0
    for name, s, m in split_ref.size_cases(H, W):
        for steps in split_ref.STEPS:
            a, b = ref.grow_batch(s, m, steps, 4), ref.grow_batch(s, m, steps, 8)
            d = not (np.array_equal(a["out"], b["out"]) and np.array_equal(a["dist"], b["dist"]))
            differ += d
            assert d or steps == 0 or H * W < 64, (name, steps)      # with 0 steps there is no step to differ in
    assert differ > 0 or min(H, W) == 1                      # a single row or column has no diagonal


@pytest.mark.parametrize("H,W", SMALL)
def test_flood_inputs_differ(H, W):
    differ = 0
    for name, s, im, m in flood_ref.size_cases(H, W):
        a, b = ref.flood_batch(s, im, m, connectivity=4), ref.flood_batch(s, im, m, connectivity=8)
        differ += not all(np.array_equal(a[k], b[k]) for k in flood_ref.MAPS)
    assert differ > 0 or min(H, W) == 1


def test_reconstruction_and_seed_inputs_differ():
    for H, W in ref.RECON_SIZES:
        for with_mask in (True, False):
            marker, under, mask = shape_ref.recon_case(H, W, 2, with_mask=with_mask)
            a, b = ref.reconstruct_batch(marker, under, mask, 4), ref.reconstruct_batch(marker, under, mask, 8)
            assert H == 1 or not np.array_equal(a["out"], b["out"]), (H, W, with_mask)
    name, masks = shape_ref.size_cases(65, 66)[0]
    assert ref.seeds(masks[0], 0, connectivity=4)[1] != ref.seeds(masks[0], 0, connectivity=8)[1]


def test_the_corner_flood_has_a_parent_across_a_tile_corner():
    s, im, m = ref.corner_flood()
    r = ref.flood(s[0], im[0], m[0], connectivity=8)
    assert ref.parents_across_a_tile_corner(r, im[0]) == 2 and r["unreached"] == 0 and r["max_level"] > 3
    assert ref.flood(s[0], im[0], m[0], connectivity=4)["unreached"] == 128


# ---- the surface ------------------------------------------------------------------------------------------------------------

def test_abi_declares_and_exports_the_new_entry_points():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    for name, n_args in NEW.items():
        proto = re.search(r"\bint %s\s*\(([^)]*)\)" % name, hdr)
        assert proto is not None and name in _hip.EXPORTS and hasattr(L, name), name
        args = [a.strip() for a in proto.group(1).split(",")]
        assert len(args) == n_args == len(_hip._SIGS[name][1]), name
        assert args.index("int connectivity") + 1 == args.index("int n_launches"), name
        assert len(_hip._SIGS[name[:-5]][1]) == n_args - 1   # the entry without _conn keeps its signature
    assert L.unet_abi_version() == 4


def test_library_refuses_a_bad_connectivity_before_any_launch():
    """ARG_CHECK answers on the host: no device is needed to be refused."""
    import ctypes as C
    import _hip
    _hip.build()
    L = _hip.lib()
    q = C.c_void_p(4096)                                     # never dereferenced: every call below is refused first
    for conn in (5, 0, -8, 6):
        assert L.unet_geodesic_sweeps_conn(1, 8, 8, -1, conn, 1, q, 0, q, None) == -2
        assert b"connectivity" in L.unet_last_error() and str(conn).encode() in L.unet_last_error()
        assert L.unet_flood_sweeps_conn(1, 8, 8, -1, conn, 1, q, 0, q, None) == -2 and b"connectivity" in L.unet_last_error()
        assert L.unet_flood_assign_conn(1, 8, 8, conn, 1, q, 0, q, None) == -2 and b"connectivity" in L.unet_last_error()
        assert L.unet_reconstruct_sweeps_conn(1, 8, 8, conn, 1, q, 0, q, None) == -2 and b"connectivity" in L.unet_last_error()
    for conn in (4, 8):                                      # the other checks hold as they do without _conn
        assert L.unet_geodesic_sweeps_conn(1, 8, 8, -1, conn, 0, q, 0, q, None) == -2
        assert L.unet_flood_sweeps_conn(1, 8, 8, -1, conn, 1, None, 0, q, None) == -2
        assert L.unet_flood_assign_conn(1, 8, 8, conn, 1, q, -1, q, None) == -2
        assert L.unet_reconstruct_sweeps_conn(1, 8, 8, conn, 1, q, 0, None, None) == -2
        assert L.unet_geodesic_sweeps_conn(1, 1, 70000, -1, conn, 1, q, 0, q, None) == -2 and b"too large" in L.unet_last_error()


def test_python_surface():
    import inspect
    import torch
    import functions
    import tester
    # the whole signature as text: every name, what is before the * (positional or keyword) and after it (keyword only), every default
    sig = lambda f: str(inspect.signature(f))
    assert sig(functions.split_cells) == "(seeds, mask, *, max_steps=None, orphans='drop', return_distance=False, _launches=8, connectivity=4)"
    assert sig(functions.watershed) == ("(seeds, image, *, mask=None, levels=None, max_level=None, return_levels=False, _launches=8, "
                                        "connectivity=4)")
    assert sig(tester.split_instances) == "(mask, fg_prob, high, *, connectivity=4)"
    assert sig(tester.split_by_watershed) == "(mask, fg_prob, high, levels=64, *, connectivity=4)"
    assert sig(tester.segment) == ("(unet, images, tile_size=None, max_batch=16, normalise=True, return_probs=False, return_instances=False, "
                                   "views=None, clean=None, shape_split=None, split=None, *, measure=False, watershed=None, connectivity=None)")
    seg = list(inspect.signature(tester.segment).parameters.values())
    P = inspect.Parameter
    assert [p.name for p in seg if p.kind is P.POSITIONAL_OR_KEYWORD][-1] == "split"        # the last one a positional caller reaches
    assert [(p.name, p.kind, p.default) for p in seg[-3:]] == [("measure", P.KEYWORD_ONLY, False), ("watershed", P.KEYWORD_ONLY, None),
                                                               ("connectivity", P.KEYWORD_ONLY, None)]
    for f in (functions.split_cells, functions.watershed, tester.split_instances, tester.split_by_watershed,
              functions.reconstruct, functions.shape_seeds, tester.split_by_shape):
        p = inspect.signature(f).parameters["connectivity"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 4
    for f in (functions.split_cells, functions.watershed, tester.split_instances, tester.split_by_watershed, tester.segment):
        assert "connectivity" in f.__doc__
    # a bad connectivity is refused first, whatever else is given: host tensors here, which every op refuses as well
    s = torch.zeros(2, 5, 7, dtype=torch.int32)
    p = torch.zeros(2, 5, 7)
    for bad in (6, 0, "8", None, True, 4.5):
        calls = [lambda: functions.split_cells(s, s, connectivity=bad), lambda: functions.watershed(s, s, connectivity=bad),
                 lambda: functions.reconstruct(s, s, connectivity=bad), lambda: functions.shape_seeds(s, connectivity=bad),
                 lambda: tester.split_instances(s, p, 0.5, connectivity=bad), lambda: tester.split_by_shape(s, connectivity=bad),
                 lambda: tester.split_by_watershed(s, p, 0.5, connectivity=bad)]
        if bad is not None:                                  # None is segment's "not given"
            calls.append(lambda: tester.segment(None, p, return_instances=True, connectivity=bad))
        for call in calls:
            with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
                call()
    for conn in (4, 8):                                      # a good one gets as far as the host tensors
        with pytest.raises(NotImplementedError):
            functions.split_cells(s, s, connectivity=conn)
        with pytest.raises(NotImplementedError):
            functions.watershed(s, s, connectivity=conn)
        with pytest.raises(NotImplementedError):
            functions.reconstruct(s, s, connectivity=conn)
        with pytest.raises(NotImplementedError):
            functions.shape_seeds(s, connectivity=conn)
        with pytest.raises(ValueError, match="return_instances"):
            tester.segment(None, p, connectivity=conn)


def test_segment_checks_fire_in_one_order():
    """segment's argument checks fire in one fixed order, whichever keywords are present: the values of connectivity, measure and
    watershed; what measure, connectivity and watershed need; split; shape_split; the device; then everything else.  A host
    tensor stands in for "wrong in something checked later": no device is needed."""
    import torch
    import tester
    V, R = ValueError, RuntimeError
    table = [(dict(connectivity=5, measure="yes", watershed="x"), V, "connectivity must be 4 or 8"),
             (dict(measure="yes", watershed="x"), V, "measure must be"),
             (dict(watershed="x", measure=True), V, "watershed must be"),
             (dict(measure=True), V, "measure needs"),
             (dict(measure=True, connectivity=8), V, "measure needs"),
             (dict(connectivity=8), V, "return_instances"),
             (dict(connectivity=4), V, "return_instances"),
             (dict(connectivity=8, return_instances=True, split=2), V, "split must be"),
             (dict(connectivity=8, return_instances=True, split=0.5, shape_split=1.0), V, "two ways"),
             (dict(connectivity=8, return_instances=True, shape_split=-1), V, "shape_split must be"),
             (dict(connectivity=8, return_instances=True, clean=3), R, "HIP device"),
             (dict(connectivity=8, return_instances=True, views="rot3"), R, "HIP device"),
             (dict(watershed=16), V, "needs split"),
             (dict(watershed=16, return_instances=True, split=0.5, shape_split=2.0), V, "does not combine"),
             (dict(watershed=16, split=0.5), V, "split needs return_instances"),
             (dict(watershed=16, split=2, return_instances=True), V, "split must be"),
             (dict(clean=3), R, "HIP device"),
             (dict(views="rot3"), R, "HIP device"),
             (dict(tile_size=600), R, "HIP device"),
             (dict(max_batch=0), R, "HIP device"),
             (dict(measure=True, return_instances=True), R, "HIP device"),
             # the two rows that changed when the checks got one order: a bad split or shape_split used to be reported after the
             # device (RuntimeError "HIP device") unless measure, watershed or connectivity was given as well
             (dict(split=2), V, "split needs return_instances"),
             (dict(shape_split=2.0), V, "shape_split needs return_instances")]
    for kw, error, word in table:
        with pytest.raises(error, match=word):
            tester.segment(None, torch.zeros(2, 5, 7), **kw)
