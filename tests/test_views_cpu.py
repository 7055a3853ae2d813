"""The dihedral views of tester.segment(views=...) without a GPU: the view codes against their three-line numpy definition, the
named sets, parse_views' errors, the chunking of the concatenated tile list, and the C ABI of the two new entry points."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_tile_gather_view", "unet_tile_stitch_view")
SHAPES = [(3, 5), (4, 4), (2, 3, 5)]


def numpy_view(I, v):
    """The definition (on the last two axes)."""
    t, fy, fx = v & 1, (v >> 1) & 1, (v >> 2) & 1
    V = np.swapaxes(I, -1, -2) if t else I
    if fy:
        V = V[..., ::-1, :]
    if fx:
        V = V[..., :, ::-1]
    return V


def distinct(shape):
    return np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) + 1


def test_the_definition_on_one_image_is_the_three_lines_of_the_issue():
    I = distinct((3, 5))
    for v in range(8):
        V = I.T if v & 1 else I
        if (v >> 1) & 1:
            V = V[::-1]
        if (v >> 2) & 1:
            V = V[:, ::-1]
        assert np.array_equal(numpy_view(I, v), V)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("v", range(8))
def test_apply_view_is_the_numpy_definition(shape, v):
    import tester
    I = distinct(shape)
    want = numpy_view(I, v)
    got = tester.apply_view(I, v)
    assert isinstance(got, np.ndarray) and got.shape == want.shape and np.array_equal(got, want)
    gt = tester.apply_view(torch.from_numpy(I), v)
    assert torch.is_tensor(gt) and np.array_equal(gt.contiguous().numpy(), want)
    assert want.shape[-2:] == tester.view_shape(shape[-2], shape[-1], v)
    assert np.array_equal(tester.undo_view(got, v), I)
    assert torch.equal(tester.undo_view(gt, v), torch.from_numpy(I))
    # the index map of the issue, pixel by pixel
    H, W = shape[-2:]
    Hv, Wv = tester.view_shape(H, W, v)
    for y, x in itertools.product(range(Hv), range(Wv)):
        y1 = Hv - 1 - y if (v >> 1) & 1 else y
        x1 = Wv - 1 - x if (v >> 2) & 1 else x
        src = (x1, y1) if v & 1 else (y1, x1)
        assert np.array_equal(got[..., y, x], I[..., src[0], src[1]])


def test_view_shape():
    import tester
    for v in range(8):
        assert tester.view_shape(3, 5, v) == ((5, 3) if v & 1 else (3, 5))
        assert tester.view_shape(4, 4, v) == (4, 4)


@pytest.mark.parametrize("shape", SHAPES)
def test_rot4_is_rot90_and_the_eight_views_differ(shape):
    import tester
    I = distinct(shape)
    assert tester.parse_views("rot4") == (0, 3, 6, 5)
    for k, v in enumerate(tester.parse_views("rot4")):
        assert np.array_equal(tester.apply_view(I, v), np.rot90(I, k, axes=(-2, -1)))
    views = [tester.apply_view(I, v) for v in range(8)]
    for a, b in itertools.combinations(range(8), 2):
        assert views[a].shape != views[b].shape or not np.array_equal(views[a], views[b]), (a, b)


def test_parse_views_accepts():
    import tester
    assert tester.parse_views("rot4") == (0, 3, 6, 5)
    assert tester.parse_views("flips") == (0, 2, 4, 6)
    assert tester.parse_views("d4") == (0, 1, 2, 3, 4, 5, 6, 7)
    assert tester.parse_views((5,)) == (5,)
    assert tester.parse_views([7, 0, 3]) == (7, 0, 3)
    assert tester.parse_views((1, 6)) == (1, 6)
    assert tester.parse_views(np.array([2, 1])) == (2, 1)
    assert tester.parse_views(range(7, -1, -1)) == (7, 6, 5, 4, 3, 2, 1, 0)
    assert all(type(v) is int for v in tester.parse_views(np.array([2, 1])))


@pytest.mark.parametrize("bad,names", [((), "()"), ((0, 0), "0"), ((8,), "8"), ((-1,), "-1"), ("rot3", "rot3"), (1.5, "1.5"),
                                       ((1, 2.0), "2.0"), ((True,), "True"), (None, "None")])
def test_parse_views_rejects_and_names_the_value(bad, names):
    import tester
    with pytest.raises(ValueError, match=re.escape(names)):
        tester.parse_views(bad)
    for f in (tester.apply_view, tester.undo_view):
        with pytest.raises(ValueError):
            f(np.zeros((2, 2)), 8)


@pytest.mark.parametrize("n_views,Tv,nb", [(1, 1, 1), (8, 1, 16), (8, 2, 16), (4, 24, 5), (8, 24, 3), (4, 12, 12), (3, 7, 50)])
def test_chunks_cover_the_tile_list_once_in_order(n_views, Tv, nb):
    import tester
    seen = []
    t_next = 0
    for t0, n, segs in tester._view_chunks(n_views, Tv, min(nb, n_views * Tv)):
        assert t0 == t_next and 1 <= n <= nb
        off = 0
        for k, a, m, o in segs:
            assert o == off and m >= 1 and 0 <= a and a + m <= Tv and 0 <= k < n_views
            seen += [(k, a + i) for i in range(m)]
            off += m
        assert off == n
        assert [s[0] for s in segs] == sorted({s[0] for s in segs})            # one segment per view in a chunk, in view order
        t_next += n
    assert seen == [(k, a) for k in range(n_views) for a in range(Tv)]


def test_abi_declares_and_exports_the_new_entry_points():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(L, name), name
    assert L.unet_abi_version() == 4
    assert len(_hip._SIGS["unet_tile_gather_view"][1]) == 15 and len(_hip._SIGS["unet_tile_stitch_view"][1]) == 18


def test_segment_takes_views_and_host_arguments_are_checked_first():
    import inspect
    import tester
    sig = inspect.signature(tester.segment)
    assert sig.parameters["views"].default is None
    assert list(sig.parameters)[:7] == ["unet", "images", "tile_size", "max_batch", "normalise", "return_probs", "return_instances"]
    with pytest.raises(RuntimeError, match="HIP device"):
        tester.segment(None, torch.zeros(4, 4), views="d4")
