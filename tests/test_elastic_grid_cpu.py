"""The restatement tests/elastic_grid_ref.py of the paper's elastic deformation against oracles nobody here wrote -
torch's bicubic interpolate for the displacement field, scipy's map_coordinates for the warp - and the host side of the
feature: the library's new entries, the ValueErrors of data.elastic_grid / data.augment / data.CropDataset that are raised
before anything touches a device, and the draw order of data.grid_displacements.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import elastic_grid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_elastic_grid", "unet_elastic_grid_sample", "unet_normalise01")
SHAPES = ((37, 53), (64, 48), (61, 61))
GRIDS = (2, 3, 5)


def test_field_equals_torch_bicubic_at_minus_three_quarters():
    """a = -0.75 is the cubic torch interpolates with; align_corners=True is the corner-aligned grid.  fp64 both sides: a
    dozen roundings of values of a few tens, 1e-12 with two orders to spare."""
    worst = 0.0
    for H, W in SHAPES:
        for G in GRIDS:
            g = np.random.RandomState(100 * G + H).normal(0, 10, (2, G, G))
            want = torch.nn.functional.interpolate(torch.from_numpy(g)[None], size=(H, W), mode="bicubic", align_corners=True)[0].numpy()
            got = ref.field(g, H, W, a=-0.75)
            assert got.shape == (2, H, W) and got.dtype == np.float64
            worst = max(worst, float(np.abs(got - want).max()))
            assert np.abs(ref.field(g, H, W, a=-0.5) - want).max() > 1e-3          # the parameter is not decoration
    print("field vs torch bicubic: largest difference %.3g" % worst)
    assert worst <= 1e-12


def test_warp_equals_scipy_map_coordinates():
    from scipy.ndimage import map_coordinates
    worst, outside = 0.0, []
    for (H, W), G in zip(SHAPES, (3, 2, 5)):
        rs = np.random.RandomState(5 + G)
        img = rs.rand(H, W) * 255
        cy, cx = ref.coordinates(rs.normal(0, 10, (2, G, G)), H, W)
        want = map_coordinates(img, np.stack([cy, cx]), order=1, mode="constant", cval=0.0)
        got = ref.bilinear(img, cy, cx)
        worst = max(worst, float(np.abs(got - want).max()))
        out = (cy < 0) | (cy > H - 1) | (cx < 0) | (cx > W - 1)
        assert (got[out] == 0).all()
        outside.append(out.mean())
    print("warp vs scipy: largest difference %.3g; share of pixels outside %s" % (worst, np.round(outside, 3)))
    assert worst <= 1e-12
    assert max(outside) > 0.03


def test_field_at_the_node_pixels_is_the_node_values():
    for H, W, G in ((37, 53, 3), (61, 61, 5), (61, 61, 3), (64, 48, 2), (9, 13, 5)):
        assert (H - 1) % (G - 1) == 0 and (W - 1) % (G - 1) == 0
        g = np.random.RandomState(G).normal(0, 10, (2, G, G))
        for a in (-0.5, -0.75):
            f = ref.field(g, H, W, a)
            assert np.array_equal(f[:, ::(H - 1) // (G - 1), ::(W - 1) // (G - 1)], g)
    # each row of the weight matrices adds up to 1: a constant grid moves every pixel alike
    for n, G in ((37, 3), (64, 2), (61, 5), (700, 3)):
        assert np.abs(ref.axis_matrix(n, G, -0.5).sum(1) - 1).max() < 1e-14


def test_fused_sample_is_the_warp_rounded_cropped_and_thresholded():
    rs = np.random.RandomState(3)
    S, pad, crop = 40, 6, 28
    img, mask = rs.rand(2, S, S) * 255, (rs.rand(2, S, S) > 0.5) * 255.0
    g = rs.normal(0, 4, (2, 2, 3, 3))
    r = ref.sample(img, mask, g, -0.5, 255, pad, crop)
    w = ref.warp(np.stack([img, mask]), g)
    assert np.array_equal(r["out_img"], np.clip(np.floor(w[0] + 0.5), 0, 255).astype(np.float32))
    assert np.array_equal(r["out_gt"], (np.floor(w[1] + 0.5) > 127)[:, pad:pad + crop, pad:pad + crop])
    assert r["out_gt"].dtype == np.int64 and r["out_gt"].shape == (2, crop, crop)
    assert np.array_equal(r["minmax"][:, 0], r["out_img"].min((1, 2))) and np.array_equal(r["minmax"][:, 1], r["out_img"].max((1, 2)))
    assert np.array_equal(ref.sample(img, mask, g, -0.5, 0, pad, crop)["out_img"], w[0].astype(np.float32))
    assert r["reads"].any() and not r["reads"].all()
    n = ref.normalise01(r["out_img"], r["minmax"])
    assert n.dtype == np.float32 and n.min() == 0 and n.max() == 1


def test_library_exports_the_new_entries():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(L, name), name
    assert L.unet_abi_version() == 4
    assert len(_hip._SIGS["unet_elastic_grid"][1]) == 10 and len(_hip._SIGS["unet_elastic_grid_sample"][1]) == 14
    assert len(_hip._SIGS["unet_normalise01"][1]) == 5


def test_library_refuses_bad_arguments_before_any_launch():
    """ARG_CHECK answers on the host: no device is needed to be refused."""
    import ctypes as C
    import _hip
    _hip.build()
    L = _hip.lib()
    p = C.c_void_p(4096)                      # never dereferenced: every call below is refused first
    ok = dict(P=1, B=1, H=8, W=8, G=3)

    def grid(**kw):
        k = dict(ok, **kw)
        return L.unet_elastic_grid(k.get("planes", p), k["P"], k["B"], k["H"], k["W"], k.get("grid", p), k["G"], -0.5, k.get("out", p), None)

    for kw, word in ((dict(planes=None), b"null"), (dict(grid=None), b"null"), (dict(out=None), b"null"), (dict(G=1), b"2 <= G <= 16"),
                     (dict(G=17), b"2 <= G <= 16"), (dict(H=1), b"H, W >= 2"), (dict(W=1), b"H, W >= 2"), (dict(B=0), b"B"), (dict(P=0), b"plane")):
        assert grid(**kw) == -2, kw
        assert word in L.unet_last_error(), (kw, L.unet_last_error())

    def sample(img=p, mask=p, S=16, g=p, G=3, levels=255, pad=2, crop=12, out=p, gt=p, mm=p):
        return L.unet_elastic_grid_sample(img, mask, 1, S, g, G, -0.5, levels, pad, crop, out, gt, mm, None)

    for kw, word in ((dict(img=None), b"null"), (dict(mask=None), b"null"), (dict(g=None), b"null"), (dict(out=None), b"null"),
                     (dict(gt=None), b"null"), (dict(mm=None), b"null"), (dict(G=1), b"2 <= G <= 16"), (dict(G=17), b"2 <= G <= 16"),
                     (dict(S=1, pad=0, crop=1), b"H, W >= 2"), (dict(pad=5, crop=12), b"pad + crop > S"), (dict(pad=-1), b"pad + crop > S"),
                     (dict(crop=0), b"pad + crop > S"), (dict(levels=100), b"levels")):
        assert sample(**kw) == -2, kw
        assert word in L.unet_last_error(), (kw, L.unet_last_error())
    assert L.unet_normalise01(None, 1, 16, p, None) == -2 and b"null" in L.unet_last_error()
    assert L.unet_normalise01(p, 1, 16, None, None) == -2 and b"null" in L.unet_last_error()
    assert L.unet_normalise01(p, 0, 16, p, None) == -2 and b"shape" in L.unet_last_error()
    assert L.unet_normalise01(p, 1, 0, p, None) == -2 and b"shape" in L.unet_last_error()


def test_host_errors():
    import data
    img = torch.zeros(20, 20)
    with pytest.raises(ValueError, match="device"):
        data.elastic_grid((img,), np.zeros((2, 3, 3)))
    with pytest.raises(ValueError, match="device"):
        data.elastic_grid((img, img), np.zeros((1, 2, 3, 3)))
    with pytest.raises(ValueError):
        data.elastic_grid((), np.zeros((2, 3, 3)))
    # the grid's own checks need no device either
    for bad in (np.zeros((2, 1, 1)), np.zeros((3, 2, 3, 3)), np.zeros((2, 3, 4)), np.zeros((1, 3, 3)), np.zeros((2, 17, 17)), np.zeros(18)):
        with pytest.raises(ValueError, match="elastic_grid"):
            data._grid_tensor(bad, 2, torch.device("cpu"), "elastic_grid")
    d = data._grid_tensor(np.ones((2, 3, 3), np.float32), 2, torch.device("cpu"), "elastic_grid")
    assert d.shape == (2, 2, 3, 3) and d.dtype == torch.float64 and d.is_contiguous()
    d = data._grid_tensor(torch.ones(2, 2, 4, 4, dtype=torch.float16), 2, torch.device("cpu"), "elastic_grid")
    assert d.shape == (2, 2, 4, 4) and d.dtype == torch.float64
    tgt = torch.zeros(20, 20)
    with pytest.raises(ValueError, match="'field' or 'grid'"):
        data.augment(img, tgt, (0, 0), 12, 0, 3, 10, elastic="bicubic")
    with pytest.raises(ValueError, match="random_state"):
        data.augment(img, tgt, (0, 0), 12, 0, 3, 10, elastic="grid")
    with pytest.raises(ValueError, match="at least 2"):
        data.grid_displacements(np.random.RandomState(0), 1, grid=1)
    with pytest.raises(ValueError, match="RandomState"):
        data.grid_displacements(None, 1)
    images, inst = np.zeros((1, 30, 30), np.uint8), np.zeros((1, 30, 30), np.uint16)
    with pytest.raises(ValueError, match="'field' or 'grid'"):
        data.CropDataset(images, inst, 3, 10, 12, 1, np.random.RandomState(0), elastic="grid3", device="cpu")
    with pytest.raises(ValueError, match="random_state"):
        data.CropDataset(images, inst, 3, 10, 12, 1, np.random.RandomState(0), elastic="grid", device="cpu")
    with pytest.raises(ValueError, match="at least 2"):
        data.CropDataset(images, inst, 3, 10, 12, 1, np.random.RandomState(0), elastic="grid", grid=1, random_state=np.random.RandomState(1),
                         device="cpu")


def test_grid_displacements_draw_order():
    """[B,2,G,G] filled in C order from one normal() call: sample after sample, rows' plane before columns' plane, 2 G^2 draws
    per sample and no other - replayed here draw by draw, and the generator is left where the replay leaves it."""
    import data
    for B, G, sigma in ((1, 3, 10.0), (3, 3, 10.0), (2, 5, 4.0), (4, 2, 1.5)):
        rs, replay = np.random.RandomState(11), np.random.RandomState(11)
        d = data.grid_displacements(rs, B, G, sigma)
        assert d.shape == (B, 2, G, G) and d.dtype == np.float64
        for b in range(B):
            rows = replay.normal(0, sigma, (G, G))
            cols = replay.normal(0, sigma, (G, G))
            assert np.array_equal(d[b, 0], rows) and np.array_equal(d[b, 1], cols)
        assert rs.randint(1 << 30) == replay.randint(1 << 30)
    assert np.array_equal(data.grid_displacements(np.random.RandomState(4), 2), np.random.RandomState(4).normal(0, 10.0, (2, 2, 3, 3)))
