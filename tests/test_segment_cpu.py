"""Overlap-tile geometry of tester.segment on the CPU: tester.tile_grid against the brute-force restatement in
tests/segment_ref.py (the output rectangles partition the image, every input window is S wide and centred on its output),
tester.reflect_index against numpy.pad(mode='reflect'), and the numpy gather / stitch restatement the GPU tests use."""
import numpy as np
import pytest

import segment_ref as ref
import tester

VALID_S = list(range(188, 1213, 32))


def check_axis(n, S):
    """One axis: tile_grid's (count, origin) equals the restatement's, the clipped outputs tile [0, n) in order without
    gaps, overlaps or empty tiles, and the grid is centred (overhang before <= overhang after <= before + 1)."""
    So = S - 184
    k, o = tester.tile_grid(n, 2, S)[0::2]
    assert (k, o) == ref.grid_1d(n, So), (n, S)
    assert o <= 0
    end = 0
    for i in range(k):
        a, b = max(o + i * So, 0), min(o + (i + 1) * So, n)
        assert a == end and b > a, (n, S, i)
        end = b
    assert end == n
    before, after = -o, o + k * So - n
    assert 0 <= before <= after <= before + 1, (n, S)


def test_tile_grid_axis_exhaustive():
    """Every extent 2..3000 (H < 92, H = So, H = So + 1 among them) at every valid S up to 1212."""
    for S in VALID_S:
        for n in range(2, 3001):
            check_axis(n, S)


SHAPES = [(2, 2), (2, 3000), (3000, 2), (37, 5), (91, 91), (92, 93), (388, 388), (389, 388), (388, 389), (520, 696),
          (696, 520), (1000, 1000), (1028, 1029), (1500, 1500), (3000, 2999), (4, 4), (5, 4), (36, 68)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_tile_grid_partitions_the_image(H, W):
    """2-D: the clipped output rectangles cover every pixel exactly once; every input window is S x S and centred on its
    (unclipped) output; tile order is row-major over the grid, as tile_windows enumerates it."""
    for S in VALID_S:
        So = S - 184
        ny, nx, oy0, ox0 = tester.tile_grid(H, W, S)
        if ny * nx > 4000:
            continue
        wins, rny, rnx = ref.tile_windows(H, W, S)
        assert (ny, nx) == (rny, rnx)
        cover = np.zeros((H, W), np.int32)
        for t, (r0, c0, oy, ox) in enumerate(wins):
            i, j = divmod(t, nx)
            assert (oy, ox) == (oy0 + i * So, ox0 + j * So)
            assert (r0, c0) == (oy - 92, ox - 92)
            assert (r0 + S) - (oy + So) == oy - r0 == 92 and (c0 + S) - (ox + So) == ox - c0 == 92
            cover[max(oy, 0):max(min(oy + So, H), 0), max(ox, 0):max(min(ox + So, W), 0)] += 1
        assert (cover == 1).all(), (H, W, S)


def test_tile_grid_rejects_sizes_without_output():
    with pytest.raises(ValueError):
        tester.tile_grid(10, 10, 184)


def test_reflect_index_is_numpy_reflect():
    """Pads up to 5x the extent, i.e. repeated reflection with period 2(n-1)."""
    for n in list(range(2, 20)) + [37, 92, 183, 388]:
        p = 5 * n + 3
        want = np.pad(np.arange(n), p, mode="reflect")
        got = np.array([tester.reflect_index(i, n) for i in range(-p, n + p)])
        assert np.array_equal(got, want), n


def test_valid_tile_sizes_and_errors():
    assert [s for s in range(100, 1300) if tester.valid_tile_size(s)] == VALID_S + [1244, 1276]
    for bad, near in ((187, "188"), (189, "188 and 220"), (573, "572 and 604"), (1000, "988 and 1020")):
        with pytest.raises(ValueError, match=near):
            tester._check_tile_size(bad)
    for ok in VALID_S:
        tester._check_tile_size(ok)


def test_auto_tile_size():
    """One tile when it fits under the cap: the smallest valid S whose output covers the image, else the cap."""
    assert tester.auto_tile_size(2, 2) == 188
    assert tester.auto_tile_size(4, 3) == 188 and tester.auto_tile_size(5, 3) == 220
    assert tester.auto_tile_size(300, 300) == 508
    assert tester.auto_tile_size(300, 2) == 508 and tester.auto_tile_size(2, 300) == 508
    for n in range(2, 2000):
        S = tester.auto_tile_size(n, 1, cap=10 ** 6)
        assert tester.valid_tile_size(S) and S - 184 >= n and (S == 188 or S - 32 - 184 < n)
        assert tester.auto_tile_size(n, n) == min(S, tester.TILE_CAP)


def test_numpy_gather_and_stitch_restatement():
    """The restatement's gather uses np.pad; rebuilt from reflect_index it is the same, and cropping each tile's centre
    and stitching it back returns the image (for value-carrying 'logits')."""
    rs = np.random.RandomState(0)
    for (B, H, W, S) in ((1, 2, 2, 188), (2, 37, 5, 188), (1, 50, 300, 220), (1, 400, 390, 572)):
        img = rs.rand(B, H, W).astype(np.float32)
        tl = ref.tiles(img, S)
        ny, nx, oy0, ox0 = tester.tile_grid(H, W, S)
        So = S - 184
        for t in range(B * ny * nx):
            b, r = divmod(t, ny * nx)
            i, j = divmod(r, nx)
            rows = [tester.reflect_index(oy0 + i * So - 92 + y, H) for y in range(S)]
            cols = [tester.reflect_index(ox0 + j * So - 92 + x, W) for x in range(S)]
            assert np.array_equal(tl[t, 0], img[b][np.ix_(rows, cols)])
        centre = tl[:, :, 92:92 + So, 92:92 + So]
        lg = np.concatenate([np.zeros_like(centre), centre], axis=1)            # l1 = value, l0 = 0
        mask, prob = ref.stitch(lg, B, H, W, S)
        assert np.array_equal(ref.stitch_plane(centre[:, 0], B, H, W, S), img)
        assert np.array_equal(mask, (img > 0).astype(np.int64))
        assert np.allclose(prob, 1 / (1 + np.exp(-img.astype(np.float64))), rtol=0, atol=1e-15)
        n = ref.normalise(img)
        assert n.dtype == np.float32 and n.min() == 0 and n.max() == 1
