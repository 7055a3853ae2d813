"""Pins tests/aux_ops_ref.py (the fp64 references and fixed inputs of tests/test_aux_ops_gpu.py) to scipy and to
oracle/aux_ref.py, and asserts the conditions that make every GPU comparison well-posed.  No GPU, no library."""
import numpy as np
import pytest
from scipy import ndimage

import aux_ops_ref as ref
from oracle import aux_ref


def test_mirror_pad_reference():
    for n, S in ref.MIRROR_CASES + [ref.MIRROR_BIG[1:]]:
        P = (S - n) // 2
        x = ref.index_image(3, n)
        assert np.array_equal(x[0], (1000.0 * np.arange(n)[:, None] + np.arange(n)[None, :]))     # exact in fp32
        out = ref.mirror_pad(x, S)
        assert out.shape == (3, S, S) and np.array_equal(out[:, P:P + n, P:P + n], x)
        for Y in range(S):                                   # the asymmetric rule, spelled out
            src = P - Y if Y < P else (Y - P if Y < P + n else n - 1 - (Y - n - P))
            assert np.array_equal(out[:, Y, P:P + n], x[:, src]) and np.array_equal(out[:, P:P + n, Y], x[:, :, src])
        mm = np.stack([x.reshape(3, -1).min(1), x.reshape(3, -1).max(1)], axis=1)
        nrm = ref.mirror_pad(x, S, mm)
        assert nrm.dtype == np.float32 and nrm.min() == 0.0 and nrm.max() == 1.0
    # the reference's own sizes: the same as aux_ref.mirror_transform
    img = np.random.RandomState(0).rand(196, 196).astype(np.float32)
    assert np.array_equal(ref.mirror_pad(img[None], aux_ref.input_size_compute(196)[1])[0], aux_ref.mirror_transform(img))
    assert [(S - n) // 2 for n, S in ref.MIRROR_CASES] == [0, 4, 1, 12] and ref.MIRROR_CASES[1][0] - 1 == 4       # P = 0 and P = n - 1
    for n, S in ((5, 12), (5, 15), (6, 5)):                  # S - n odd, P = n, S < n
        with pytest.raises(ValueError):
            aux_ref.mirror_index(S, n)
    B, n, S = ref.MIRROR_BIG
    assert B * S * S > 16384 * 256
    const = np.full((1, 5, 5), 3.0, np.float32)              # a constant image normalises to 0/0
    assert np.isnan(ref.mirror_pad(const, 13, np.array([[3.0, 3.0]], np.float32))).all()


@pytest.mark.parametrize("H,W,sigma", ref.GAUSS_CASES)
def test_gaussian_reference_vs_scipy(H, W, sigma):
    """Reference and fp32 taps against scipy.ndimage.gaussian_filter(mode='constant'): what separates them is the taps'
    rounding to fp32, <= (2r+1) 2^-24 on a field in [-1, 1) per pass (measured <= 7e-9)."""
    f = ref.gaussian_field(5, 3, H, W)
    w, r = ref.gaussian_taps32(sigma)
    assert r == int(4.0 * sigma + 0.5) and len(w) == 2 * r + 1 and w.dtype == np.float32
    assert np.abs(f).max() <= 1.0 and not np.array_equal(f[0], f[1])
    for scale in (1.0, 7.0):
        got = ref.gaussian_filter(f, w, r, scale)
        sp = np.stack([ndimage.gaussian_filter(x.astype(np.float64), sigma, mode="constant", cval=0.0) for x in f]) * scale
        assert np.abs(got - sp).max() <= 6e-8 * scale
        b = ref.gaussian_bound(f, w, r, scale)
        assert (4 * r + 3) * 2.0 ** -24 * scale * np.abs(f).max() * 0.99 < b < (4 * r + 4) * 2.0 ** -24 * scale * 1.001


def test_gaussian_cases_cover_the_edges():
    rad = [ref.gaussian_taps32(s)[1] for _, _, s in ref.GAUSS_CASES]
    (H0, W0, _), (H1, W1, _), _, (H3, W3, _) = ref.GAUSS_CASES
    assert rad == [12, 12, 0, 40] and rad[0] > H0 and rad[1] > W1 and rad[3] == W3 and H0 != W0 and H3 != W3
    H, W, _ = ref.GAUSS_BIG
    assert 3 * H * W > 16384 * 256 and H != W


@pytest.mark.parametrize("H,W", ref.WARP_CASES)
def test_warp_reference_and_inputs(H, W):
    img, dy, dx = ref.warp_case(H, W)
    assert img.dtype == dy.dtype == dx.dtype == np.float32 and img.shape == (ref.WARP_B, H, W)
    for d in (dy, dx):                                        # multiples of 1/8 in [-3, 3]
        assert np.array_equal(d * 8, np.round(d * 8)) and np.abs(d).max() <= 3.0
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = ref.warp_coords(dy, dx)                         # fp32 forms the same coordinate exactly
    assert np.array_equal((yy.astype(np.float32) + dy).astype(np.float64), cy)
    assert np.array_equal((xx.astype(np.float32) + dx).astype(np.float64), cx)
    out = ref.warp_outside(dy, dx)
    want = ref.warp_bilinear(img, dy, dx)
    assert np.all(want[out] == 0.0)
    assert np.abs(want - ref.warp_bilinear_numpy(img, dy, dx)).max() <= 1e-12 * np.abs(img).max()      # scipy, degenerate shapes included
    # planted coordinates
    assert cy[0, 0, 0] == 0 and cx[0, 0, 0] == 0 and want[0, 0, 0] == img[0, 0, 0]
    assert cy[0, -1, -1] == H - 1 and cx[0, -1, -1] == W - 1 and not out[0, -1, -1] and want[0, -1, -1] == img[0, -1, -1]
    if W >= 5:
        assert cy[0, 0, 1] == -0.125 and out[0, 0, 1] and cy[0, H - 1, 2] == H - 1 + 0.125 and out[0, H - 1, 2]
        assert not out[0, H - 1, W - 2] and want[0, H - 1, W - 2] == 0.5 * (float(img[0, H - 1, W - 2]) + float(img[0, H - 1, W - 1]))
    if H >= 5:
        assert cx[0, 1, 0] == -0.125 and out[0, 1, 0] and cx[0, 2, W - 1] == W - 1 + 0.125 and out[0, 2, W - 1]
        assert not out[0, H - 2, W - 1] and want[0, H - 2, W - 1] == 0.5 * (float(img[0, H - 2, W - 1]) + float(img[0, H - 1, W - 1]))
    if H * W > 100:
        assert 0.10 <= out.mean() <= 0.50                    # enough pixels on either side of the border
        # asymmetric image, different fields: swapping dy and dx, or transposing, changes the result far beyond the bound
        assert np.abs(ref.warp_bilinear(img, dx, dy) - want).max() > 1000 * ref.warp_bound(img)
        assert not np.array_equal(dy, dx) and not np.array_equal(dy[0], dy[1])


def test_rotate_reference_is_the_oracle_with_pad_as_parameter():
    img = (np.random.RandomState(0).rand(36, 36) * 255).astype(np.uint8)
    S = aux_ref.input_size_compute(36)[1]
    for deg in (0, 30, 77.5):
        assert np.array_equal(ref.reflect_rotate_crop(img, deg, S, S), aux_ref.reflect_rotate_crop(img.astype(np.float64), deg))
        assert np.array_equal(ref.to_levels(ref.reflect_rotate_crop(img, deg, S, S), 255), aux_ref.reflect_rotate_crop(img, deg))
    # the shapes cover what they are there for (rot_region_w(S) = 2 (ceil(0.70711 S) + 32) + 2)
    W = {S: 2 * (int(np.ceil(S * 0.70711)) + 32) + 2 for S in (4, 6, 8)}
    N = [n + 2 * pad for n, pad, _, _ in ref.ROT_CASES]
    assert W == {4: 72, 6: 76, 8: 78} and all(Ni >= W[c[2]] for Ni, c in zip(N, ref.ROT_CASES))
    assert N[0] == W[8] and N[5] == W[6]                                     # padded extent = sampled region
    assert any(pad > n - 1 for n, pad, _, _ in ref.ROT_CASES) and ref.ROT_CASES[4][1] > 10 * ref.ROT_CASES[4][0]
    assert {Ni % 2 for Ni in N} == {0, 1}
    assert sum(deg % 30 != 0 for _, _, _, deg in ref.ROT_CASES) >= 4 and ref.ROT_CASES[6][3] == 90.0


def test_rotate_by_90_degrees_is_a_permutation():
    n, pad, S, deg = ref.ROT_CASES[6]
    for im in ref.integer_images(n, 0):
        t = ref.reflect_rotate_crop(im, deg, pad, S)
        p = np.rot90(np.pad(im.astype(np.float64), pad, mode="reflect"))
        c = p.shape[0] // 2 - S // 2
        assert np.abs(t - p[c:c + S, c:c + S]).max() < 1e-9                # integers: 0.5 from every boundary, at any level count
        assert np.array_equal(ref.to_levels(t, 255), p[c:c + S, c:c + S]) and np.array_equal(ref.to_levels(t, 65535), p[c:c + S, c:c + S])


@pytest.mark.parametrize("levels", [255, 65535])
@pytest.mark.parametrize("case", range(6))
def test_rotate_integer_cases_are_well_posed(case, levels):
    """The seeds rotate_seed() picks: every fp64 value before rounding is at least 2e-5 x levels (more for an image whose value
    range exceeds the level count) away from every k + 0.5, and both clamps run."""
    n, pad, S, deg = ref.ROT_CASES[case]
    seed = ref.rotate_seed(case, levels)
    assert seed is not None
    img = ref.block_images(n, levels, seed)
    t = np.stack([ref.reflect_rotate_crop(im, deg, pad, S) for im in img])
    m = ref.level_margin(img, levels)
    assert m >= 2e-5 * levels
    assert ref.half_level_distance(t, levels).min() >= m
    if ref.clamps_expected(case, levels):
        assert (t > levels + 0.5).any() and (t < 0).any()
    q = ref.to_levels(t, levels)
    assert q.min() == 0 and q.max() <= levels and len(np.unique(q)) >= 2
    if levels == 255 and n >= 8:
        assert len(np.unique(q)) > 4                          # edge pixels take values strictly between the two levels
    # half_level_distance itself, against the definition
    k = np.arange(levels)[:, None] + 0.5
    assert np.allclose(np.abs(t.reshape(1, -1)[:, :16] - k).min(0), ref.half_level_distance(t, levels).reshape(-1)[:16], rtol=0, atol=1e-6 * m)


def test_eval_counts_and_class_balance_references():
    rs = np.random.RandomState(4)
    pred = rs.randint(0, 2, (7, 7)); lab = rs.choice([0, 1, 3], (7, 7))
    i, u, d = aux_ref.eval_counts(pred, lab)
    assert i == ((pred != 0) & (lab != 0)).sum() and u == ((pred != 0) | (lab != 0)).sum() and d == np.abs(pred - lab).sum()
    assert d > u - i                                          # a label of 3 counts 2 or 3 in |pr - lb|
    gt = np.zeros((1, 2), np.int64); gt[0, 1] = 1
    assert np.array_equal(aux_ref.class_balance(gt), np.ones((1, 2), np.float32))
    gt = np.ones((7, 300), np.int64); gt[3, 17] = 0          # exactly one 0
    w = aux_ref.class_balance(gt)
    assert w[3, 17] == np.float32(2099.0) and (w == 1).sum() == 2099
    for one_class in (np.zeros((3, 3), np.int64), np.ones((3, 3), np.int64)):
        with pytest.raises(IndexError):
            aux_ref.class_balance(one_class)
