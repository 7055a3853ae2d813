"""Per-op tests of aux.hip (and loss.hip's unet_eval_masks) through the C ABI: every entry point either side of the hot path against the fp64 references of
tests/aux_ops_ref.py (pinned to scipy and oracle/aux_ref.py, and their inputs shown well-posed, by tests/test_aux_ops_cpu.py)
at small adversarial shapes: H != W, pad != S, odd sizes, more than one block, the grid-stride loops behind the grid caps,
windows and pads longer than the image.  Every pointer handed to the library comes from a guarded.Arena (tests/guarded.py):
inputs are copies with poison around them, outputs are poisoned and exact, scratch has exactly the bytes the *_scratch_bytes
export returns; mem.verify(outputs...) after every call = every element written, every guard intact."""
import ctypes as C

import numpy as np
import pytest
import torch

import aux_ops_ref as ref
import guarded as gd
from gpu_support import hip, put, rejected, still_poison
from oracle import aux_ref

pytestmark = pytest.mark.gpu


# ---- 1. unet_minmax ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 1023, 1024, 1025, 70001])
def test_minmax(hip, n):
    """x.min() / x.max() per image, bit-exact.  A workgroup of 1024 lanes strides over the image: sizes either side of 1024,
    extremes at indices 0, n - 1, 1023 and 1024, an all-negative image (a maximum that starts from 0 would win) and a
    constant one (lo == hi).  NaN input is out of contract: fminf / fmaxf drop a NaN, numpy propagates it; not tested."""
    L = hip.lib()
    rs = np.random.RandomState(n)
    x = rs.randn(3, n).astype(np.float32)
    at = lambda i: min(i, n - 1)
    x[0, at(0)] = -50.0; x[0, n - 1] = 60.0 if n > 1 else -50.0
    x[1, at(1023)] = 70.0
    if n > 1024:
        x[1, 1024] = -80.0
    x[2] = -np.abs(x[2]) - 1.0                                  # all negative
    for data in (x, np.full((3, n), -2.5, np.float32)):
        mem = gd.Arena()
        out = mem.out((3, 2), torch.float32, "minmax")
        hip.check(L.unet_minmax(mem.ptr(put(mem, data, "x")), 3, n, mem.ptr(out), hip.stream()))
        mem.verify(out)
        assert np.array_equal(out.cpu().numpy(), np.stack([data.min(1), data.max(1)], axis=1))


# ---- 2. unet_mirror_pad -----------------------------------------------------------------------------------------------------
def run_mirror(hip, mem, x, S, minmax=None):
    B, n, _ = x.shape
    out = mem.out((B, S, S), torch.float32, "mirrored")
    mm = None if minmax is None else put(mem, minmax, "minmax")
    rc = hip.lib().unet_mirror_pad(mem.ptr(put(mem, x, "x")), B, n, S, mem.ptr(mm), mem.ptr(out), hip.stream())
    return rc, out


@pytest.mark.parametrize("n,S", ref.MIRROR_CASES)
def test_mirror_pad(hip, n, S):
    """aux_ref.mirror_index on both axes of an index-encoding image, bit-exact; with minmax, (v - lo) / (hi - lo) as fp32 numpy
    evaluates it, bit-exact (the subtraction and the division are correctly rounded on both sides)."""
    x = ref.index_image(3, n)
    mem = gd.Arena()
    rc, out = run_mirror(hip, mem, x, S)
    hip.check(rc)
    mem.verify(out)
    assert np.array_equal(out.cpu().numpy(), ref.mirror_pad(x, S))
    mm = np.stack([x.reshape(3, -1).min(1), x.reshape(3, -1).max(1)], axis=1) + np.float32([[0.0, 0.0], [-3.0, 7.0], [0.5, 0.0]])
    mem = gd.Arena()
    rc, out = run_mirror(hip, mem, x, S, mm.astype(np.float32))
    hip.check(rc)
    mem.verify(out)
    assert np.array_equal(out.cpu().numpy(), ref.mirror_pad(x, S, mm.astype(np.float32)))


def test_mirror_pad_grid_stride(hip):
    B, n, S = ref.MIRROR_BIG                                   # more elements than 16384 blocks x 256 lanes
    x = ref.index_image(B, n)
    mem = gd.Arena()
    rc, out = run_mirror(hip, mem, x, S)
    hip.check(rc)
    mem.verify(out)
    assert np.array_equal(out.cpu().numpy(), ref.mirror_pad(x, S))


def test_mirror_pad_rejects_and_constant_image(hip):
    for n, S in ((5, 12), (5, 15), (6, 5)):                    # S - n odd, P = n (one more than the mirror has), S < n
        mem = gd.Arena()
        rc, out = run_mirror(hip, mem, ref.index_image(3, n), S)
        rejected(hip, rc, mem, out)
    # a constant image normalises to 0/0: NaN, as in numpy.  A NaN is what assert_written looks for, so this one case checks
    # the guards only (verify without outputs) and that the NaN is not the poison pattern.
    x = ref.index_image(3, 5); x[1] = 4.0
    mm = np.stack([x.reshape(3, -1).min(1), x.reshape(3, -1).max(1)], axis=1)
    mem = gd.Arena()
    rc, out = run_mirror(hip, mem, x, 13, mm)
    hip.check(rc)
    mem.verify()
    got = out.cpu().numpy()
    assert np.array_equal(got, ref.mirror_pad(x, 13, mm), equal_nan=True) and np.isnan(got[1]).all() and not np.isnan(got[[0, 2]]).any()


# ---- 3. unet_eval_masks -----------------------------------------------------------------------------------------------------
def eval_case(n, pad, B=3):
    """(big [B,2,Hb,Wb], byte offset of the [n+2pad]^2 view inside it, strides, crop logits [B,2,n,n], labels [B,n,n]).
    Outside the n x n crop window plane 1 is 1e30 and plane 0 is -1e30: a read one pixel off changes the mask."""
    rs = np.random.RandomState(10 * n + pad)
    e = n + 2 * pad
    Hb, Wb = e + 3, e + 5
    big = np.empty((B, 2, Hb, Wb), np.float32); big[:, 0] = -1e30; big[:, 1] = 1e30
    lg = rs.randn(B, 2, n, n).astype(np.float32)
    flat = lg.reshape(B, 2, -1)
    k = n * n
    for b in range(B):                                         # planted ties -> class 0
        flat[b, 1, (0 + b) % k] = flat[b, 0, (0 + b) % k]
        flat[b, 0, (k - 1 - b) % k] = -0.0; flat[b, 1, (k - 1 - b) % k] = 0.0
        flat[b, 0, (k // 2 + b) % k] = 0.0; flat[b, 1, (k // 2 + b) % k] = -0.0
    big[:, :, 1 + pad:1 + pad + n, 2 + pad:2 + pad + n] = lg
    labels = rs.choice([0, 1, 3], (B, n, n)).astype(np.int64)
    return big, (1 * Wb + 2) * 4, (2 * Hb * Wb, Hb * Wb, Wb), lg, labels


@pytest.mark.parametrize("n,pad", [(1, 0), (7, 3), (65, 0), (259, 2)])
def test_eval_masks(hip, n, pad):
    """Crop + argmax + IoU / pixel-error counts, bit-exact against argmax of the crop and aux_ref.eval_counts; labels from
    {0, 1, 3} (the counts use != 0 and |pr - lb|).  259^2 pixels exceed 256 blocks x 256 lanes: grid-stride loop, partial waves."""
    L = hip.lib()
    B = 3
    big, off, (bs, ps, rs_), lg, labels = eval_case(n, pad)
    want = np.argmax(lg, axis=1).astype(np.int64)
    assert (want == 0).any() or n == 1
    mem = gd.Arena()
    bigd = put(mem, big, "logits")
    view = C.c_void_p(mem.address(bigd) + off)
    lab = put(mem, labels, "labels")
    mask = mem.out((B, n, n), torch.int64, "mask"); stats = mem.out((B, 3), torch.int64, "stats")
    for rep in range(2):                                       # the memset of stats is part of the call: same result twice
        hip.check(L.unet_eval_masks(view, bs, ps, rs_, pad, mem.ptr(lab), mem.ptr(mask), B, n, mem.ptr(stats), hip.stream()))
        mem.verify(mask, stats)
        assert np.array_equal(mask.cpu().numpy(), want)
        for b in range(B):
            assert tuple(stats[b].tolist()) == aux_ref.eval_counts(want[b], labels[b]), (rep, b)
    # labels = NULL, stats = NULL: the mask and nothing else
    mask2 = mem.out((B, n, n), torch.int64, "mask (alone)"); untouched = mem.out((B, 3), torch.int64, "stats (not passed)")
    hip.check(L.unet_eval_masks(view, bs, ps, rs_, pad, None, mem.ptr(mask2), B, n, None, hip.stream()))
    mem.verify(mask2)
    assert np.array_equal(mask2.cpu().numpy(), want) and still_poison(untouched)
    # labels without stats: rejected
    mask3 = mem.out((B, n, n), torch.int64, "mask (rejected)")
    rejected(hip, L.unet_eval_masks(view, bs, ps, rs_, pad, mem.ptr(lab), mem.ptr(mask3), B, n, None, hip.stream()), mem, mask3)


# ---- 4. unet_class_balance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 2), (7, 300), (259, 259)])
def test_class_balance(hip, H, W):
    """aux_ref.class_balance per image, bit-exact; counts = the number of ones.  Labels other than {0, 1} are out of contract
    (the kernel counts != 0, the reference counts the second unique value)."""
    L = hip.lib()
    rs = np.random.RandomState(H)
    lab = np.zeros((3, H * W), np.int64)
    lab[0, rs.randint(H * W)] = 1                                # exactly one 1
    lab[1] = 1; lab[1, rs.randint(H * W)] = 0                    # exactly one 0
    lab[2] = rs.rand(H * W) < 0.3
    lab[2, 0] = 0; lab[2, -1] = 1
    lab = lab.reshape(3, H, W)
    mem = gd.Arena()
    w = mem.out((3, H, W), torch.float32, "weights"); cnt = mem.out((3,), torch.int64, "counts")
    hip.check(L.unet_class_balance(mem.ptr(put(mem, lab, "labels")), 3, H, W, mem.ptr(w), mem.ptr(cnt), hip.stream()))
    mem.verify(w, cnt)
    assert cnt.tolist() == [int(l.sum()) for l in lab]
    assert np.array_equal(w.cpu().numpy(), np.stack([aux_ref.class_balance(l) for l in lab]))


def test_class_balance_one_class(hip):
    import functions
    L = hip.lib()
    H, W = 7, 300
    lab = np.zeros((2, H, W), np.int64); lab[1] = 1
    mem = gd.Arena()
    w = mem.out((2, H, W), torch.float32, "weights"); cnt = mem.out((2,), torch.int64, "counts")
    labd = put(mem, lab, "labels")
    hip.check(L.unet_class_balance(mem.ptr(labd), 2, H, W, mem.ptr(w), mem.ptr(cnt), hip.stream()))
    mem.verify(w, cnt)
    assert cnt.tolist() == [0, H * W]
    got = w.cpu().numpy()
    assert np.all(got[0] == 0.0) and np.all(got[1] == 1.0)
    for b in range(2):                                          # the wrapper raises like the reference's counts[1]
        with pytest.raises(IndexError):
            functions.class_balance(labd[b:b + 1])


# ---- 5. unet_gaussian_filter ------------------------------------------------------------------------------------------------
def run_gauss(hip, H, W, sigma, scale, B=3):
    f = ref.gaussian_field(7, B, H, W)
    taps, r = ref.gaussian_taps32(sigma)
    mem = gd.Arena()
    tmp = mem.scratch(B * H * W * 4, "tmp"); out = mem.out((B, H, W), torch.float32, "smoothed")
    hip.check(hip.lib().unet_gaussian_filter(mem.ptr(put(mem, f, "field")), B, H, W, mem.ptr(put(mem, taps, "taps")), r, scale,
                                             mem.ptr(tmp), mem.ptr(out), hip.stream()))
    mem.verify(out)
    err = np.abs(out.cpu().numpy() - ref.gaussian_filter(f, taps, r, scale)).max()
    bound = ref.gaussian_bound(f, taps, r, scale)
    print("gaussian %dx%d sigma %g scale %g: max err %.3g, bound %.3g" % (H, W, sigma, scale, err, bound))
    assert err <= bound


@pytest.mark.parametrize("scale", [1.0, 7.0])
@pytest.mark.parametrize("H,W,sigma", ref.GAUSS_CASES)
def test_gaussian_filter(hip, H, W, sigma, scale):
    """The two zero-extended correlations in fp64 with the same fp32 taps, times scale.  Bound (aux_ops_ref.gaussian_bound):
    each pass is a chain of at most m = 2 r + 1 fmaf, one rounding (u = 2^-24) of a partial sum <= A = max|field| sum|w| each;
    pass 2 also carries pass 1's error through sum|w| ~ 1; the final multiply by scale rounds once: (2 m + 1) u A scale to first
    order, taken as gamma_(4r+4) A scale.  Windows wider than the image (r = 12 > H, > W; r = 40 = W) and r = 0 included."""
    run_gauss(hip, H, W, sigma, scale)


def test_gaussian_filter_grid_stride(hip):
    H, W, sigma = ref.GAUSS_BIG                                # 3 H W > 16384 blocks x 256 lanes
    run_gauss(hip, H, W, sigma, 7.0)


# ---- 6. unet_warp_bilinear --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", ref.WARP_CASES)
def test_warp_bilinear(hip, H, W):
    """scipy.ndimage.map_coordinates(order=1, mode='constant') in fp64.  The displacements are multiples of 1/8, so both sides
    form the same coordinates: outside pixels are exactly 0, inside ones within 4 x 2^-23 max|img| (five roundings of the
    kernel's expression; fy, fx and their complements are exact).  H != W, extents of 1 and 2 (the H - 2 < 0 clamp), planted
    coordinates 0, H - 1, -1/8, H - 1 + 1/8; image and fields are asymmetric (the CPU test shows that swapping dy and dx moves
    the result by more than 1000 bounds)."""
    img, dy, dx = ref.warp_case(H, W)
    B = img.shape[0]
    mem = gd.Arena()
    out = mem.out((B, H, W), torch.float32, "warped")
    hip.check(hip.lib().unet_warp_bilinear(mem.ptr(put(mem, img, "img")), mem.ptr(put(mem, dy, "dy")), mem.ptr(put(mem, dx, "dx")),
                                           B, H, W, mem.ptr(out), hip.stream()))
    mem.verify(out)
    got = out.cpu().numpy()
    want = ref.warp_bilinear(img, dy, dx)
    outside = ref.warp_outside(dy, dx)
    assert np.all(got[outside] == 0.0)
    err = np.abs(got - want)[~outside].max()
    print("warp %dx%d: max err %.3g, bound %.3g, %.0f %% outside" % (H, W, err, ref.warp_bound(img), 100 * outside.mean()))
    assert err <= ref.warp_bound(img)


# ---- 7. unet_reflect_rotate_crop ---------------------------------------------------------------------------------------------
def run_rotate(hip, mem, img, pad, S, angles, levels, scratch_B=None):
    """img fp32 [B,n,n] -> (rc, out [B,S,S]); scratch is exactly unet_rotate_scratch_bytes(B, S)."""
    L = hip.lib()
    B, n, _ = img.shape
    out = mem.out((B, S, S), torch.float32, "rotated")
    sc = mem.scratch(L.unet_rotate_scratch_bytes(B, S), "rotate scratch")
    ang = (C.c_float * B)(*[float(a) for a in angles])
    rc = L.unet_reflect_rotate_crop(mem.ptr(put(mem, img, "img")), B, n, pad, S, ang, levels, mem.ptr(out), mem.ptr(sc), hip.stream())
    return rc, out


def rotate_ref(img, pad, S, angles):
    return np.stack([ref.reflect_rotate_crop(im, float(np.float32(a)), pad, S) for im, a in zip(img, angles)])


@pytest.mark.parametrize("case", range(len(ref.ROT_CASES)))
def test_reflect_rotate_crop_float(hip, case):
    """levels = 0 against np.pad(reflect) + scipy.ndimage.rotate in fp64 + centre crop, <= 2e-5 of the value range (the
    project's figure for the fp32 prefilter and weights).  pad != S, a padded extent equal to the sampled region, a pad of 20
    image lengths, odd and even extents, angles off the 30-degree table; grey images and the high-contrast block images."""
    n, pad, S, deg = ref.ROT_CASES[case]
    imgs = [ref.float_images(n, case)]
    if deg != 90.0:
        imgs.append(ref.block_images(n, 255, ref.rotate_seed(case, 255)))
    for img in imgs:
        mem = gd.Arena()
        rc, out = run_rotate(hip, mem, img, pad, S, [deg] * len(img), 0)
        hip.check(rc)
        mem.verify(out)
        err = np.abs(out.cpu().numpy() - rotate_ref(img, pad, S, [deg] * len(img))).max() / 255.0
        print("rotate case %d (n %d pad %d S %d, %g deg), float: max err %.3g of the value range" % (case, n, pad, S, deg, err))
        assert err < ref.ROT_TOL


@pytest.mark.parametrize("levels", [255, 65535])
@pytest.mark.parametrize("case", range(6))
def test_reflect_rotate_crop_levels_exact(hip, case, levels):
    """Integer modes compare exactly, no '1 level off' allowance: the block images come from seeds for which every fp64 value
    before rounding is at least 2e-5 x levels away from every k + 0.5 and for which both clamps run
    (tests/test_aux_ops_cpu.py::test_rotate_integer_cases_are_well_posed)."""
    n, pad, S, deg = ref.ROT_CASES[case]
    img = ref.block_images(n, levels, ref.rotate_seed(case, levels))
    mem = gd.Arena()
    rc, out = run_rotate(hip, mem, img, pad, S, [deg] * len(img), levels)
    hip.check(rc)
    mem.verify(out)
    want = ref.to_levels(rotate_ref(img, pad, S, [deg] * len(img)), levels)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), (np.abs(got - want).max(), (got != want).sum())


def test_reflect_rotate_crop_90_degrees_exact(hip):
    """A multiple of 90 degrees permutes the pixels: integer images come back exactly at 255 and 65535 levels, and within the
    float tolerance at levels = 0 (the fp32 prefilter followed by the spline's 1/6, 4/6, 1/6 is the identity only to rounding)."""
    n, pad, S, deg = ref.ROT_CASES[6]
    img = ref.integer_images(n, 0)
    want = rotate_ref(img, pad, S, [deg] * len(img))
    for levels in (255, 65535, 0):
        mem = gd.Arena()
        rc, out = run_rotate(hip, mem, img, pad, S, [deg] * len(img), levels)
        hip.check(rc)
        mem.verify(out)
        if levels:
            assert np.array_equal(out.cpu().numpy(), np.round(want))
        else:
            assert np.abs(out.cpu().numpy() - want).max() < ref.ROT_TOL * 255


def test_reflect_rotate_crop_batch_of_64_and_rejects(hip):
    n, pad, S = ref.ROT_BATCH64
    rs = np.random.RandomState(64)
    img = (rs.rand(64, n, n) * 255).astype(np.float32)
    angles = [-171.3 + 8.37 * i for i in range(64)]            # 64 distinct angles, -171 .. 356
    mem = gd.Arena()
    rc, out = run_rotate(hip, mem, img, pad, S, angles, 0)
    hip.check(rc)
    mem.verify(out)
    assert np.abs(out.cpu().numpy() - rotate_ref(img, pad, S, angles)).max() < ref.ROT_TOL * 255
    # rejected without writing: B = 65, odd S, a padded image smaller than the sampled region (N = 76 < 78), levels = 7
    one = img[:1]
    for im, p, s, lv in ((np.concatenate([img, one]), pad, S, 0), (one, pad, 7, 0), (one, pad - 1, S, 0), (one, pad, S, 7)):
        mem = gd.Arena()
        rc, out = run_rotate(hip, mem, im, p, s, [30.0] * len(im), lv)
        rejected(hip, rc, mem, out)


# ---- 8. data.elastic_transform with H != W ----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(40, 56), (56, 40)])
def test_elastic_transform_rectangular(hip, H, W):
    """Through the wrapper with explicit fields against aux_ref.elastic_transform, at the tolerance of
    test_elastic_transform_vs_reference_golden (2e-5 of the 0 .. 255 range)."""
    import data
    rs = np.random.RandomState(H)
    img = rs.rand(H, W) * 255.0
    tgt = (rs.rand(H, W) > 0.5) * 255.0
    f0, f1 = rs.rand(H, W), rs.rand(H, W)
    alpha, sigma = 30.0, 4.0
    a, b = data.elastic_transform((torch.from_numpy(img).float().cuda(), torch.from_numpy(tgt).float().cuda()), alpha=alpha, sigma=sigma,
                                  fields=(f0, f1))
    (ra, rb), _, _ = aux_ref.elastic_transform((img.astype(np.float32).astype(np.float64), tgt), alpha, sigma, (f0, f1))
    assert a.shape == (H, W) and b.shape == (H, W)
    ea, eb = np.abs(a.cpu().numpy() - ra).max(), np.abs(b.cpu().numpy() - rb).max()
    print("elastic %dx%d: max err %.3g / %.3g (tolerance %.3g)" % (H, W, ea, eb, 255 * 2e-5))
    assert ea < 255 * 2e-5 and eb < 255 * 2e-5
