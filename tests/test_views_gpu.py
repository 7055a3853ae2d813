"""Dihedral views on the device: unet_tile_gather_view against unet_tile_gather on the materialised view, unet_tile_stitch_view
against the per-view probabilities of unet_tile_stitch / unet_tile_stitch_k summed in numpy, and tester.segment(views=...) against
the composite of per-view segment() calls - all bit for bit.  Every raw pointer is a tests/guarded.Arena buffer."""
import ctypes

import numpy as np
import pytest
import torch

import guarded
from gpu_support import dev, image, math_mode, net

pytestmark = pytest.mark.gpu

D4 = (0, 1, 2, 3, 4, 5, 6, 7)
VIEW_LISTS = [(0,), (5,), (1, 6), D4, D4[::-1]]
FIRST, LAST = 1, 2


@pytest.fixture(scope="module")
def net3(dev):
    import multiclass_ref
    import network
    m = network.Unet(n_classes=3)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in multiclass_ref.head_params(3).items()})
    return m.to(dev)


def view_grid(H, W, S, v):
    import tester
    Hv, Wv = tester.view_shape(H, W, v)
    return (Hv, Wv) + tester.tile_grid(Hv, Wv, S)


# ---- gather_view ------------------------------------------------------------------------------------------------------------

def gather_pair(ar, dev, x, mm, S, v, t0=None, nt=None, shift=0):
    """(unet_tile_gather_view of x, unet_tile_gather of the contiguous view) for tiles [t0, t0+nt) of view v; shift: floats the
    output pointer of gather_view is moved by (the buffer is that much longer)."""
    import _hip
    import tester
    B, H, W = x.shape
    Hv, Wv, ny, nx, oy0, ox0 = view_grid(H, W, S, v)
    if t0 is None:
        t0, nt = 0, B * ny * nx
    xv = ar.inp(tester.apply_view(x, v).contiguous())
    assert xv.shape == (B, Hv, Wv)
    want = ar.out((nt, 1, S, S))
    _hip.run("unet_tile_gather", dev, ar.ptr(xv), B, Hv, Wv, ar.ptr(mm), S, oy0, ox0, ny, nx, t0, nt, ar.ptr(want))
    buf = ar.out(nt * S * S + shift)
    p = ctypes.c_void_p(ar.address(buf) + 4 * shift)
    _hip.run("unet_tile_gather_view", dev, ar.ptr(x), B, H, W, ar.ptr(mm), S, v, oy0, ox0, ny, nx, t0, nt, p)
    ar.verify(want)
    assert bool(torch.isnan(buf[:shift]).all())                     # the floats before a shifted pointer are still poison
    return buf[shift:].view(nt, 1, S, S), want


@pytest.mark.parametrize("B,H,W,S", [(1, 2, 2, 188), (1, 37, 5, 188), (2, 9, 14, 188), (1, 50, 75, 220), (1, 300, 200, 572)])
def test_gather_view_is_gather_of_the_materialised_view(dev, B, H, W, S):
    """All 8 codes, raw and normalised, bit for bit; 188 = 5 x 32 + 28 leaves a partial block on each axis of a transposed
    view's 32 x 32 moves, 9 x 14 overhangs its 3 x 4 grid on both axes, 2 x 2 and 37 x 5 reflect several times."""
    import _hip
    ar = guarded.Arena(dev)
    x = ar.inp(torch.from_numpy(image(H * W + B, B, H, W, blobs=8)))
    mm = ar.out((B, 2))
    _hip.run("unet_minmax", dev, ar.ptr(x), B, H * W, ar.ptr(mm))
    for v in D4:
        for m in (None, mm):
            got, want = gather_pair(ar, dev, x, m, S, v)
            assert torch.equal(got, want), (v, m is not None)
        assert m is mm and float(want.min()) >= 0.0 and float(want.max()) <= 1.0
    ar.check()


def test_gather_view_of_a_sub_range_and_through_a_4_byte_aligned_pointer(dev):
    """Tiles [5, 18) of the 24 of each view start and end inside the view and cross from image 0 to image 1; an output pointer
    that is only 4-byte aligned takes the scalar store path of the untransposed views."""
    import _hip
    ar = guarded.Arena(dev)
    B, H, W, S = 2, 9, 14, 188
    x = ar.inp(torch.from_numpy(image(77, B, H, W, blobs=8)))
    mm = ar.out((B, 2))
    _hip.run("unet_minmax", dev, ar.ptr(x), B, H * W, ar.ptr(mm))
    for v in D4:
        got, want = gather_pair(ar, dev, x, mm, S, v, t0=5, nt=13)
        assert torch.equal(got, want), v
        got, want = gather_pair(ar, dev, x, None, S, v, t0=5, nt=13, shift=1)
        assert torch.equal(got, want), v
    ar.check()


# ---- stitch_view ------------------------------------------------------------------------------------------------------------

def synthetic_logits(seed, T, K, So):
    rs = np.random.RandomState(seed)
    lg = (rs.randn(T, K, So, So) * 4).astype(np.float32)
    tie = rs.rand(T, So, So) < 0.1
    lg[:, 1][tie] = lg[:, 0][tie]                                   # exact ties l0 == l1
    if K > 2:
        top = rs.rand(T, So, So) < 0.05                             # ... some of them at the maximum
        lg[:, 0][top] = lg[:, 1][top] = np.abs(lg).max(axis=1)[top] + 1
    return lg


def per_view_probs(ar, dev, lg, K, B, H, W, S, v):
    """The existing stitch kernels on the view-shaped problem, brought back to the image's frame in numpy."""
    import _hip
    import tester
    Hv, Wv, ny, nx, oy0, ox0 = view_grid(H, W, S, v)
    T = B * ny * nx
    mask = ar.out((B, Hv, Wv), torch.int64)
    prob = ar.out((B, Hv, Wv) if K == 2 else (B, K, Hv, Wv))
    if K == 2:
        _hip.run("unet_tile_stitch", dev, ar.ptr(lg), S - 184, oy0, ox0, ny, nx, 0, T, B, Hv, Wv, ar.ptr(mask), ar.ptr(prob))
    else:
        _hip.run("unet_tile_stitch_k", dev, ar.ptr(lg), S - 184, K, oy0, ox0, ny, nx, 0, T, B, Hv, Wv, ar.ptr(mask), ar.ptr(prob))
    ar.verify(mask, prob)
    return np.ascontiguousarray(tester.undo_view(prob.cpu().numpy(), v))


def restate(probs, vs, K):
    acc = probs[vs[0]].copy()
    for v in vs[1:]:
        acc = acc + probs[v]
    assert acc.dtype == np.float32
    avg = acc / np.float32(len(vs))
    mask = (avg > 0.5).astype(np.int64) if K == 2 else np.argmax(acc, axis=1).astype(np.int64)
    return avg, mask


@pytest.mark.parametrize("B,H,W,S", [(1, 2, 2, 188), (2, 9, 14, 188), (1, 37, 5, 188), (1, 50, 75, 220)])
@pytest.mark.parametrize("K", [2, 3, 16])
def test_stitch_view_sums_the_views_in_stream_order(dev, K, B, H, W, S):
    """prob and mask bit-equal to: per-view probabilities of the existing kernels, undo_view, float32 sum in view order, a true
    division, and > 0.5 / argmax of the sums (ties -> the lowest class).  Each list of views is stitched once with one launch
    per view and once with every view split into two launches at an odd tile index.  prob and mask start as poison (NaN, -1):
    a FIRST launch that added, or a pixel never written, would show; before the LAST view the mask is still poison."""
    import _hip
    import tester
    ar = guarded.Arena(dev)
    So = S - 184
    Tv = B * tester.tile_grid(H, W, S)[0] * tester.tile_grid(H, W, S)[1]
    cut = (Tv // 2) | 1 if Tv > 2 else 0
    lgs = {v: ar.inp(torch.from_numpy(synthetic_logits(1000 * K + 10 * H + v, Tv, K, So))) for v in D4}
    probs = {v: per_view_probs(ar, dev, lgs[v], K, B, H, W, S, v) for v in D4}
    if H * W > 4:
        assert len({probs[v].tobytes() for v in D4}) == 8
        assert K > 2 or (probs[0] == 0.5).any()                     # the planted ties: where > 0.5 and l1 > l0 part ways
    for vs in VIEW_LISTS:
        want_p, want_m = restate(probs, vs, K)
        for split in ((False, True) if cut else (False,)):
            out = guarded.Arena(dev)
            prob = out.out((B, H, W) if K == 2 else (B, K, H, W))
            mask = out.out((B, H, W), torch.int64)
            for n, v in enumerate(vs):
                Hv, Wv, ny, nx, oy0, ox0 = view_grid(H, W, S, v)
                assert B * ny * nx == Tv
                phase = (FIRST if n == 0 else 0) | (LAST if n == len(vs) - 1 else 0)
                for a, b in (((0, cut), (cut, Tv)) if split else ((0, Tv),)):
                    first = ctypes.c_void_p(ar.address(lgs[v]) + a * K * So * So * 4)
                    _hip.run("unet_tile_stitch_view", dev, first, So, K, v, oy0, ox0, ny, nx, a, b - a, B, H, W, phase, len(vs),
                             out.ptr(prob), out.ptr(mask) if phase & LAST else None)
                if not phase & LAST:
                    assert bool((mask == -1).all()), (vs, v)
            out.verify(prob, mask)
            assert np.array_equal(prob.cpu().numpy(), want_p), (vs, split)
            assert np.array_equal(mask.cpu().numpy(), want_m), (vs, split)
    ar.check()


def test_stitch_view_rejects_bad_arguments_without_writing(dev):
    import _hip
    import tester
    L = _hip.lib()
    st = _hip.stream(dev)
    ar = guarded.Arena(dev)
    B, H, W, S, So = 1, 9, 14, 188, 4
    v = 1
    Hv, Wv, ny, nx, oy0, ox0 = view_grid(H, W, S, v)
    assert (Hv, Wv, ny, nx) == (14, 9, 4, 3)
    gy, gx, y0, x0 = tester.tile_grid(H, W, S)                                   # the image's own grid: 3 x 4
    T = ny * nx
    lg = ar.inp(torch.from_numpy(synthetic_logits(5, T, 16, So)))
    prob = ar.out((B, 16, H, W))
    mask = ar.out((B, H, W), torch.int64)
    x = ar.inp(torch.from_numpy(image(9, B, H, W, blobs=8)))
    tiles = ar.out((T, 1, S, S))

    def stitch(K=2, view=v, grid=(oy0, ox0, ny, nx), phase=3, n_views=1, m=mask):
        return L.unet_tile_stitch_view(ar.ptr(lg), So, K, view, grid[0], grid[1], grid[2], grid[3], 0, T, B, H, W, phase, n_views,
                                       ar.ptr(prob), ar.ptr(m), st)

    def gather(view=v, grid=(oy0, ox0, ny, nx), size=S):
        return L.unet_tile_gather_view(ar.ptr(x), B, H, W, None, size, view, grid[0], grid[1], grid[2], grid[3], 0, T, ar.ptr(tiles), st)

    for kw in (dict(view=8), dict(view=-1), dict(grid=(y0, x0, gy, gx)), dict(K=17), dict(K=1), dict(phase=4), dict(phase=-1),
               dict(n_views=0), dict(m=None), dict(m=None, phase=2)):
        assert stitch(**kw) != 0, kw
        assert L.unet_last_error().startswith(b"unet_tile_stitch_view"), kw
    for kw in (dict(view=8), dict(view=-1), dict(grid=(y0, x0, gy, gx)), dict(size=190)):
        assert gather(**kw) != 0, kw
        assert L.unet_last_error().startswith(b"unet_tile_gather_view"), kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(prob).all()) and bool((mask == -1).all()) and bool(torch.isnan(tiles).all())
    ar.check()
    # the same calls with valid arguments
    assert stitch(m=None, phase=1, n_views=2) == 0 and bool((mask == -1).all())
    assert stitch(K=16) == 0 and gather() == 0
    ar.verify(prob, mask, tiles)
    # the image's own grid is the right one for an untransposed view
    assert stitch(view=6, grid=(y0, x0, gy, gx)) == 0 and gather(view=6, grid=(y0, x0, gy, gx)) == 0
    ar.check()


# ---- segment(views=...) -------------------------------------------------------------------------------------------------------

def composite(net, x, vs, S, mb):
    """The hand-made average: one segment() per materialised view, undo_view, float32 sum in order, divide, threshold."""
    import tester
    acc = None
    for v in vs:
        _, p = tester.segment(net, tester.apply_view(x, v).contiguous(), tile_size=S, max_batch=mb, return_probs=True)
        p = np.ascontiguousarray(tester.undo_view(p.cpu().numpy(), v))
        acc = p if acc is None else acc + p
    assert acc.dtype == np.float32
    avg = acc / np.float32(len(vs))
    K = getattr(net, "n_classes", 2)
    return avg, ((avg > 0.5) if K == 2 else np.argmax(acc, axis=1)).astype(np.int64)


def check_against_composite(net, dev, B, H, W, S, views, mb, seed):
    import tester
    x = torch.from_numpy(image(seed, B, H, W, blobs=8)).to(dev)
    want_p, want_m = composite(net, x, tester.parse_views(views), S, mb)
    m, p = tester.segment(net, x, tile_size=S, max_batch=mb, return_probs=True, views=views)
    assert m.dtype == torch.int64 and p.dtype == torch.float32 and m.shape == (B, H, W) and p.shape == want_p.shape
    assert torch.equal(p.cpu(), torch.from_numpy(want_p))
    assert torch.equal(m.cpu(), torch.from_numpy(want_m))
    return want_p, want_m


@pytest.mark.parametrize("B,H,W,S,views,mb", [(1, 4, 8, 188, "d4", 16),        # 16 tiles, one chunk of all 8 views
                                              (2, 9, 14, 188, "rot4", 5),      # chunks straddle views and images
                                              (1, 130, 200, 220, "d4", 3)])
def test_segment_views_is_the_composite_of_per_view_segments(dev, net, B, H, W, S, views, mb):
    """Exact because the fp32 forward of a tile does not depend on the chunk it is in
    (test_segment_gpu.test_chunking_does_not_change_the_result)."""
    check_against_composite(net, dev, B, H, W, S, views, mb, H + W)


def test_segment_views_three_classes(dev, net3):
    want_p, want_m = check_against_composite(net3, dev, 1, 9, 14, 188, "flips", 16, 3)
    assert want_p.shape == (1, 3, 9, 14) and np.abs(want_p.sum(axis=1) - 1).max() < 1e-6


def test_segment_views_bf16_same_chunks(dev, net, math_mode):
    """bf16 tensors: max_batch is one view's 12 tiles, so both sides run the same forwards (a bf16 forward is only known to be
    reproducible for the same chunk)."""
    import tester
    math_mode(2)
    assert tester.tile_grid(9, 14, 188)[:2] == (3, 4)
    check_against_composite(net, dev, 1, 9, 14, 188, "rot4", 12, 8)


def test_identity_view_is_the_plain_path(dev, net):
    import tester
    x = torch.from_numpy(image(12, 2, 40, 30, blobs=8)).to(dev)
    m0, p0 = tester.segment(net, x, tile_size=220, max_batch=3, return_probs=True)
    m1, p1 = tester.segment(net, x, tile_size=220, max_batch=3, return_probs=True, views=(0,))
    assert torch.equal(p0, p1)
    off = p0 != 0.5
    assert torch.equal(m0[off], m1[off]) and bool((m1[~off] == 0).all())


def test_determinism_side_stream_instances_and_shapes(dev, net, net3):
    import tester
    from functions import label_cells
    x = torch.from_numpy(image(31, 2, 9, 14, blobs=8)).to(dev)
    kw = dict(tile_size=188, max_batch=5, return_probs=True, views="d4")
    m0, p0 = tester.segment(net, x, **kw)
    m1, p1 = tester.segment(net, x, **kw)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        m2, p2 = tester.segment(net, x, **kw)
    torch.cuda.current_stream(dev).wait_stream(s)
    assert torch.equal(m0, m1) and torch.equal(p0, p1) and torch.equal(m0, m2) and torch.equal(p0, p2)
    m3, p3, inst = tester.segment(net, x, return_instances=True, **kw)
    assert torch.equal(m3, m0) and torch.equal(p3, p0) and torch.equal(inst, label_cells(m0)[0])
    only = tester.segment(net, x, tile_size=188, max_batch=5, views="d4")
    assert torch.is_tensor(only) and torch.equal(only, m0)
    ms, ps = tester.segment(net, x[1], **kw)
    assert ms.shape == (9, 14) and ps.shape == (9, 14) and torch.equal(ms, m0[1]) and torch.equal(ps, p0[1])
    mk, pk = tester.segment(net3, x[1], **kw)
    assert mk.shape == (9, 14) and pk.shape == (3, 9, 14)
    with pytest.raises(ValueError, match="rot3"):
        tester.segment(None, x, views="rot3")                                    # parsed before the net is even looked at
