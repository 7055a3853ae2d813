"""Overlap-tile segmentation on the device (tester.segment -> unet_tile_gather, unet_forward, unet_tile_stitch) against the
numpy restatement in tests/segment_ref.py (np.pad(reflect) tiles, numpy stitch), Unet.forward on the same chunks and the
fp64 C oracle."""
import numpy as np
import pytest
import torch

import segment_ref as ref
from gpu_support import dev, image, math_mode, net

pytestmark = pytest.mark.gpu


def gather(x, S, t0, nt, minmax=None):
    import _hip
    import tester
    B, H, W = x.shape
    ny, nx, oy0, ox0 = tester.tile_grid(H, W, S)
    out = torch.full((nt, 1, S, S), float("nan"), device=x.device)
    _hip.run("unet_tile_gather", x.device, _hip.ptr(x), B, H, W, _hip.ptr(minmax), S, oy0, ox0, ny, nx, t0, nt, _hip.ptr(out))
    return out


def minmax(x):
    import _hip
    B, H, W = x.shape
    mm = torch.empty(B, 2, device=x.device)
    _hip.run("unet_minmax", x.device, _hip.ptr(x), B, H * W, _hip.ptr(mm))
    return mm


# ---- gather --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,S", [(1, 2, 2, 188), (1, 37, 5, 188), (1, 520, 696, 188), (1, 1000, 1000, 188),
                                     (3, 520, 696, 572), (3, 37, 300, 220), (2, 389, 388, 1212)])
def test_gather_is_numpy_reflect_pad(dev, B, H, W, S):
    """Bit-identical to np.pad(reflect) + slicing, raw and normalised ((x - min) / (max - min), fp32 true division), for
    the whole tile range and for sub-ranges that start mid-image."""
    img = image(B * 1000 + H + W, B, H, W, blobs=12)
    x = torch.from_numpy(img).to(dev)
    T = len(ref.tile_windows(H, W, S)[0]) * B
    want, want_n = ref.tiles(img, S), ref.tiles(img, S, norm=True)
    assert np.array_equal(gather(x, S, 0, T).cpu().numpy(), want)
    assert np.array_equal(gather(x, S, 0, T, minmax(x)).cpu().numpy(), want_n)
    if T > 2:
        t0, nt = T // 2, T - T // 2 - 1
        assert np.array_equal(gather(x, S, t0, nt).cpu().numpy(), want[t0:t0 + nt])
        assert np.array_equal(gather(x, S, t0, nt, minmax(x)).cpu().numpy(), want_n[t0:t0 + nt])


def test_gather_of_the_last_tiles_of_an_image_over_2GiB(dev):
    """24000^2 float32 (2.3 GB): the last tiles of the image read rows whose byte offsets exceed 2^31.  Expected values
    from np.pad(reflect) of the image's last rows, which is all the windows of the last grid row read."""
    import tester
    H = W = 24000
    S, K = 572, 1200
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.rand(1, H, W, generator=g, device=dev)
    assert x.numel() * 4 > 2 ** 31
    ny, nx, oy0, ox0 = tester.tile_grid(H, W, S)
    So = S - 184
    nt = 3
    t0 = ny * nx - nt
    tail = x[0, H - K:].cpu().numpy()
    assert oy0 + (ny - 1) * So - 92 >= H - K
    pad = np.pad(tail, S, mode="reflect")                          # the top band is not the image's, and is never read
    lo, hi = float(x.min()), float(x.max())
    mm = torch.tensor([[lo, hi]], device=dev)
    got, got_n = gather(x, S, t0, nt).cpu().numpy(), gather(x, S, t0, nt, mm).cpu().numpy()
    for k in range(nt):
        i, j = divmod(t0 + k, nx)
        r0, c0 = oy0 + i * So - 92 - (H - K) + S, ox0 + j * So - 92 + S
        want = pad[r0:r0 + S, c0:c0 + S]
        assert np.array_equal(got[k, 0], want), k
        assert np.array_equal(got_n[k, 0], (want - np.float32(lo)) / (np.float32(hi) - np.float32(lo))), k


def test_unaligned_buffers_take_the_scalar_path(dev):
    """Tile and logit buffers that are not 16-byte aligned: same results as aligned ones."""
    import _hip
    import tester
    B, H, W, S = 2, 45, 70, 188
    So = S - 184
    ny, nx, oy0, ox0 = tester.tile_grid(H, W, S)
    T = B * ny * nx
    img = image(3, B, H, W, blobs=12)
    x = torch.from_numpy(img).to(dev)
    buf = torch.full((T * S * S + 1,), float("nan"), device=dev)
    _hip.run("unet_tile_gather", dev, _hip.ptr(x), B, H, W, None, S, oy0, ox0, ny, nx, 0, T, _hip.ptr(buf[1:]))
    assert np.array_equal(buf[1:].cpu().numpy().reshape(T, 1, S, S), ref.tiles(img, S))
    lg = np.random.RandomState(4).randn(T, 2, So, So).astype(np.float32)
    lbuf = torch.zeros(lg.size + 1, device=dev)
    lbuf[1:] = torch.from_numpy(lg.ravel()).to(dev)
    mask = torch.full((B, H, W), -7, dtype=torch.int64, device=dev)
    prob = torch.empty(B, H, W, device=dev)
    _hip.run("unet_tile_stitch", dev, _hip.ptr(lbuf[1:]), So, oy0, ox0, ny, nx, 0, T, B, H, W, _hip.ptr(mask), _hip.ptr(prob))
    want_m, want_p = ref.stitch(lg, B, H, W, S)
    assert np.array_equal(mask.cpu().numpy(), want_m)
    assert np.abs(prob.cpu().numpy() - want_p).max() <= 4e-7


def test_gather_rejects_bad_ranges(dev):
    import _hip
    x = torch.zeros(1, 50, 60, device=dev)
    out = torch.empty(4, 1, 188, 188, device=dev)
    L = _hip.lib()
    st = _hip.stream(dev)
    ny, nx = 13, 15                                               # So = 4
    assert L.unet_tile_gather(_hip.ptr(x), 1, 50, 60, None, 188, -1, 0, ny, nx, ny * nx - 3, 4, _hip.ptr(out), st) != 0
    assert L.unet_tile_gather(_hip.ptr(x), 1, 50, 60, None, 188, -1, 0, ny + 1, nx, 0, 4, _hip.ptr(out), st) != 0
    assert L.unet_tile_gather(_hip.ptr(x), 1, 50, 60, None, 190, -1, 0, ny, nx, 0, 4, _hip.ptr(out), st) != 0
    assert L.unet_tile_gather(_hip.ptr(x), 1, 50, 60, None, 188, -1, 0, ny, nx, ny * nx - 4, 4, _hip.ptr(out), st) == 0


# ---- stitch --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,S", [(1, 2, 2, 188), (2, 37, 5, 188), (1, 520, 696, 572), (3, 130, 70, 220),
                                     (1, 1500, 1500, 700)])
def test_stitch_mask_probability_and_bounds(dev, B, H, W, S):
    """Synthetic logits with exact ties: the mask is bit-identical to the numpy stitch (ties -> class 0), the probability
    within 4e-7 of fp64 softmax; every pixel is written, nothing outside [B,H,W] is (guards around both outputs).  The
    tiles are stitched in three ranges of different lengths."""
    import _hip
    import tester
    So = S - 184
    ny, nx, oy0, ox0 = tester.tile_grid(H, W, S)
    T = B * ny * nx
    rs = np.random.RandomState(H * W + B)
    lg = (rs.randn(T, 2, So, So) * 4).astype(np.float32)
    tie = rs.rand(T, So, So) < 0.1
    lg[:, 1][tie] = lg[:, 0][tie]
    lg[:, 1][rs.rand(T, So, So) < 0.01] = 1e30                   # exp overflow -> probability 0 / 1
    want_m, want_p = ref.stitch(lg, B, H, W, S)
    G, n = 4096, B * H * W
    mbuf = torch.full((n + 2 * G,), -7, dtype=torch.int64, device=dev)
    pbuf = torch.full((n + 2 * G,), float("nan"), device=dev)
    lgd = torch.from_numpy(lg).to(dev)
    cuts = sorted({0, T, T // 3, (2 * T) // 3 + (T > 2)})
    for a, b in zip(cuts[:-1], cuts[1:]):
        _hip.run("unet_tile_stitch", dev, _hip.ptr(lgd[a:b]), So, oy0, ox0, ny, nx, a, b - a, B, H, W, _hip.ptr(mbuf[G:G + n]),
                 _hip.ptr(pbuf[G:G + n]))
    m, p = mbuf.cpu().numpy(), pbuf.cpu().numpy()
    assert (m[:G] == -7).all() and (m[G + n:] == -7).all()
    assert np.isnan(p[:G]).all() and np.isnan(p[G + n:]).all()
    m, p = m[G:G + n].reshape(B, H, W), p[G:G + n].reshape(B, H, W)
    assert np.array_equal(m, want_m)
    assert not np.isnan(p).any()
    assert np.abs(p - want_p).max() <= 4e-7
    # without the probability, the mask alone (prob NULL)
    mbuf.fill_(-7)
    _hip.run("unet_tile_stitch", dev, _hip.ptr(lgd), So, oy0, ox0, ny, nx, 0, T, B, H, W, _hip.ptr(mbuf[G:G + n]), None)
    m = mbuf.cpu().numpy()
    assert np.array_equal(m[G:G + n].reshape(B, H, W), want_m) and (m[:G] == -7).all() and (m[G + n:] == -7).all()


@pytest.mark.parametrize("K", [2, 3])
def test_stitch_and_stitch_k_against_numpy_on_a_clipped_grid(dev, K):
    """unet_tile_stitch (K = 2) and unet_tile_stitch_k (K = 2 and 3) on a 2 x 9 x 14 batch, whose 3 x 4 grid of 4-pixel tiles
    overhangs the image on both axes, against numpy on guarded buffers.  Logits with exact ties, some of them at the maximum:
    the masks are bit-equal to l1 > l0 and to the first maximum (ties -> the lowest class).  Probabilities against fp64:
    1 / (1 + e^(l0 - l1)) within 4e-7 (d = l0 - l1 is rounded once, which moves p by at most p (1 - p) |d| 2^-24 <=
    0.23 * 2^-24; expf's 2 ulp move it by at most 4 p (1 - p) 2^-24 <= 2^-24; the sum and the division add 2^-24 each: below
    3.3 * 2^-24 = 2e-7), the softmax within multiclass_ref.softmax_bound."""
    import _hip
    import guarded
    import multiclass_ref
    import tester
    B, H, W, S = 2, 9, 14, 188
    So = S - 184
    ny, nx, oy0, ox0 = tester.tile_grid(H, W, S)
    assert (ny, nx) == (3, 4) and oy0 < 0 and ox0 < 0
    T = B * ny * nx
    rs = np.random.RandomState(31 + K)
    lg = (rs.randn(T, K, So, So) * 4).astype(np.float32)
    tie = rs.rand(T, So, So) < 0.2
    lg[:, 1][tie] = lg[:, 0][tie]
    top = rs.rand(T, So, So) < 0.1
    lg[:, 0][top] = lg[:, 1][top] = np.abs(lg).max(axis=1)[top] + 1
    ar = guarded.Arena(dev)
    lgd = ar.inp(torch.from_numpy(lg))
    want_m, want_p = multiclass_ref.stitch_k(lg, B, H, W, S)
    assert (want_m == 0).any() and (want_m == K - 1).any()
    mask, prob = ar.out((B, H, W), torch.int64), ar.out((B, K, H, W))
    _hip.run("unet_tile_stitch_k", dev, ar.ptr(lgd), So, K, oy0, ox0, ny, nx, 0, T, B, H, W, ar.ptr(mask), ar.ptr(prob))
    ar.verify(mask, prob)
    assert np.array_equal(mask.cpu().numpy(), want_m)
    assert np.abs(prob.cpu().numpy() - want_p).max() <= multiclass_ref.softmax_bound(lg, K)
    if K == 2:
        want_m2, want_p2 = ref.stitch(lg, B, H, W, S)
        assert np.array_equal(want_m2, want_m)
        mask2, prob2 = ar.out((B, H, W), torch.int64), ar.out((B, H, W))
        _hip.run("unet_tile_stitch", dev, ar.ptr(lgd), So, oy0, ox0, ny, nx, 0, T, B, H, W, ar.ptr(mask2), ar.ptr(prob2))
        ar.verify(mask2, prob2)
        assert np.array_equal(mask2.cpu().numpy(), want_m2)
        assert np.abs(prob2.cpu().numpy() - want_p2).max() <= 4e-7


# ---- end to end ----------------------------------------------------------------------------------------------------------

def pipeline(net, img, S, max_batch, norm=True):
    """numpy tiles -> Unet.forward on the same chunks segment uses -> numpy stitch."""
    B, H, W = img.shape
    tl = torch.from_numpy(ref.tiles(img, S, norm=norm)).to(next(net.parameters()).device)
    with torch.no_grad():
        lg = torch.cat([net(tl[a:a + max_batch]) for a in range(0, tl.shape[0], max_batch)]).cpu().numpy()
    return ref.stitch(lg, B, H, W, S), lg


@pytest.mark.parametrize("mode", [3, 2])
@pytest.mark.parametrize("B,H,W,S,mb", [(1, 520, 696, None, 16), (1, 520, 696, 572, 3), (1, 1500, 1500, None, 3),
                                        (1, 1500, 1500, 572, 6), (1, 300, 300, None, 16), (2, 130, 400, 220, 5)])
def test_segment_matches_numpy_pipeline(dev, net, math_mode, mode, B, H, W, S, mb):
    """fp32 (Winograd, the default) and bf16 math: masks bit for bit, probabilities within 4e-7 of fp64 softmax of the
    pipeline's logits.  S=None: the automatic size (one 508 tile for 300^2, one 892 tile for 520x696, four 1212 tiles - the
    cap - for 1500^2)."""
    import tester
    math_mode(mode)
    img = image(H + W + mode, B, H, W, blobs=12)
    S_used = S or tester.auto_tile_size(H, W)
    if S is None:
        assert (H, W, S_used, tester.tile_grid(H, W, S_used)[:2]) in ((300, 300, 508, (1, 1)), (520, 696, 892, (1, 1)),
                                                                       (1500, 1500, 1212, (2, 2)))
    (want_m, want_p), _ = pipeline(net, img, S_used, mb)
    m, p = tester.segment(net, torch.from_numpy(img).to(dev), tile_size=S, max_batch=mb, return_probs=True)
    assert m.dtype == torch.int64 and p.dtype == torch.float32 and m.shape == (B, H, W) == p.shape
    assert np.array_equal(m.cpu().numpy(), want_m)
    assert np.abs(p.cpu().numpy() - want_p).max() <= 4e-7
    print("S=%d: foreground fraction %.3f" % (S_used, want_m.mean()))


def test_segment_half_width_net_and_unnormalised(dev):
    """A base_ch=32 module uses its own handle; normalise=False feeds the raw values."""
    import network
    import tester
    from oracle import prng
    m32 = network.Unet(base_ch=32)
    m32.load_state_dict({k: torch.from_numpy(v) for k, v in prng.make_params(3, base=32).items()})
    m32 = m32.to(dev)
    img = image(5, 1, 400, 250, blobs=12) / 255
    (want_m, _), _ = pipeline(m32, img, 572, 16, norm=False)
    got = tester.segment(m32, torch.from_numpy(img).to(dev), tile_size=572, normalise=False)
    assert np.array_equal(got.cpu().numpy(), want_m)


def test_bf16_chunks_stay_below_2GiB_tensors(dev, net, math_mode):
    """With bf16 tensors a chunk of 16 tiles of 1212^2 would put conv11c's output over 2 GiB, which the bf16 kernels cannot
    address: segment runs chunks of 11 instead, the same as the pipeline in chunks of 11."""
    import tester
    math_mode(2)
    img = image(61, 1, 3100, 3100, blobs=12)
    assert tester.auto_tile_size(3100, 3100) == 1212 and tester.tile_grid(3100, 3100, 1212)[:2] == (4, 4)
    (want_m, _), _ = pipeline(net, img, 1212, 11)
    got = tester.segment(net, torch.from_numpy(img).to(dev), max_batch=16)
    assert np.array_equal(got.cpu().numpy(), want_m)


def test_segment_two_tiles_vs_fp64_c_oracle(dev, net):
    """S=188 (So=4), a 4x8 image = 2 tiles: the mask agrees with the fp64 C oracle on every pixel whose fp64 logit margin
    exceeds 10x the forward tolerance (2e-5 of the logit scale), as tests/test_net_gpu.py judges argmax masks."""
    import tester
    from oracle import oracle_c, prng
    img = image(11, 1, 4, 8, blobs=12)
    m = tester.segment(net, torch.from_numpy(img).to(dev), tile_size=188).cpu().numpy()
    tl = ref.tiles(img, 188, norm=True).astype(np.float64)
    assert tl.shape[0] == 2
    lg, _ = oracle_c.unet_fwd_bwd(prng.make_params(0, dtype=np.float64), tl)
    want, _ = ref.stitch(lg, 1, 4, 8, 188)
    margin = ref.stitch_plane(np.abs(lg[:, 1] - lg[:, 0]), 1, 4, 8, 188)
    safe = margin > 2e-4 * np.abs(lg).max()
    assert safe.mean() > 0.9
    assert np.array_equal(m[0][safe[0]], want[0][safe[0]])


def test_chunking_does_not_change_the_result(dev, net):
    """max_batch 1 and 16 on the same 16-tile image: identical masks and probabilities."""
    import tester
    x = torch.from_numpy(image(21, 1, 1500, 1500, blobs=12)).to(dev)
    m1, p1 = tester.segment(net, x, max_batch=1, return_probs=True)
    m16, p16 = tester.segment(net, x, max_batch=16, return_probs=True)
    assert torch.equal(m1, m16)
    assert torch.equal(p1, p16)


def test_side_stream_and_repeat_determinism(dev, net):
    import tester
    x = torch.from_numpy(image(31, 2, 700, 450, blobs=12)).to(dev)
    m0, p0 = tester.segment(net, x, max_batch=3, return_probs=True)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(2):
            m1, p1 = tester.segment(net, x, max_batch=3, return_probs=True)
    torch.cuda.current_stream(dev).wait_stream(s)
    m2, p2 = tester.segment(net, x, max_batch=3, return_probs=True)
    assert torch.equal(m0, m1) and torch.equal(p0, p1) and torch.equal(m0, m2) and torch.equal(p0, p2)


def test_return_shapes_and_integer_images(dev, net):
    import tester
    img = np.round(image(41, 2, 90, 130, blobs=12)).clip(0, 255)
    x = torch.from_numpy(img.astype(np.float32)).to(dev)
    mb = tester.segment(net, x)
    assert mb.shape == (2, 90, 130) and mb.dtype == torch.int64
    m, p = tester.segment(net, x[1], return_probs=True)
    assert m.shape == (90, 130) and p.shape == (90, 130) and m.dtype == torch.int64 and p.dtype == torch.float32
    assert torch.equal(m, mb[1])
    assert torch.equal(tester.segment(net, x.to(torch.uint8)), mb)
    assert torch.equal(tester.segment(net, x.to(torch.uint16)), mb)


def test_segment_errors(dev, net):
    import tester
    x = torch.from_numpy(image(51, 1, 60, 60, blobs=12)).to(dev)
    with pytest.raises(RuntimeError, match="HIP device"):
        tester.segment(net, x.cpu())
    with pytest.raises(ValueError):
        tester.segment(net, x[:, :1, :])
    with pytest.raises(ValueError):
        tester.segment(net, x[:, :, :1])
    with pytest.raises(ValueError, match="572 and 604"):
        tester.segment(net, x, tile_size=600)
    with pytest.raises(ValueError):
        tester.segment(net, x[None])
    c = torch.full((2, 40, 40), 3.0, device=dev)
    c[0, 5, 5] = 4.0
    with pytest.raises(ValueError, match="constant"):
        tester.segment(net, c)
    assert tester.segment(net, c, normalise=False).shape == (2, 40, 40)
