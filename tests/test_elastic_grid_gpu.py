"""The paper's elastic deformation on the device (elastic.hip: unet_elastic_grid, unet_elastic_grid_sample, unet_normalise01;
data.elastic_grid, data.augment(elastic='grid'), data.CropDataset(elastic='grid')) against the fp64 restatement
tests/elastic_grid_ref.py, which tests/test_elastic_grid_cpu.py pins to torch's bicubic and scipy's map_coordinates.  Every
buffer handed to the raw entry points is a poisoned guarded.Arena buffer.  The references are computed once per case."""
import functools
import os

import numpy as np
import pytest
import torch

import elastic_grid_ref as ref
import guarded
from gpu_support import dev

pytestmark = pytest.mark.gpu

WARP_CASES = ((37, 53, 3), (64, 48, 2), (61, 61, 5))          # H, W, G: odd sizes, no multiple of the 16 x 64 tile, several blocks
A_VALUES = (-0.5, -0.75)
SAMPLE_CASES = ((92, 20, 52), (61, 0, 61))                    # S, pad, crop
LEVELS = (255, 65535, 0)
# |device - fp64 restatement| for float outputs of values up to 255: what is left is the narrowing to fp32 at the store (half
# an ulp at 255 = 7.6e-6) and fp64 roundings (1e-13); 255 * 1e-6 = 2.55e-4 is the issue's outer bound, 2e-5 the one asserted
FLOAT_BOUND = 2e-5


def blobs(rs, B, H, W):
    """{0,255} masks: a few discs per image"""
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((B, H, W), bool)
    for b in range(B):
        for _ in range(6):
            cy, cx, r = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(4, max(5, min(H, W) / 4))
            m[b] |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return m * np.float32(255)


@functools.lru_cache(maxsize=None)
def warp_case(H, W, G, a):
    """P = 2 planes (grey levels, a mask) of B = 3 samples, a different sigma = 10 grid per sample, and the restatement.  The
    grids come from RandomState(7): for it the share of pixels that sample outside the image lies in 3 .. 25 % at all three
    shapes and both a (asserted by the test); RandomState(5) gives 25.7 % at 64 x 48."""
    rs = np.random.RandomState(5)
    planes = np.stack([(rs.rand(3, H, W) * 255).astype(np.float32), blobs(rs, 3, H, W)])
    grids = np.random.RandomState(7).normal(0, 10, (3, 2, G, G))
    want = ref.warp(planes, grids, a)
    outside = np.mean([(lambda cy, cx: (cy < 0) | (cy > H - 1) | (cx < 0) | (cx > W - 1))(*ref.coordinates(g, H, W, a)) for g in grids])
    return planes, grids, want, float(outside)


def raw_grid(dev, planes, grids, a):
    import _hip
    arena = guarded.Arena(dev)
    P, B, H, W = planes.shape
    x = arena.inp(torch.from_numpy(planes), "planes")
    g = arena.inp(torch.from_numpy(np.ascontiguousarray(grids, np.float64)), "grid")
    out = arena.out((P, B, H, W), torch.float32, "out")
    _hip.run("unet_elastic_grid", dev, arena.ptr(x), P, B, H, W, arena.ptr(g), grids.shape[-1], a, arena.ptr(out))
    arena.verify(out)
    return out.cpu().numpy()


@pytest.mark.parametrize("a", A_VALUES)
@pytest.mark.parametrize("H,W,G", WARP_CASES)
def test_general_warp_equals_the_restatement(dev, H, W, G, a):
    planes, grids, want, outside = warp_case(H, W, G, a)
    assert 0.03 <= outside <= 0.25, outside                   # enough pixels whose source lies outside: they must be 0
    got = raw_grid(dev, planes, grids, a)
    err = float(np.abs(got - want).max())
    print("elastic_grid %dx%d G=%d a=%g: largest |device - fp64| = %.3g, %.1f %% of the pixels sample outside" % (H, W, G, a, err, 100 * outside))
    assert (got[want == 0] == 0).all()
    assert err <= FLOAT_BOUND


@pytest.mark.parametrize("a", A_VALUES)
@pytest.mark.parametrize("H,W,G", WARP_CASES)
def test_zero_and_whole_pixel_grids_are_exact(dev, H, W, G, a):
    """A zero grid returns the input bit for bit; a constant grid of whole pixels (r, c) returns the input shifted by exactly
    (r, c): out[y, x] = in[y + r, x + c], 0 where that lies outside."""
    planes = warp_case(H, W, G, a)[0]
    got = raw_grid(dev, planes, np.zeros((3, 2, G, G)), a)
    assert np.array_equal(got.view(np.uint32), planes.view(np.uint32))
    shifts = ((3, -5), (-2, 7), (-H, 1))                       # the last one moves every source out of the image
    grids = np.stack([np.stack([np.full((G, G), float(r)), np.full((G, G), float(c))]) for r, c in shifts])
    got = raw_grid(dev, planes, grids, a)
    for b, (r, c) in enumerate(shifts):
        want = np.zeros_like(planes[:, b])
        ys, xs = np.arange(H), np.arange(W)
        oy, ox = ys[(ys + r >= 0) & (ys + r < H)], xs[(xs + c >= 0) & (xs + c < W)]
        if len(oy) and len(ox):
            want[:, oy[0]:oy[-1] + 1, ox[0]:ox[-1] + 1] = planes[:, b, oy[0] + r:oy[-1] + r + 1, ox[0] + c:ox[-1] + c + 1]
        assert np.array_equal(got[:, b].view(np.uint32), want.view(np.uint32)), (r, c)


SAMPLE_SEEDS = {(92, 255): 1, (92, 65535): 1, (92, 0): 1, (61, 255): 1, (61, 65535): 1, (61, 0): 1}


@functools.lru_cache(maxsize=None)
def sample_case(S, pad, crop, levels):
    """B = 2 images of grey levels 0 .. max(levels, 255) and {0,255} masks, sigma = 10 grids of 3 x 3, the restatement, and the
    host-side facts the exact comparison rests on"""
    rs = np.random.RandomState(SAMPLE_SEEDS[S, levels])
    img = np.floor(rs.rand(2, S, S) * (max(levels, 255) + 1)).astype(np.float32)
    mask = blobs(rs, 2, S, S)
    grids = rs.normal(0, 10, (2, 2, 3, 3))
    r = ref.sample(img, mask, grids, -0.5, levels, pad, crop)
    # no value within 1e-6 of a rounding boundary k + 0.5, no mask value within 1e-6 of the threshold: else another seed
    for raw in (r["raw_img"], r["raw_mask"]):
        assert np.abs(raw - np.floor(raw) - 0.5).min() > 1e-6
    assert np.abs(r["raw_mask"] - 127).min() > 1e-6
    assert 0 < r["out_gt"].mean() < 1
    return img, mask, grids, r


def raw_sample(dev, img, mask, grids, levels, pad, crop, normalise=False):
    import _hip
    arena = guarded.Arena(dev)
    B, S, _ = img.shape
    x = arena.inp(torch.from_numpy(img), "img")
    m = arena.inp(torch.from_numpy(mask), "mask")
    g = arena.inp(torch.from_numpy(np.ascontiguousarray(grids, np.float64)), "grid")
    out = arena.out((B, S, S), torch.float32, "out_img")
    gt = arena.out((B, crop, crop), torch.int64, "out_gt")
    mm = arena.out((B, 2), torch.float32, "minmax")
    _hip.run("unet_elastic_grid_sample", dev, arena.ptr(x), arena.ptr(m), B, S, arena.ptr(g), grids.shape[-1], -0.5, levels, pad, crop,
             arena.ptr(out), arena.ptr(gt), arena.ptr(mm))
    arena.verify(out, gt, mm)
    res = [out.cpu().numpy(), gt.cpu().numpy(), mm.cpu().numpy()]
    if normalise:
        _hip.run("unet_normalise01", dev, arena.ptr(out), B, S * S, arena.ptr(mm))
        arena.verify(out)
        res.append(out.cpu().numpy())
    return res


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("S,pad,crop", SAMPLE_CASES)
def test_fused_sample_equals_the_restatement(dev, S, pad, crop, levels):
    """out_img and out_gt equal the restatement (levels > 0; with levels = 0 the image is a float output of values up to 255
    and held to FLOAT_BOUND); minmax is the min and max of out_img; unet_normalise01 gives numpy's fp32 (x - lo) / (hi - lo)
    bit for bit; and the mask is read for the label window only.

    The last check as the issue words it - poison EVERY mask pixel outside the window - cannot hold for a correct kernel: a
    window pixel displaced by up to 25 pixels samples the mask outside the window (asserted below for pad > 0), exactly as
    augment's gt[pad:pad+crop] of the fully warped mask does.  What is poisoned instead is every mask pixel outside the
    window that no window pixel's bilinear footprint touches (from the restatement's fp64 coordinates): a kernel that warps
    the mask anywhere outside the window, or reads beyond the four neighbours, meets NaN, and a NaN that reaches out_gt
    turns a 1 into a 0."""
    img, mask, grids, r = sample_case(S, pad, crop, levels)
    out, gt, mm, norm = raw_sample(dev, img, mask, grids, levels, pad, crop, normalise=True)
    if levels:
        assert np.array_equal(out, r["out_img"])
    else:
        err = float(np.abs(out - r["raw_img"]).max())
        print("elastic_grid_sample S=%d float image: largest |device - fp64| = %.3g" % (S, err))
        assert err <= FLOAT_BOUND
    assert gt.dtype == np.int64 and np.array_equal(gt, r["out_gt"])
    assert np.array_equal(mm[:, 0], out.reshape(2, -1).min(1)) and np.array_equal(mm[:, 1], out.reshape(2, -1).max(1))
    want = ref.normalise01(out, mm)
    assert np.array_equal(norm.view(np.uint32), want.view(np.uint32))
    assert norm.min() == 0 and norm.max() == 1
    window = np.zeros((2, S, S), bool)
    window[:, pad:pad + crop, pad:pad + crop] = True
    if pad:
        assert (r["reads"] & ~window).any()                  # the window's pixels do sample the mask outside the window
    poison = ~window & ~r["reads"]
    if pad:
        assert poison.sum() > (~window).sum() // 2
    poisoned = mask.copy()
    poisoned[poison] = np.nan
    gt2 = raw_sample(dev, img, poisoned, grids, levels, pad, crop)[1]
    assert np.array_equal(gt2, gt)


def augment_inputs(dev):
    rs = np.random.RandomState(9)
    image = torch.from_numpy(np.floor(rs.rand(2, 96, 96) * 256).astype(np.float32)).to(dev)
    target = torch.from_numpy(blobs(rs, 2, 96, 96)).to(dev)
    return image, target, [(10, 30), (44, 3)], [30.0, 240.0]


def test_augment_grid(dev):
    import data
    from functions import input_size_compute
    image, target, origins, angles = augment_inputs(dev)
    crop = 52
    S = input_size_compute(torch.empty(crop, crop))[1]
    run = lambda seed: data.augment(image, target, origins, crop, angles, 3, 10, random_state=np.random.RandomState(seed), elastic="grid")
    inp, gt = run(7)
    assert inp.shape == (2, 1, S, S) and inp.dtype == torch.float32
    assert gt.shape == (2, 1, crop, crop) and gt.dtype == torch.int64
    for b in range(2):
        assert float(inp[b].min()) == 0.0 and float(inp[b].max()) == 1.0
    assert set(gt.unique().tolist()) == {0, 1}
    # stable for equal seeds, different for others
    again = run(7)
    assert torch.equal(inp, again[0]) and torch.equal(gt, again[1])
    assert not torch.equal(inp, run(8)[0])
    # a batched call is the per-sample calls, the generator consumed sample after sample
    rs = np.random.RandomState(7)
    for b in range(2):
        one = data.augment(image[b], target[b], origins[b], crop, angles[b], 3, 10, random_state=rs, elastic="grid")
        assert one[0].shape == (1, S, S) and one[1].shape == (1, crop, crop)
        assert torch.equal(one[0], inp[b]) and torch.equal(one[1], gt[b])
    # disp overrides the draw; alpha is ignored
    d = data.grid_displacements(np.random.RandomState(7), 2, 3, 10)
    given = data.augment(image, target, origins, crop, angles, 99, 10, disp=d, elastic="grid")
    assert torch.equal(given[0], inp) and torch.equal(given[1], gt)
    given = data.augment(image, target, origins, crop, angles, 3, 10, disp=torch.from_numpy(d).to(dev), elastic="grid", random_state=None)
    assert torch.equal(given[0], inp) and torch.equal(given[1], gt)
    # and it is the pieces: rotate, the restatement of the fused sample, the normalisation
    both = data.reflect_rotate_crop(torch.cat([torch.stack([image[b, x:x + crop, y:y + crop] for b, (x, y) in enumerate(origins)]),
                                               torch.stack([target[b, x:x + crop, y:y + crop] for b, (x, y) in enumerate(origins)])]),
                                    angles + angles, S).cpu().numpy()
    pad = (S - crop) // 2
    r = ref.sample(both[:2], both[2:], d, -0.5, 255, pad, crop)
    for raw in (r["raw_img"], r["raw_mask"]):                # 3e5 values: none within 1e-9 of a rounding boundary (fp64 noise is 1e-12)
        assert np.abs(raw - np.floor(raw) - 0.5).min() > 1e-9
    assert np.array_equal(gt[:, 0].cpu().numpy(), r["out_gt"])
    assert np.array_equal(inp[:, 0].cpu().numpy(), ref.normalise01(r["out_img"], r["minmax"]))


def test_augment_field_is_unchanged(dev):
    """elastic='field' (the default) gives what augment gave before the option existed: elastic_transform composed by hand the
    way augment composes it, with the same host draws."""
    import data
    from functions import input_size_compute
    image, target, origins, angles = augment_inputs(dev)
    crop = 52
    S = input_size_compute(torch.empty(crop, crop))[1]
    for kw in (dict(), dict(elastic="field"), dict(elastic="field", grid=5, a=-0.75)):
        inp, gt = data.augment(image, target, origins, crop, angles, 3, 10, random_state=np.random.RandomState(4), **kw)
        img = torch.stack([image[b, x:x + crop, y:y + crop] for b, (x, y) in enumerate(origins)]).float()
        tgt = torch.stack([target[b, x:x + crop, y:y + crop] for b, (x, y) in enumerate(origins)]).float()
        both = data.reflect_rotate_crop(torch.cat((img, tgt)), angles + angles, S, levels=255)
        wi, wg = data.elastic_transform((both[:2], both[2:]), 3, 10, random_state=np.random.RandomState(4))
        wi = torch.floor(wi + 0.5).clamp_(0, 255)
        wg = torch.floor(wg + 0.5).clamp_(0, 255)
        pad = int((S - crop) / 2)
        wg = (wg[:, pad:crop + pad, pad:crop + pad] > 127).long()
        lo, hi = wi.amin(dim=(1, 2), keepdim=True), wi.amax(dim=(1, 2), keepdim=True)
        wi = (wi - lo) / (hi - lo)
        assert torch.equal(inp, wi[:, None]) and torch.equal(gt, wg[:, None])


def test_elastic_grid_public(dev):
    """data.elastic_grid on [H,W] and [B,H,W] tuples equals the raw entry point; device-side ValueErrors."""
    import data
    planes, grids, want, _ = warp_case(37, 53, 3, -0.5)
    a, b = torch.from_numpy(planes[0]).to(dev), torch.from_numpy(planes[1]).to(dev)
    got = data.elastic_grid((a, b), grids)
    assert len(got) == 2 and got[0].shape == (3, 37, 53) and got[0].dtype == torch.float32
    raw = raw_grid(dev, planes, grids, -0.5)
    assert np.array_equal(got[0].cpu().numpy(), raw[0]) and np.array_equal(got[1].cpu().numpy(), raw[1])
    one = data.elastic_grid((a[1], b[1]), torch.from_numpy(grids[1]).to(dev), a=-0.5)
    assert one[0].shape == (37, 53) and np.array_equal(one[0].cpu().numpy(), raw[0, 1]) and np.array_equal(one[1].cpu().numpy(), raw[1, 1])
    narrow = grids[1].astype(np.float32)                   # any float type: used as the fp64 numbers it holds
    assert torch.equal(data.elastic_grid((a[1],), torch.from_numpy(narrow).to(dev))[0], data.elastic_grid((a[1],), narrow.astype(np.float64))[0])
    same = data.elastic_grid((a,), grids[0])                # [2,G,G]: every sample alike
    assert np.array_equal(same[0][0].cpu().numpy(), raw[0, 0])
    with pytest.raises(ValueError):
        data.elastic_grid((a, b[:2]), grids)
    with pytest.raises(ValueError):
        data.elastic_grid((a,), grids[:2])
    with pytest.raises(ValueError):
        data.elastic_grid((a,), np.zeros((3, 2, 1, 1)))
    with pytest.raises(ValueError):
        data.elastic_grid((a.cpu(),), grids)


def test_crop_dataset_grid_trains_a_step(dev, tmp_path):
    """CropDataset(elastic='grid') yields batches trainer.training's step accepts: one step on a base-32 net at the smallest
    legal tile (crop 196, S = 380), and the batch is data.augment(elastic='grid') with a host replay of the draws."""
    import data
    import network
    import prepare_ref
    import trainer
    N, H, W, crop = 2, 230, 250, 196
    rs = np.random.RandomState(77)
    images = (rs.rand(N, H, W) * 255).astype(np.uint8)
    inst = prepare_ref.ids_batch("discs", 21, N, H, W).astype(np.uint16)
    make = lambda: data.CropDataset(images, inst, 3, 10, crop, 2, np.random.RandomState(5), random_state=np.random.RandomState(6),
                                    elastic="grid", grid=3)
    ds = make()
    assert len(ds) == 1
    (inp, gt), = list(ds)
    assert inp.shape == (2, 1, 380, 380) and inp.dtype == torch.float32 and gt.shape == (2, 1, crop, crop) and gt.dtype == torch.int64
    replay = np.random.RandomState(5)
    origins, angles = [], []
    for i in range(N):
        origins.append(data.draw_crop(replay, ds.pairs, ds.target_weighted_crop_distribution[i], (H, W), crop))
        angles.append(replay.choice(np.arange(0, 360, 30)))
    winp, wgt = data.augment(ds.image, ds.target, origins, crop, angles, 3, 10, random_state=np.random.RandomState(6), elastic="grid")
    assert torch.equal(inp, winp) and torch.equal(gt, wgt)
    assert 0 < int(gt.sum()) < gt.numel()
    ds = make()
    net = network.Unet(base_ch=32).to(dev)
    trainer.training(net, ds, ds, 0, 2, dev, str(tmp_path), "elastic-grid-test")
    loss = np.loadtxt(os.path.join(str(tmp_path), "progress", "loss.out"))
    loss_val = np.loadtxt(os.path.join(str(tmp_path), "progress", "loss_val.out"))
    assert loss.size == 1 and np.isfinite(loss).all() and np.isfinite(loss_val).all()
