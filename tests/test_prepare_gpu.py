"""Targets and weighted crops from instance images on the device (data.preprocess_gt / binary_target -> unet_carve_borders,
data.crop_distribution -> unet_crop_counts, data.CropDataset) against the numpy/scipy restatement tests/prepare_ref.py, which
tests/test_prepare_cpu.py pins to the reference's own outputs and to hand-worked answers.  Everything compared here is exact
(integers; the float64 probabilities within the bound derived in test_prepare_cpu.py).  Every pointer handed to the raw entry
points is a poisoned guarded.Arena buffer."""
import os

import numpy as np
import pytest
import torch

import guarded
import prepare_ref as ref
from gpu_support import dev

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 2), (2, 1), (1, 40), (9, 9), (17, 5), (33, 31), (64, 64), (37, 300), (300, 37), (129, 97), (520, 696)]
REACHES = (0, 1, 4, 8)
NP_OF_CODE = {0: np.int64, 1: np.float32, 2: np.int32, 3: np.uint8}
WANTS = ((True, True, True), (True, False, False), (False, True, False), (False, False, True))     # gt, edges, bin
P_BOUND = 1e-12


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "prepare_golden.npz"))


def raw_carve(dev, ids, code, reach, want=WANTS[0]):
    """unet_carve_borders on guarded buffers: [gt, edges, bin] (None where not asked for) and status, as numpy."""
    import _hip
    a = guarded.Arena(dev)
    B, H, W = ids.shape
    x = a.inp(torch.from_numpy(ids.astype(NP_OF_CODE[code])), "ids")
    outs = [a.out((B, H, W), dt, name) if w else None
            for w, dt, name in zip(want, (torch.float32, torch.float32, torch.uint8), ("gt", "edges", "bin"))]
    if outs[2] is not None:
        outs[2].fill_(0x55)              # 0xFF is a value of bin: mark it with one that is not, the guards stay poison
    status = a.out((B,), torch.int64, "status")
    _hip.run("unet_carve_borders", dev, a.ptr(x), code, B, H, W, reach, *(a.ptr(o) for o in outs), a.ptr(status))
    a.verify(outs[0], outs[1], status)
    return [None if o is None else o.cpu().numpy() for o in outs], status.cpu().numpy()


def check_carve(dev, ids, code, reach, want, tag):
    g, e, b, bad = ref.carve_batch(ids, reach)
    got, status = raw_carve(dev, ids, code, reach, want)
    assert status.tolist() == bad.tolist(), tag
    for name, o, w in zip(("gt", "edges", "bin"), got, (g, e, b)):
        assert (o is None) == (not want[("gt", "edges", "bin").index(name)])
        if o is not None:
            assert o.dtype == w.dtype and np.array_equal(o, w), (tag, name)
    return g, e, b


@pytest.mark.parametrize("H,W", SIZES)
def test_carve_equals_the_restatement(dev, H, W):
    """Bit for bit at this size: every kind of id map, with B 1 and 3, the three dtypes and the four patterns of requested outputs
    taking turns: up to 33 x 31 at every reach, above it at two reaches per kind (all four over the kinds), the real frame once
    per kind (the restatement costs up to a second per image there)."""
    seed = 31 * H + W
    big = H * W > 129 * 97
    plan = {"discs": (4,), "discs_hi": (4,), "speckle": (4,), "zeros": (1,), "one": (0,), "two_piece": (4,), "edges": (8,)}
    if not big:                                              # up to 33 x 31 the full cross, above it two reaches per kind
        plan = {kind: REACHES if H * W <= 33 * 31 else (REACHES[k % 4], REACHES[(k + 2) % 4]) for k, kind in enumerate(ref.KINDS)}
    turn = 0
    for k, kind in enumerate(ref.KINDS):
        for reach in plan[kind]:
            B = 3 if (kind == "zeros" if big else turn % 2) else 1
            ids = ref.ids_batch(kind, seed, B, H, W)
            code, want = (k + turn) % 3, WANTS[turn % 4]
            g, e, b = check_carve(dev, ids, code, reach, want, (kind, reach, B, code, want))
            if want != WANTS[0] and not big and reach == 4:
                check_carve(dev, ids, (code + 1) % 3, reach, WANTS[0], (kind, reach, B, "all outputs"))
            turn += 1
            # the inputs do what they are here for
            n = (e // 255).astype(np.int64)
            if kind == "discs_hi" and reach >= 4 and H * W >= 48 * 70:
                assert ((ids > 0) & (n >= 1) & (g > 0)).any() and ((ids > 0) & (g == 0)).any()
            if kind == "speckle" and reach >= 4 and H >= 33 and W >= 31:
                assert n.max() >= 40
            if kind == "two_piece":
                far = max(0, 3 * H // 4 + 1 - reach)         # rows out of the second id's reach: pieces of one id carve nothing
                assert (g[:, :far] == ids[:, :far]).all()


def test_carve_status_and_bad_arguments(dev):
    import _hip
    import data
    ids = ref.ids_batch("discs_hi", 9, 3, 40, 52)
    ids[0, 3, :7] = -1
    ids[0, 20, 20] = 1 << 24
    ids[2, 39, 40:] = -(1 << 31)
    ids[2, 0, 0] = (1 << 24) + 5
    for code in (0, 1, 2):
        g, e, b = check_carve(dev, ids, code, 4, WANTS[0], code)
        assert not g[0, 3, :7].any() and g[0, 20, 20] == 0
    assert ref.carve_batch(ids, 4)[3].tolist() == [8, 0, 13]
    f = ids.astype(np.float32)
    f[1, 5, 5] = np.nan
    _, status = raw_carve(dev, f, 1, 4)
    assert status.tolist() == [8, 1, 13]
    for t in (torch.from_numpy(ids), torch.from_numpy(f)):
        with pytest.raises(ValueError, match="outside"):
            data.preprocess_gt(t.to(dev))
    with pytest.raises(NotImplementedError):
        data.preprocess_gt(torch.from_numpy(ids))
    with pytest.raises(NotImplementedError):
        data.crop_distribution(torch.zeros(50, 50), 36)
    t = torch.zeros(64, dtype=torch.int64, device=dev)
    L = _hip.lib()
    assert L.unet_carve_borders(_hip.ptr(t), 7, 1, 4, 4, 4, _hip.ptr(t), None, None, _hip.ptr(t), None) == -2
    assert b"dtype" in L.unet_last_error()
    assert L.unet_carve_borders(_hip.ptr(t), 0, 1, 4, 4, 9, _hip.ptr(t), None, None, _hip.ptr(t), None) == -2
    assert b"reach" in L.unet_last_error()
    assert L.unet_carve_borders(_hip.ptr(t), 0, 1, 4, 4, 4, None, None, None, _hip.ptr(t), None) == -2
    assert b"at least one" in L.unet_last_error()


def count_masks(H, W, seed):
    """B = 3 masks {0,1}: carved overlapping discs, nothing, and the left third (windows from all foreground to none)"""
    discs = ref.carve_fast(ref.ids_case("discs_hi", seed, H, W))[2] > 0
    half = np.zeros((H, W), bool)
    half[:, :W // 3] = True
    return np.stack([discs, np.zeros((H, W), bool), half])


def raw_counts(dev, mask, code, crop, skip):
    import _hip
    a = guarded.Arena(dev)
    B, H, W = mask.shape
    ny, nx = len(range(0, H - crop, skip)), len(range(0, W - crop, skip))
    m = a.inp(torch.from_numpy(mask), "mask")
    counts = a.out((B, ny, nx), torch.int32, "counts")
    nbytes = _hip.lib().unet_crop_counts_scratch_bytes(B, H, W, crop, skip)
    assert nbytes > 0
    scratch = a.scratch(nbytes, "scratch")
    _hip.run("unet_crop_counts", dev, a.ptr(m), code, B, H, W, crop, skip, a.ptr(counts), a.ptr(scratch))
    a.verify(counts)
    return counts.cpu().numpy()


@pytest.mark.parametrize("H,W,crop,skip", [(40, 52, 36, 10), (40, 52, 39, 10), (41, 41, 40, 10), (96, 120, 36, 10), (96, 120, 60, 7),
                                           (96, 120, 36, 7), (96, 120, 60, 10), (520, 696, 388, 10), (5, 3000, 4, 10)])
def test_crop_counts_equal_the_restatement(dev, H, W, crop, skip):
    """The integers, for the four dtypes (foreground = any non-zero value), and through data.crop_distribution the reference's
    probabilities: same zero pattern, non-zero entries within the derived bound; the empty mask gives the uniform row."""
    import data
    masks = count_masks(H, W, H + W + crop)
    want = np.stack([ref.crop_counts(m, crop, skip) for m in masks])
    if (H, W, crop) == (41, 41, 40):
        assert want.shape == (3, 1, 1)
    values = {0: 255, 1: 0.25, 2: -3, 3: 255}
    for code in (0, 1, 2, 3):
        m = (masks * values[code]).astype(NP_OF_CODE[code])
        got = raw_counts(dev, m, code, crop, skip)
        assert np.array_equal(got, want), code
        pairs, p = data.crop_distribution(torch.from_numpy(m).to(dev), crop, skip)
        assert pairs == ref.crop_pairs(H, W, crop, skip) and p.shape == (3, len(pairs)) and p.dtype == np.float64
        for b in range(3):
            wp = ref.crop_probabilities(want[b], crop)
            assert np.array_equal(p[b] == 0, wp == 0)
            nz = wp != 0
            assert (np.abs(p[b][nz] - wp[nz]) <= P_BOUND * wp[nz]).all()
        assert np.array_equal(p[1], np.full(len(pairs), 1.0 / len(pairs)))
    if len(pairs) >= 20:                                     # some mask has windows inside and outside [0.1, 0.9]
        assert any((wp == 0).any() and (wp != 0).any() for wp in (ref.crop_probabilities(w, crop) for w in want))
    one = data.crop_distribution(torch.from_numpy(masks[0]).to(dev), crop, skip)
    assert one[1].shape == (1, len(pairs)) and np.array_equal(one[1][0], p[0])


def test_crop_counts_bad_arguments(dev):
    import _hip
    import data
    L = _hip.lib()
    t = torch.zeros(4096, dtype=torch.int32, device=dev)
    for H, W, crop, skip, word in ((36, 52, 36, 10, b"no window"), (40, 36, 36, 10, b"no window"), (40, 52, 0, 10, b"at least 1"),
                                   (40, 52, 36, 0, b"at least 1")):
        assert L.unet_crop_counts_scratch_bytes(1, H, W, crop, skip) == 0
        assert L.unet_crop_counts(_hip.ptr(t), 2, 1, H, W, crop, skip, _hip.ptr(t), _hip.ptr(t), None) == -2
        assert word in L.unet_last_error()
    assert L.unet_crop_counts(_hip.ptr(t), 4, 1, 40, 52, 36, 10, _hip.ptr(t), _hip.ptr(t), None) == -2
    assert b"dtype" in L.unet_last_error()
    with pytest.raises(ValueError):
        data.crop_distribution(torch.zeros(36, 52, device=dev), 36)


def check_p(got, want):
    assert got.shape == want.shape and np.array_equal(got == 0, want == 0)
    nz = want != 0
    assert (np.abs(got[nz] - want[nz]) <= P_BOUND * want[nz]).all()


def test_public_path_equals_the_reference(dev, golden):
    """preprocess_gt, binary_target and crop_distribution on the fixture's images as they were born (uint16 in numpy; the
    speckle image int32), single and stacked, against the reference's own outputs; a side stream gives the same."""
    import data
    for name in golden["names"]:
        ids = torch.from_numpy(golden[name + "_ids"]).to(dev)
        gt, mask_global = data.preprocess_gt(ids)
        assert gt.dtype == torch.float32 and mask_global.dtype == torch.float32 and gt.shape == ids.shape
        assert np.array_equal(gt.cpu().numpy(), golden[name + "_gt"])
        assert np.array_equal(mask_global.cpu().numpy(), golden[name + "_mask_global"])
        target = data.binary_target(ids)
        assert target.dtype == torch.uint8 and np.array_equal(target.cpu().numpy(), golden[name + "_bin"])
        for crop in golden[name + "_crops"]:
            pairs, p = data.crop_distribution(target, int(crop))
            assert [list(q) for q in pairs] == golden["%s_pairs%d" % (name, crop)].tolist()
            check_p(p[0], golden["%s_p%d" % (name, crop)])
    names = ("discs", "discs_hi")
    stack = torch.from_numpy(np.stack([golden[n + "_ids"] for n in names])).to(dev)
    assert stack.dtype == torch.uint16

    def run():
        gt, mask_global = data.preprocess_gt(stack)
        target = data.binary_target(stack.long())
        return gt, mask_global, target, data.crop_distribution(target, 36), data.preprocess_gt(stack.double(), kernel=3, iterations=1)

    first = run()
    for k, key in enumerate(("_gt", "_mask_global", "_bin")):
        assert np.array_equal(first[k].cpu().numpy(), np.stack([golden[n + key] for n in names]))
    for b, n in enumerate(names):
        check_p(first[3][1][b], golden[n + "_p36"])
    want1 = ref.carve_batch(stack.cpu().numpy(), 1)
    assert np.array_equal(first[4][0].cpu().numpy(), want1[0]) and np.array_equal(first[4][1].cpu().numpy(), want1[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        second = run()
    s.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first[:3], second[:3])) and np.array_equal(first[3][1], second[3][1])
    with pytest.raises(ValueError):
        data.preprocess_gt(stack, kernel=5, iterations=5)


def test_crop_dataset_draws_augments_and_trains(dev, tmp_path):
    """CropDataset on 4 images of 230 x 250, crop 196 (S = 380), batches of 2: its targets and distribution are the
    restatement's, its draws a host replay's with the same seed, its batches bit-identical to data.augment with those draws;
    and trainer.training runs an epoch of two steps on it."""
    import data
    import network
    import trainer
    N, H, W, crop = 4, 230, 250, 196
    rs = np.random.RandomState(77)
    images = (rs.rand(N, H, W) * 255).astype(np.uint8)
    inst = ref.ids_batch("discs", 21, N, H, W).astype(np.uint16)
    ds = data.CropDataset(images, inst, 3, 10, crop, 2, np.random.RandomState(5), random_state=np.random.RandomState(6))
    assert len(ds) == 2
    want_bin = ref.carve_batch(inst, 4)[2]
    assert ds.target.dtype == torch.uint8 and np.array_equal(ds.target.cpu().numpy(), want_bin)
    assert 0.1 < (want_bin > 0).mean() < 0.95
    assert ds.pairs == ref.crop_pairs(H, W, crop)
    for b in range(N):
        check_p(ds.target_weighted_crop_distribution[b], ref.crop_probabilities(ref.crop_counts(want_bin[b], crop), crop))
    batches = list(ds)
    replay, fields = np.random.RandomState(5), np.random.RandomState(6)
    img, tgt = torch.from_numpy(images).to(dev).float(), torch.from_numpy(want_bin).to(dev)
    for k, (inp, gt) in enumerate(batches):
        idx = [2 * k, 2 * k + 1]
        origins, angles = [], []
        for i in idx:
            origins.append(data.draw_crop(replay, ds.pairs, ds.target_weighted_crop_distribution[i], (H, W), crop))
            angles.append(replay.choice(np.arange(0, 360, 30)))
        assert all(0 <= x <= H - crop and 0 <= y <= W - crop for x, y in origins)
        winp, wgt = data.augment(img[idx], tgt[idx], origins, crop, angles, 3, 10, random_state=fields)
        assert inp.shape == (2, 1, 380, 380) and inp.dtype == torch.float32 and gt.shape == (2, 1, crop, crop) and gt.dtype == torch.int64
        assert torch.equal(inp, winp) and torch.equal(gt, wgt)
        assert 0 < int(gt.sum()) < gt.numel()
    ds = data.CropDataset(images, inst, 3, 10, crop, 2, np.random.RandomState(5), random_state=np.random.RandomState(6))
    net = network.Unet().to(dev)
    trainer.training(net, ds, ds, 0, 2, dev, str(tmp_path), "prepare-test")
    loss = np.loadtxt(os.path.join(str(tmp_path), "progress", "loss.out"))
    loss_val = np.loadtxt(os.path.join(str(tmp_path), "progress", "loss_val.out"))
    assert loss.size == 1 and np.isfinite(loss).all() and np.isfinite(loss_val).all()
