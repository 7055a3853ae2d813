"""The topology-preserving warp and the warping error on the device (functions.warp_labels, functions.warping_error ->
unet_warp_init / unet_warp_sweeps / unet_warp_finish) against the numpy restatement tests/warp_ref.py (pinned to the component
definition, to a sequential warp and to hand-worked answers by tests/test_warp_cpu.py).  Everything is an integer and is compared
bit for bit; warping_error is the same float64 quotient on both sides.  Every pointer handed to the raw entry points is a poisoned
guarded.Arena buffer."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import guarded
import warp_ref as ref
from gpu_support import dev

pytestmark = pytest.mark.gpu

# either side of the 64-pixel tile and of its 16-pixel halo; the 1- and 2-pixel ones have no interior
SIZES = [(1, 1), (1, 40), (2, 2), (3, 3), (5, 7), (33, 31), (64, 64), (63, 65), (65, 63), (129, 97), (257, 255)]
CODE = {torch.int64: 0, torch.float32: 1, torch.int32: 2, torch.uint8: 3}
INTS = ("mismatch", "mismatch_before", "flips")


def raw_warp(dev, gt, pred, reach=None, mask=None, connectivity=4, passes=16, launches=8, dtype=torch.uint8):
    """The three entry points on guarded buffers, with the wrapper's loop: a dict like warp_ref.warp_batch's."""
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = gt.shape
    g, p = a.inp(torch.from_numpy(gt).to(dtype), "gt"), a.inp(torch.from_numpy(pred).to(dtype), "pred")
    m = None if mask is None else a.inp(torch.from_numpy(mask).to(dtype), "mask")
    state = a.out((B, H, W), torch.uint8, "state")
    before, after = a.out((B,), torch.int32, "mismatch_before"), a.out((B,), torch.int32, "mismatch")
    slots = a.out((launches + 2, 4, B), torch.int32, "flips")            # slot 0 and the last one are never named
    scratch = a.scratch(L.unet_warp_scratch_bytes(B, H, W), "scratch")
    warped, mm = a.out((B, H, W), torch.int32, "warped"), a.out((B, H, W), torch.float32, "mismatch_map")
    _hip.run("unet_warp_init", dev, a.ptr(g), CODE[dtype], a.ptr(p), CODE[dtype], a.ptr(m), CODE[dtype], B, H, W,
             -1 if reach is None else ref.dist2(reach), connectivity, a.ptr(state), a.ptr(before), a.ptr(scratch))
    a.verify(before)
    st = state.cpu().numpy()
    assert (st < 8).all()                                    # uint8 poison is a legitimate-looking byte: check the bits instead
    per_sweep = []
    for _ in range(H * W + 2):
        _hip.run("unet_warp_sweeps", dev, a.ptr(state), B, H, W, passes, launches, a.ptr(slots), 1, a.ptr(scratch))
        s = slots.cpu().numpy()
        assert (s[0] == -1).all() and (s[-1] == -1).all() and (s[1:-1] >= 0).all()
        assert not s[1:-1, passes // 4:].any()
        per_sweep.extend(s[1:-1, :passes // 4].reshape(-1, B).astype(np.int64))
        if not s[1:-1].any(axis=(1, 2)).all():
            break
    else:
        raise AssertionError("the warp did not end")
    _hip.run("unet_warp_finish", dev, a.ptr(state), B, H, W, connectivity, a.ptr(warped), a.ptr(mm), a.ptr(after))
    a.verify(warped, mm, after)
    per_sweep = np.stack(per_sweep)
    st2 = state.cpu().numpy()
    assert np.array_equal(st2 & 6, st & 6)                   # T and may never change
    return {"warped": warped.cpu().numpy(), "mismatch_map": mm.cpu().numpy() != 0, "mismatch": after.cpu().numpy().astype(np.int64),
            "mismatch_before": before.cpu().numpy().astype(np.int64), "flips": per_sweep.sum(axis=0),
            "sweeps": int(np.argmin(per_sweep.any(axis=1))) + 1, "may": (st & 4) != 0}


def same(got, want, what):
    for k in ("warped", "mismatch_map", "may") + INTS:
        assert np.array_equal(got[k], want[k]), (what, k)
    assert got["sweeps"] == want["sweeps"], (what, got["sweeps"], want["sweeps"])


def wrapped(dev, gt, pred, reach=None, mask=None, connectivity=4, dtype=torch.uint8, **kw):
    """functions.warp_labels -> a dict like raw_warp's (no may)."""
    import functions
    t = lambda x: None if x is None else torch.from_numpy(x).to(dev).to(dtype)
    warped, c = functions.warp_labels(t(gt), t(pred), reach=reach, mask=t(mask), connectivity=connectivity, **kw)
    assert warped.dtype == torch.int32 and warped.shape == gt.shape and warped.is_cuda and c.mismatch_map.shape == gt.shape
    return {"warped": warped.cpu().numpy(), "mismatch_map": c.mismatch_map.cpu().numpy() != 0, "mismatch": c.mismatch,
            "mismatch_before": c.mismatch_before, "flips": c.flips, "sweeps": c.sweeps}


def same_wrapped(got, want, what):
    for k in ("warped", "mismatch_map") + INTS:
        assert np.array_equal(got[k], want[k]) and (k not in INTS or got[k].dtype == np.int64), (what, k)
    assert got["sweeps"] == want["sweeps"], (what, got["sweeps"], want["sweeps"])


@pytest.mark.parametrize("H,W", SIZES)
def test_warp_equals_the_restatement(dev, H, W):
    """Bit for bit: every kind of image at this size (B 1-4; the batch of four holds an all-background, an all-foreground and a
    gt == pred image next to a busy one), every reach through the raw entry points, both connectivities through
    functions.warp_labels."""
    flips = 0
    small = H * W <= 129 * 97                                # above, the restatement's time decides: two reaches per case
    for k, (name, g, p) in enumerate(ref.size_cases(H, W)):
        reach = ref.REACHES[1 + k % 4]
        for r in ref.REACHES if small else (None, reach):
            want = ref.warp_batch(g, p, r)
            same(raw_warp(dev, g, p, r), want, (name, r))
            flips += int(want["flips"].sum())
        want8 = ref.warp_batch(g, p, reach, connectivity=8)
        same_wrapped(wrapped(dev, g, p, reach, connectivity=8), want8, (name, reach, 8))
        same_wrapped(wrapped(dev, g, p, reach), want if not small else ref.warp_batch(g, p, reach), (name, reach, 4))
        if small:
            same(raw_warp(dev, g, p, reach, connectivity=8), want8, (name, "raw 8"))
    assert flips > 0 or min(H, W) < 3


def test_the_corridor(dev):
    """9 x 400: a stub that grows along a line by two pixels per sweep, 200 sweeps, 50 launches of 16 passes through six tiles."""
    g, p = (x[None].astype(np.uint8) for x in ref.corridor(9, 400))
    want = ref.warp_batch(g, p)
    assert want["sweeps"] == 200 and want["mismatch"].tolist() == [0]
    same(raw_warp(dev, g, p), want, "corridor")
    same_wrapped(wrapped(dev, g[0], p[0]), {k: (v[0] if k in ("warped", "mismatch_map") else v) for k, v in want.items()}, "corridor [H,W]")


@pytest.mark.parametrize("passes", (4, 8, 16))
def test_blocking_and_batching_change_nothing(dev, passes):
    """P passes per launch and any number of launches per round give the result of the passes one by one: the test of the halo,
    of the ping-pong between the two state planes (an odd number of launches ends in the second one) and of the sweep counters."""
    cases = [("corridor",) + tuple(x[None].astype(np.uint8) for x in ref.corridor(9, 400))]
    cases += [c for c in ref.size_cases(129, 97) if c[0] in ("mixed", "serpentine")] + [ref.size_cases(63, 65)[0]]
    for name, g, p in cases:
        want = ref.warp_batch(g, p)
        for launches in (1, 3, 8):
            same(raw_warp(dev, g, p, passes=passes, launches=launches), want, (name, passes, launches))
            same_wrapped(wrapped(dev, g, p, _passes=passes, _launches=launches), want, (name, passes, launches, "wrapper"))


def test_masks(dev):
    """A user mask alone and with a reach, as another dtype than the images."""
    import functions
    name, g, p = ref.size_cases(129, 97)[3]
    rs = np.random.RandomState(12)
    m = (rs.rand(*g.shape) < 0.7).astype(np.uint8) * 3
    m[:, :, 64:] = m[:, ::-1, 64:]
    for reach in (None, 2.5):
        want = ref.warp_batch(g, p, reach, m)
        assert want["flips"].sum() > 0 and (want["flips"] < ref.warp_batch(g, p, reach)["flips"]).any()
        same(raw_warp(dev, g, p, reach, m), want, ("mask", reach))
        t = lambda x, d: torch.from_numpy(x).to(dev).to(d)
        warped, c = functions.warp_labels(t(g, torch.int64), t(p, torch.bool), reach=reach, mask=t(m, torch.float32))
        assert np.array_equal(warped.cpu().numpy(), want["warped"]) and np.array_equal(c.flips, want["flips"])


@pytest.mark.parametrize("dtype", (torch.bool, torch.uint8, torch.int64, torch.float32, torch.int32))
def test_input_dtypes(dev, dtype):
    name, g, p = ref.size_cases(65, 63)[0]
    g, p = g * 7, p * 200                                    # foreground is any value != 0
    want = ref.warp_batch(g, p, 5)
    same_wrapped(wrapped(dev, g, p, 5, dtype=dtype), want, dtype)
    if dtype != torch.bool:
        same(raw_warp(dev, g, p, 5, dtype=dtype), want, dtype)


def test_the_last_interior_row_flips_and_the_border_never(dev):
    """A rectangle two pixels inside the image against an all-foreground prediction grows onto the last interior row and column
    of every side, across tile borders, and stops there."""
    for H, W in ((66, 67), (5, 130)):
        g = np.zeros((1, H, W), np.uint8)
        g[0, 2:H - 2, 2:W - 2] = 1
        p = np.ones((1, H, W), np.uint8)
        want = ref.warp_batch(g, p)
        assert want["warped"][0, 1:-1, 1:-1].all() and want["mismatch"][0] == 2 * H + 2 * W - 4
        got = raw_warp(dev, g, p)
        same(got, want, (H, W))
        edge = ~ref.interior(H, W)
        assert not got["warped"][0][edge].any() and not got["may"][0][edge].any()


def test_warping_error_at_388(dev):
    import functions
    g, p = ref.cells_pair(3, 99, 388, 388)
    g2, p2 = ref.cells_pair(4, 60, 388, 388)
    gt, pred = np.stack([g, g2]), np.stack([p, p2])
    want = ref.scores(pred, gt, reach=5)
    got = functions.warping_error(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), reach=5)
    assert got._fields == ("warping_error", "mismatch", "mismatch_before", "flips", "sweeps", "error_regions", "warping_error_mean")
    for k in INTS + ("error_regions",):
        assert getattr(got, k).dtype == np.int64 and np.array_equal(getattr(got, k), want[k]), k
    assert got.sweeps == want["sweeps"]
    assert got.warping_error.dtype == np.float64 and np.array_equal(got.warping_error, got.mismatch / np.float64(388 * 388))
    assert np.array_equal(got.warping_error, want["warping_error"]) and got.warping_error_mean == want["warping_error_mean"]
    warped, c = functions.warp_labels(torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev), reach=5)
    mm = c.mismatch_map.cpu().numpy() != 0
    assert np.array_equal(mm, warped.cpu().numpy() != pred)
    assert got.error_regions.tolist() == [ndimage.label(m, ref.CROSS)[1] for m in mm]
    assert (got.flips > 0).all() and (got.mismatch > 0).all() and (got.error_regions > 1).all()


def test_errors(dev):
    import _hip
    import functions
    g = torch.zeros(2, 9, 7, dtype=torch.uint8, device=dev)
    with pytest.raises(NotImplementedError):
        functions.warp_labels(g.cpu(), g.cpu())
    with pytest.raises(NotImplementedError):
        functions.warping_error(g, g.cpu())
    with pytest.raises(NotImplementedError):
        functions.warp_labels(g, g, mask=g.cpu())
    with pytest.raises(ValueError, match="equal shape"):
        functions.warp_labels(g, g[:1])
    with pytest.raises(ValueError, match="equal shape"):
        functions.warp_labels(g, g, mask=g[0])
    with pytest.raises(ValueError, match="connectivity"):
        functions.warping_error(g, g, connectivity=6)
    with pytest.raises(ValueError, match="reach"):
        functions.warp_labels(g, g, reach=-1)
    with pytest.raises(ValueError):
        functions.warp_labels(g[0, 0], g[0, 0])
    L = _hip.lib()
    o = torch.zeros(4096, dtype=torch.int32, device=dev)
    q = _hip.ptr(o)
    for passes in (0, 2, 12, 32):
        assert L.unet_warp_sweeps(q, 1, 8, 8, passes, 1, q, 0, q, None) == -2 and b"passes_per_launch" in L.unet_last_error()
    assert L.unet_warp_sweeps(q, 1, 8, 8, 16, 0, q, 0, q, None) == -2
    assert L.unet_warp_sweeps(None, 1, 8, 8, 16, 1, q, 0, q, None) == -2
    assert L.unet_warp_sweeps(q, 1, 8, 8, 16, 1, None, 0, q, None) == -2
    assert L.unet_warp_sweeps(q, 1, 1, 70000, 16, 1, q, 0, q, None) == -2 and b"too large" in L.unet_last_error()
    assert L.unet_warp_init(q, 2, q, 2, None, 0, 1, 70000, 1, -1, 4, q, q, q, None) == -2 and b"too large" in L.unet_last_error()
    assert L.unet_warp_init(q, 2, q, 4, None, 0, 1, 8, 8, -1, 4, q, q, q, None) == -2 and b"dtype" in L.unet_last_error()
    assert L.unet_warp_init(q, 2, q, 2, None, 0, 1, 8, 8, -1, 5, q, q, q, None) == -2 and b"connectivity" in L.unet_last_error()
    assert L.unet_warp_init(q, 2, None, 2, None, 0, 1, 8, 8, -1, 4, q, q, q, None) == -2
    assert L.unet_warp_finish(q, 1, 8, 8, 4, q, None, q, None) == -2
    assert L.unet_warp_finish(q, 1, 8, 8, 7, q, q, q, None) == -2
    assert L.unet_warp_scratch_bytes(0, 8, 8) == 0 and L.unet_warp_scratch_bytes(1, 8, 8) >= 64 * 21
    r = functions.warping_error(g + 1, g)                    # all-foreground prediction, all-background gt: nothing is simple
    assert r.flips.tolist() == [0, 0] and r.mismatch.tolist() == [63, 63] and r.error_regions.tolist() == [1, 1] and r.sweeps == 1
