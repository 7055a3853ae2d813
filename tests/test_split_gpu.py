"""Seeded geodesic growth inside a mask on the device (functions.split_cells -> unet_geodesic_init / unet_geodesic_sweeps /
unet_geodesic_finish; tester.split_instances; tester.segment(split=...)) against the numpy restatement tests/split_ref.py (pinned
to a per-seed dilation distance and to hand-worked answers by tests/test_split_cpu.py, which also asserts that these inputs hold
ties, unreached pixels, seeds outside the mask and walls).  Everything is an integer and is compared bit for bit.  Every pointer
handed to the raw entry points is a poisoned guarded.Arena buffer.

The serpentine is 41 x 400 and not 41 x 200: with a seed at each end of the corridor the largest distance is half its length, and
only rows of 400 take that above 4000 (test_split_cpu.py asserts it); it needs far more launches than one round of 8 either way."""
import functools

import numpy as np
import pytest
import torch

import guarded
import split_ref as ref
from gpu_support import dev, net, image  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CODE = {torch.int64: 0, torch.float32: 1, torch.int32: 2, torch.uint8: 3}
KEYS = ("out", "dist") + ref.INTS
UNSET = 0x5A5A5A5A                                           # int32 poison is -1, which dist legitimately holds: dist starts as this


@functools.lru_cache(maxsize=None)
def cases(H, W):
    return ref.size_cases(H, W)


@functools.lru_cache(maxsize=None)
def want_for(H, W, k, steps):
    name, s, m = cases(H, W)[k]
    return ref.grow_batch(s, m, steps)


def raw_split(dev, seeds, mask, steps=None, launches=8, dtype=torch.uint8):
    """The three entry points on guarded buffers, with the wrapper's loop: a dict like split_ref.grow_batch's, plus "launches"
    (the launches up to and including the first that changed nothing) and "enqueued"."""
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = seeds.shape
    s = a.inp(torch.from_numpy(seeds).to(torch.int32), "seeds")
    m = a.inp(torch.from_numpy(mask).to(dtype), "mask")
    outside, status = a.out((B,), torch.int32, "seeds_outside"), a.out((B,), torch.int64, "status")
    unreached, far = a.out((B,), torch.int32, "unreached"), a.out((B,), torch.int32, "max_dist")
    slots = a.out((launches + 2, B), torch.int32, "changed")             # slot 0 and the last one are never named
    scratch = a.scratch(L.unet_geodesic_scratch_bytes(B, H, W), "scratch")
    out, dist = a.out((B, H, W), torch.int32, "out"), a.out((B, H, W), torch.int32, "dist")
    dist.fill_(UNSET)
    st = -1 if steps is None else steps
    _hip.run("unet_geodesic_init", dev, a.ptr(s), a.ptr(m), CODE[dtype], B, H, W, a.ptr(outside), a.ptr(status), a.ptr(scratch))
    a.verify(outside, status)
    per_launch = []
    for _ in range(H * W + 2):
        _hip.run("unet_geodesic_sweeps", dev, B, H, W, st, launches, a.ptr(slots), 1, a.ptr(scratch))
        c = slots.cpu().numpy()
        assert (c[0] == -1).all() and (c[-1] == -1).all() and (c[1:-1] >= 0).all()
        per_launch.extend(c[1:-1].astype(np.int64))
        if not c[1:-1].any(axis=1).all():
            break
    else:
        raise AssertionError("the growth did not end")
    _hip.run("unet_geodesic_finish", dev, B, H, W, st, a.ptr(out), a.ptr(dist), a.ptr(unreached), a.ptr(far), a.ptr(scratch))
    a.verify(out, unreached, far)
    per_launch = np.stack(per_launch)
    first_idle = int(np.argmin(per_launch.any(axis=1)))
    assert not per_launch[first_idle:].any()                 # a launch that changed nothing: so did every one after it
    d = dist.cpu().numpy()
    assert (d != UNSET).all()
    return {"out": out.cpu().numpy(), "dist": d, "unreached": unreached.cpu().numpy().astype(np.int64),
            "seeds_outside": outside.cpu().numpy().astype(np.int64), "max_dist": far.cpu().numpy().astype(np.int64),
            "status": status.cpu().numpy(), "launches": first_idle + 1, "enqueued": len(per_launch),
            "lowered": per_launch.sum(axis=0)}


def wrapped(dev, seeds, mask, steps=None, dtype=torch.uint8, seed_dtype=torch.int64, **kw):
    """functions.split_cells -> a dict like raw_split's (no status)."""
    import functions
    s, m = torch.from_numpy(seeds).to(dev).to(seed_dtype), torch.from_numpy(mask).to(dev).to(dtype)
    labels, info, dist = functions.split_cells(s, m, max_steps=steps, return_distance=True, **kw)
    assert labels.dtype == torch.int32 and dist.dtype == torch.int32 and labels.shape == seeds.shape == dist.shape and labels.is_cuda
    for v in info[:3]:
        assert v.dtype == np.int64 and v.shape == (seeds.shape[0] if seeds.ndim == 3 else 1,)
    return {"out": labels.cpu().numpy(), "dist": dist.cpu().numpy(), "unreached": info.unreached, "seeds_outside": info.seeds_outside,
            "max_dist": info.max_distance, "launches": info.launches}


def same(got, want, what):
    for k in KEYS:
        if k in got:
            assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("H,W", ref.SIZES)
def test_growth_equals_the_restatement(dev, H, W):
    """Bit for bit: every kind of image at this size (B 1-4; the batch of four holds an image without seeds, one with an empty
    mask and one with a full mask next to a busy one), every max_steps through the raw entry points, int64 seeds through
    functions.split_cells."""
    lowered = 0
    for k, (name, s, m) in enumerate(cases(H, W)):
        for steps in ref.STEPS:
            want = want_for(H, W, k, steps)
            got = raw_split(dev, s, m, steps)
            same(got, want, (name, steps))
            assert np.array_equal(got["lowered"] > 0, want["max_dist"] > 0), (name, steps)
            lowered += int(got["lowered"].sum())
        steps = ref.STEPS[k % 4]
        same(wrapped(dev, s, m, steps), want_for(H, W, k, steps), (name, steps, "wrapper"))
    assert lowered > 0 or H * W < 4
    name, s, m = cases(H, W)[0]
    got = wrapped(dev, s[0], m[0])                            # [H,W]
    assert got["out"].shape == (H, W)
    same(got, {k: (v[0] if k in ("out", "dist") else v[:1]) for k, v in want_for(H, W, 0, None).items()}, "[H,W]")


@pytest.mark.parametrize("dtype", (torch.uint8, torch.int64, torch.float32, torch.int32, torch.bool))
def test_mask_dtypes(dev, dtype):
    name, s, m = cases(65, 63)[2]
    want = want_for(65, 63, 2, None)
    if dtype != torch.bool:
        same(raw_split(dev, s, m, dtype=dtype), want, dtype)
    same(wrapped(dev, s, m, dtype=dtype, seed_dtype=torch.int32), want, (dtype, "wrapper"))
    if dtype == torch.float32:                                # foreground is any value != 0
        import functions
        mf = torch.from_numpy(m).to(dev).float() * -0.25
        labels, info = functions.split_cells(torch.from_numpy(s).to(dev), mf)
        assert np.array_equal(labels.cpu().numpy(), want["out"]) and np.array_equal(info.unreached, want["unreached"])


def test_the_serpentine(dev):
    """41 x 400, one corridor of 8420 pixels with a seed at each end: the growths meet in the middle after 4209 steps, and each
    launch carries them one tile further, seven tiles per row of the corridor: 65 launches, nine rounds of 8."""
    s, m = ref.serpentine()
    want = ref.grow_batch(s, m)
    assert want["max_dist"][0] > 4000 and want["unreached"][0] == 0
    got = raw_split(dev, s, m)
    same(got, want, "serpentine")
    assert got["launches"] > 8 and got["enqueued"] == -(-got["launches"] // 8) * 8
    w = wrapped(dev, s, m)
    same(w, want, "serpentine, wrapper")
    assert w["launches"] == got["launches"]


def test_batching_the_launches_changes_nothing(dev):
    """Any number of launches per call gives the same keys after the same number of launches: the test of the ping-pong between
    the two key planes (an odd number of launches ends in the second one) and of the change counters."""
    for H, W, k in ((129, 97, 3), (63, 65, 0), (257, 255, 1)):
        name, s, m = cases(H, W)[k]
        for steps in (None, 5):
            want = want_for(H, W, k, steps)
            needed = None
            for launches in (1, 3, 8):
                got = raw_split(dev, s, m, steps, launches=launches)
                same(got, want, (name, steps, launches))
                w = wrapped(dev, s, m, steps, _launches=launches)
                same(w, want, (name, steps, launches, "wrapper"))
                needed = got["launches"] if needed is None else needed
                assert got["launches"] == w["launches"] == needed, (name, steps, launches)
                assert got["enqueued"] == -(-needed // launches) * launches, (name, steps, launches)
            assert needed >= 2                                # one launch that lowered keys, one that found nothing to do


def test_determinism(dev):
    """One 257 x 255 busy case five times, once on a side stream: bit-identical."""
    import functions
    name, s, m = cases(257, 255)[0]
    want = want_for(257, 255, 0, None)
    st, mt = torch.from_numpy(s).to(dev), torch.from_numpy(m).to(dev)
    runs = []
    for k in range(5):
        if k == 3:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                labels, info, dist = functions.split_cells(st, mt, return_distance=True)
            torch.cuda.current_stream(dev).wait_stream(side)
        else:
            labels, info, dist = functions.split_cells(st, mt, return_distance=True)
        runs.append((labels.cpu().numpy(), dist.cpu().numpy(), info))
    for labels, dist, info in runs:
        assert np.array_equal(labels, want["out"]) and np.array_equal(dist, want["dist"])
        assert np.array_equal(info.unreached, want["unreached"]) and np.array_equal(info.max_distance, want["max_dist"])
        assert info.launches == runs[0][2].launches


def test_orphans_keep(dev):
    import functions
    for H, W, k in ((129, 97, 3), (65, 63, 1), (5, 7, 2)):
        name, s, m = cases(H, W)[k]
        for steps in (None, 5):
            grown = want_for(H, W, k, steps)
            want = np.stack([ref.keep_orphans(o, sb, mb) for o, sb, mb in zip(grown["out"], s, m)])
            assert (want != grown["out"]).any() and ((want > 0) == (m != 0)).all()
            labels, info = functions.split_cells(torch.from_numpy(s).to(dev), torch.from_numpy(m).to(dev), max_steps=steps, orphans="keep")
            assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want), (name, steps)
            assert np.array_equal(info.unreached, grown["unreached"])                # counted before the orphans got their ids


def test_errors(dev):
    """Every error is raised before any device work; an id of 2^24 through the raw calls is counted and is no seed."""
    import _hip
    import functions
    s = torch.zeros(2, 9, 7, dtype=torch.int32, device=dev)
    host, real = s.cpu(), s.float()
    before = torch.cuda.memory_allocated(dev)
    with pytest.raises(NotImplementedError):
        functions.split_cells(host, s)
    with pytest.raises(NotImplementedError):
        functions.split_cells(s, host)
    with pytest.raises(ValueError, match="equal shape"):
        functions.split_cells(s, s[:1])
    with pytest.raises(ValueError, match="equal shape"):
        functions.split_cells(s[0, 0], s[0, 0])
    with pytest.raises(ValueError, match="max_steps"):
        functions.split_cells(s, s, max_steps=-1)
    with pytest.raises(ValueError, match="orphans"):
        functions.split_cells(s, s, orphans="grow")
    with pytest.raises(ValueError, match="int32 or int64"):
        functions.split_cells(real, s)
    assert torch.cuda.memory_allocated(dev) == before        # nothing was allocated for any of them
    bad = s.clone()
    bad[1, 2, 3] = -1
    with pytest.raises(ValueError, match="negative"):
        functions.split_cells(bad, s)
    bad[1, 2, 3] = 1 << 24
    with pytest.raises(ValueError, match="2\\^24"):
        functions.split_cells(bad, s)
    seeds = np.zeros((1, 3, 5), np.int32)
    seeds[0, 1] = (1 << 24, -3, 0, 0, 6)
    got = raw_split(dev, seeds, np.ones((1, 3, 5), np.uint8))
    want = ref.grow_batch(seeds, np.ones((1, 3, 5), np.uint8))
    same(got, want, "an id of 2^24")
    assert got["status"].tolist() == [2] and set(np.unique(got["out"])) == {6} and got["dist"][0, 1].tolist() == [4, 3, 2, 1, 0]
    L = _hip.lib()
    q = _hip.ptr(torch.zeros(4096, dtype=torch.int32, device=dev))
    assert L.unet_geodesic_sweeps(1, 8, 8, -1, 0, q, 0, q, None) == -2
    assert L.unet_geodesic_init(q, q, 7, 1, 8, 8, q, q, q, None) == -2 and b"dtype" in L.unet_last_error()
    assert L.unet_geodesic_finish(1, 8, 8, -1, q, None, q, q, None, None) == -2


# ---- tester.split_instances and tester.segment(split=...) ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def net3(dev):
    import multiclass_ref
    import network
    m = network.Unet(n_classes=3)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in multiclass_ref.head_params(3).items()})
    return m.to(dev)


def split_by_hand(mask, fg_prob, high):
    """tester.split_instances in numpy: the restatement on the 4-connected components of fg_prob >= high."""
    from scipy import ndimage
    seeds = ndimage.label(fg_prob >= high, ref.CROSS)[0]
    return ref.keep_orphans(ref.grow(seeds, mask)["out"], seeds, mask)


def check_segment(dev, model, fg_of, mask_expected=True, **kw):
    """One 100 x 130 image at tile_size=188; high = the median of the foreground probability over the mask's pixels, which makes
    the seeds a non-empty proper subset of the mask whenever those probabilities vary.  mask_expected: the mask must be
    non-empty and its probabilities must vary, so that the statement is not vacuous.  Where the mask is empty (the seed-0
    two-class net under views='flips', see there) high is the largest probability of the image: every seed is outside the mask."""
    import tester
    x = torch.from_numpy(image(30, 1, 100, 130, blobs=9)[0]).to(dev)
    kw = dict(tile_size=188, max_batch=64, return_probs=True, return_instances=True, **kw)
    m0, p0, i0 = tester.segment(model, x, **kw)
    fg = fg_of(p0)
    inside = fg[m0 != 0]
    varies = inside.numel() > 0 and len(torch.unique(inside)) > 1
    print("mask %d px, %d distinct probabilities on it, largest probability %.6g" % (inside.numel(), len(torch.unique(inside)), float(fg.max())))
    assert varies or not mask_expected
    high = float(inside.median()) if inside.numel() else float(fg.max())
    seeds = (fg >= high) & (m0 != 0)
    assert 0 < high <= 1 and int((fg >= high).sum()) > 0
    if varies:
        assert 0 < int(seeds.sum()) < int((m0 != 0).sum())   # a non-empty proper subset of the mask
    m1, p1, i1 = tester.segment(model, x, split=high, **kw)
    assert torch.equal(m1, m0) and torch.equal(p1, p0)
    assert i1.dtype == torch.int32 and i1.shape == m0.shape
    assert torch.equal(i1, tester.split_instances(m1, fg_of(p1), high))
    assert np.array_equal(i1.cpu().numpy(), split_by_hand(m1.cpu().numpy(), fg_of(p1).cpu().numpy(), np.float32(high)))
    assert ((i1 != 0) == (m1 != 0)).all()                    # orphans='keep': every mask pixel has an id
    del kw["return_probs"]
    m2, i2 = tester.segment(model, x, split=high, **kw)      # the probabilities are formed internally: same mask, same instances
    assert torch.equal(m2, m0) and torch.equal(i2, i1)
    return i0, i1


def test_segment_split(dev, net):
    import tester
    check_segment(dev, net, lambda p: p)
    x = torch.from_numpy(image(31, 1, 100, 130, blobs=9)[0]).to(dev)
    with pytest.raises(ValueError, match="return_instances"):
        tester.segment(net, x, tile_size=188, split=0.7)
    for bad in (0, 1.5, -0.1, "0.5", True):
        with pytest.raises(ValueError, match="split"):
            tester.segment(net, x, tile_size=188, return_instances=True, split=bad)


def test_segment_split_with_views(dev, net):
    """The seed-0 two-class net answers > 0.5 on isolated pixels only (89 of this image's 13000), never on the same pixel in two of
    the four flipped views: the averaged probability stays <= 0.25 and the mask is empty, on this image and on each of 32 others
    that were tried (blobs, noise, inverted, binary, ramps, checkerboards, stripes, a single spike).  So here every seed lies
    outside the mask and the split instance map is all 0 (the three-class net's mask is empty under 'flips' as well); what this
    case holds is that split changes neither mask nor probabilities of a views call and takes its probabilities from it."""
    check_segment(dev, net, lambda p: p, mask_expected=False, views="flips")


def test_segment_split_three_classes(dev, net3):
    check_segment(dev, net3, lambda p: 1 - p[0])
