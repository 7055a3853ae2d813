"""Seeds from the shape of a mask on the device (functions.distance_map -> unet_distance_map; functions.reconstruct ->
unet_reconstruct_init / unet_reconstruct_sweeps / unet_reconstruct_finish; functions.shape_seeds; tester.split_by_shape;
tester.segment(shape_split=...)) against the numpy restatement tests/shape_ref.py (pinned to scipy's distance transform, to a
count of the maxima by their dynamics, to a plateau search and to hand-worked answers by tests/test_shape_cpu.py, which also
asserts that the busy inputs hold a component with two seeds, merged maxima, a seed min_radius drops and a region on the image
edge).  Everything is an integer and is compared bit for bit.  Every pointer handed to the raw entry points is a poisoned
guarded.Arena buffer."""
import functools

import numpy as np
import pytest
import torch

import guarded
import shape_ref as ref
import split_ref
from gpu_support import dev, net, image  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CODE = {torch.int64: 0, torch.float32: 1, torch.int32: 2, torch.uint8: 3}
EDGE = {"ignore": 0, "background": 1}


@functools.lru_cache(maxsize=None)
def cases(H, W):
    return ref.size_cases(H, W)


@functools.lru_cache(maxsize=None)
def want_d2(H, W, k, edge):
    return np.stack([ref.distance2(m, edge) for m in cases(H, W)[k][1]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def want_seeds(H, W, k, h, edge):
    return ref.seeds_batch(cases(H, W)[k][1], h, ref.RADII, edge)


def raw_distance(dev, mask, edge="ignore", dtype=torch.uint8):
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = mask.shape
    m = a.inp(torch.from_numpy(mask).to(dtype), "mask")
    d2 = a.out((B, H, W), torch.int32, "d2")
    scratch = a.scratch(L.unet_distance_map_scratch_bytes(B, H, W), "scratch")
    _hip.run("unet_distance_map", dev, a.ptr(m), CODE[dtype], B, H, W, EDGE[edge], a.ptr(d2), a.ptr(scratch))
    a.verify(d2)
    return d2.cpu().numpy()


def raw_reconstruct(dev, marker, under, mask=None, launches=8, dtype=torch.int64, mask_dtype=torch.uint8):
    """The three entry points on guarded buffers, with the wrapper's loop: a dict like shape_ref.reconstruct_batch's, plus
    "launches" (the launches up to and including the first that raised nothing) and "enqueued"."""
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = marker.shape
    mr, un = a.inp(torch.from_numpy(marker).to(dtype), "marker"), a.inp(torch.from_numpy(under).to(dtype), "under")
    mk = None if mask is None else a.inp(torch.from_numpy(mask).to(mask_dtype), "mask")
    status, raised = a.out((B,), torch.int64, "status"), a.out((B,), torch.int32, "raised")
    slots = a.out((launches + 2, B), torch.int32, "changed")             # slot 0 and the last one are never named
    scratch = a.scratch(L.unet_reconstruct_scratch_bytes(B, H, W), "scratch")
    out = a.out((B, H, W), torch.int32, "out")
    _hip.run("unet_reconstruct_init", dev, a.ptr(mr), CODE[dtype], a.ptr(un), CODE[dtype], a.ptr(mk), CODE[mask_dtype], B, H, W, a.ptr(status),
             a.ptr(scratch))
    a.verify(status)
    per_launch = []
    for _ in range(H * W + 2):
        _hip.run("unet_reconstruct_sweeps", dev, B, H, W, launches, a.ptr(slots), 1, a.ptr(scratch))
        c = slots.cpu().numpy()
        assert (c[0] == -1).all() and (c[-1] == -1).all() and (c[1:-1] >= 0).all()
        per_launch.extend(c[1:-1].astype(np.int64))
        if not c[1:-1].any(axis=1).all():
            break
    else:
        raise AssertionError("the reconstruction did not end")
    _hip.run("unet_reconstruct_finish", dev, B, H, W, a.ptr(out), a.ptr(raised), a.ptr(scratch))
    a.verify(out, raised)
    per_launch = np.stack(per_launch)
    first_idle = int(np.argmin(per_launch.any(axis=1)))
    assert not per_launch[first_idle:].any()                 # a launch that raised nothing: so did every one after it
    return {"out": out.cpu().numpy(), "raised": raised.cpu().numpy().astype(np.int64), "status": status.cpu().numpy(),
            "launches": first_idle + 1, "enqueued": len(per_launch)}


def wrapped_reconstruct(dev, marker, under, mask=None, dtype=torch.int32, **kw):
    import functions
    t = lambda a, d: None if a is None else torch.from_numpy(a).to(dev).to(d)
    out, info = functions.reconstruct(t(marker, dtype), t(under, dtype), mask=t(mask, torch.uint8), **kw)
    assert out.dtype == torch.int32 and out.shape == marker.shape and out.is_cuda
    assert info.raised.dtype == np.int64 and info.raised.shape == (marker.shape[0] if marker.ndim == 3 else 1,)
    return {"out": out.cpu().numpy(), "raised": info.raised, "launches": info.launches}


def same(got, want, what):
    for k in ("out", "raised", "status"):
        if k in got:
            assert np.array_equal(got[k], want[k]), (what, k)


def seeds_on(dev, mask, h, r, edge="ignore", dtype=torch.uint8):
    import functions
    ids, n = functions.shape_seeds(torch.from_numpy(mask).to(dev).to(dtype), h, min_radius=r, edge=edge)
    assert ids.dtype == torch.int32 and n.dtype == torch.int32 and ids.shape == mask.shape and ids.is_cuda
    return ids.cpu().numpy(), n.cpu().numpy()


# ---- the three ops against the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", ref.SIZES)
def test_distance_map_equals_the_restatement(dev, H, W):
    """Bit for bit, both edge rules: every kind of image at this size (B 1-4; the batch of four holds an empty and a full image
    next to busy ones) through the raw entry point, and through functions.distance_map."""
    import functions
    for k, (name, m) in enumerate(cases(H, W)):
        for edge in ref.EDGES:
            want = want_d2(H, W, k, edge)
            assert np.array_equal(raw_distance(dev, m, edge), want), (name, edge)
            got = functions.distance_map(torch.from_numpy(m).to(dev), edge=edge)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (name, edge, "wrapper")
    got = functions.distance_map(torch.from_numpy(m[0]).to(dev))       # [H,W]
    assert got.shape == (H, W) and np.array_equal(got.cpu().numpy(), want_d2(H, W, k, "ignore")[0])
    full = functions.distance_map(torch.ones(2, H, W, dtype=torch.uint8, device=dev)).cpu().numpy()
    assert (full == H * H + W * W).all()


@pytest.mark.parametrize("H,W", ref.SIZES)
def test_reconstruct_equals_the_restatement(dev, H, W):
    """Values, raised and status bit for bit, with and without a mask, B 1-4, int64 through the raw calls and int32 through
    functions.reconstruct."""
    raised = 0
    for B in (1, 2, 4) if H * W <= 129 * 127 else (3,):
        for with_mask in (True, False):
            marker, under, mask = ref.recon_case(H, W, B, with_mask=with_mask)
            want = ref.reconstruct_batch(marker, under, mask)
            got = raw_reconstruct(dev, marker, under, mask)
            same(got, want, (B, with_mask))
            w = wrapped_reconstruct(dev, marker, under, mask)
            same(w, want, (B, with_mask, "wrapper"))
            assert w["launches"] == got["launches"] >= (2 if want["raised"].any() else 1)
            raised += int(want["raised"].sum())
    assert raised > 0 or H * W < 4
    w = wrapped_reconstruct(dev, marker[0], under[0])                  # [H,W], mask=None
    assert w["out"].shape == (H, W)
    same(w, {k: v[:1] if k != "out" else v[0] for k, v in want.items()}, "[H,W]")


@pytest.mark.parametrize("H,W", ref.SIZES)
def test_shape_seeds_equal_the_restatement(dev, H, W):
    """Ids and counts bit for bit: every h and min_radius under 'ignore', h = 2 under 'background'."""
    seen = 0
    for k, (name, m) in enumerate(cases(H, W)):
        for h, edge in [(h, "ignore") for h in ref.HS] + [(2, "background")]:
            for r, (ids, n) in zip(ref.RADII, want_seeds(H, W, k, h, edge)):
                got_ids, got_n = seeds_on(dev, m, h, r, edge)
                assert np.array_equal(got_n, n) and np.array_equal(got_ids, ids), (name, h, r, edge)
                seen += int(n.sum())
    assert seen > 0
    ids, n = seeds_on(dev, m[-1], 2.0, 0)                              # [H,W]
    assert ids.shape == (H, W) and n.shape == (1,) and np.array_equal(ids, want_seeds(H, W, k, 2, "ignore")[0][0][-1])


@pytest.mark.parametrize("dtype", (torch.uint8, torch.int64, torch.float32, torch.int32, torch.bool))
def test_mask_dtypes(dev, dtype):
    import functions
    name, m = cases(65, 66)[1]
    marker, under, _ = ref.recon_case(65, 66, len(m))
    want_r = ref.reconstruct_batch(marker, under, m)
    for edge in ref.EDGES:
        want = want_d2(65, 66, 1, edge)
        if dtype != torch.bool:
            assert np.array_equal(raw_distance(dev, m, edge, dtype), want), (dtype, edge)
        assert np.array_equal(functions.distance_map(torch.from_numpy(m).to(dev).to(dtype), edge=edge).cpu().numpy(), want), (dtype, edge)
    if dtype != torch.bool:
        same(raw_reconstruct(dev, marker, under, m, dtype=torch.int32, mask_dtype=dtype), want_r, dtype)
    out, info = functions.reconstruct(torch.from_numpy(marker).to(dev), torch.from_numpy(under).to(dev), mask=torch.from_numpy(m).to(dev).to(dtype))
    assert np.array_equal(out.cpu().numpy(), want_r["out"]) and np.array_equal(info.raised, want_r["raised"])
    ids, n = want_seeds(65, 66, 1, 2, "ignore")[1]
    got_ids, got_n = seeds_on(dev, m, 2.0, 4, dtype=dtype)
    assert np.array_equal(got_ids, ids) and np.array_equal(got_n, n)
    if dtype == torch.float32:                                # the region is any value != 0
        got = functions.distance_map(torch.from_numpy(m).to(dev).float() * -0.25)
        assert np.array_equal(got.cpu().numpy(), want_d2(65, 66, 1, "ignore"))


def test_the_serpentine(dev):
    """41 x 400, one corridor of 8420 pixels under a flat ceiling with the only high marker on its first pixel: the value
    crosses one tile border per launch, six per row of the corridor, so the launches are what the restatement's walk along the
    corridor counts (128), sixteen rounds of 8."""
    marker, under, mask = ref.serpentine()
    want = ref.reconstruct_batch(marker, under, mask)
    launches = ref.tiled_launches((0, 0), mask[0])
    got = raw_reconstruct(dev, marker, under, mask)
    same(got, want, "serpentine")
    assert got["launches"] == launches > 8 and got["enqueued"] == -(-launches // 8) * 8
    w = wrapped_reconstruct(dev, marker, under, mask)
    same(w, want, "serpentine, wrapper")
    assert w["launches"] == launches


def test_batching_the_launches_changes_nothing(dev):
    """Any number of launches per call gives the same values after the same number of launches: the test of the ping-pong between
    the two planes (an odd number of launches ends in the second one) and of the change counters."""
    for H, W, B in ((129, 127, 2), (63, 64, 1), (257, 255, 1)):
        marker, under, mask = ref.recon_case(H, W, B)
        want = ref.reconstruct_batch(marker, under, mask)
        needed = None
        for launches in (1, 3, 8):
            got = raw_reconstruct(dev, marker, under, mask, launches=launches)
            same(got, want, (H, W, launches))
            w = wrapped_reconstruct(dev, marker, under, mask, _launches=launches)
            same(w, want, (H, W, launches, "wrapper"))
            needed = got["launches"] if needed is None else needed
            assert got["launches"] == w["launches"] == needed, (H, W, launches)
            assert got["enqueued"] == -(-needed // launches) * launches, (H, W, launches)
        assert needed >= 2                                    # one launch that raised values, one that found nothing to do


def test_determinism(dev):
    """One 257 x 255 busy case five times, once on a side stream: bit-identical."""
    import functions
    name, m = cases(257, 255)[0]
    ids, n = want_seeds(257, 255, 0, 2, "ignore")[0]
    mt = torch.from_numpy(m).to(dev)
    runs = []
    for k in range(5):
        if k == 3:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                got = functions.shape_seeds(mt, 2.0)
            torch.cuda.current_stream(dev).wait_stream(side)
        else:
            got = functions.shape_seeds(mt, 2.0)
        runs.append((got[0].cpu().numpy(), got[1].cpu().numpy()))
    for got_ids, got_n in runs:
        assert np.array_equal(got_ids, ids) and np.array_equal(got_n, n)


def test_the_element_wise_steps(dev):
    """unet_shape_heights, unet_shape_lower and unet_shape_maxima on guarded buffers: the exact integer square root at the values
    where an fp64 root is one off or the argument is largest, the lift, the cut at 0, the compare and the floor."""
    import _hip
    a = guarded.Arena(dev)
    d2 = np.concatenate([np.arange(0, 3000), np.arange(1, 46341, dtype=np.int64)[-1500:] ** 2, np.arange(1, 46341, dtype=np.int64)[-1500:] ** 2 - 1,
                         [2 ** 31 - 1, 2 * 32767 ** 2]]).astype(np.int32)
    d2 = d2[:len(d2) // 7 * 7].reshape(1, 7, -1)
    B, H, W = d2.shape
    src = a.inp(torch.from_numpy(d2), "d2")
    q, lifted = a.out((B, H, W), torch.int32, "q"), a.out((B, H, W), torch.int32, "lifted")
    _hip.run("unet_shape_heights", dev, a.ptr(src), B, H, W, 37, a.ptr(q), a.ptr(lifted))
    a.verify(q, lifted)
    want = ref.isqrt256(d2)
    assert np.array_equal(q.cpu().numpy(), want) and np.array_equal(lifted.cpu().numpy(), want + 37)
    low = a.out((B, H, W), torch.int32, "lowered")
    _hip.run("unet_shape_lower", dev, a.ptr(q), B, H, W, 1000, a.ptr(low))
    a.verify(low)
    assert np.array_equal(low.cpu().numpy(), np.maximum(want - 1000, 0)) and (want < 1000).any()
    peaks = a.out((B, H, W), torch.float32, "peaks")
    _hip.run("unet_shape_maxima", dev, a.ptr(lifted), a.ptr(q), B, H, W, 5000, a.ptr(peaks))      # q < lifted everywhere
    a.verify(peaks)
    assert np.array_equal(peaks.cpu().numpy(), (want + 37 >= 5000).astype(np.float32))
    _hip.run("unet_shape_maxima", dev, a.ptr(q), a.ptr(q), B, H, W, 0, a.ptr(peaks))
    assert not peaks.cpu().numpy().any()


def test_errors(dev):
    import functions
    m = torch.ones(2, 9, 7, dtype=torch.uint8, device=dev)
    v = torch.zeros(2, 9, 7, dtype=torch.int32, device=dev)
    for host in (m.cpu(), np.ones((9, 7), np.uint8)):
        with pytest.raises(NotImplementedError):
            functions.distance_map(host)
        with pytest.raises(NotImplementedError):
            functions.shape_seeds(host)
    for args in ((v.cpu(), v), (v, v.cpu())):
        with pytest.raises(NotImplementedError):
            functions.reconstruct(*args)
    with pytest.raises(NotImplementedError):
        functions.reconstruct(v, v, mask=m.cpu())
    with pytest.raises(ValueError, match="edge"):
        functions.distance_map(m, edge="reflect")
    with pytest.raises(ValueError, match="edge"):
        functions.shape_seeds(m, edge="reflect")
    for bad in (-1, "2", True, float("nan")):
        with pytest.raises(ValueError, match="h must"):
            functions.shape_seeds(m, bad)
    with pytest.raises(ValueError, match="min_radius"):
        functions.shape_seeds(m, 2.0, min_radius=-1)
    with pytest.raises(ValueError, match="32767"):            # over the limit: a squared distance would not fit
        functions.distance_map(torch.ones(1, 32768, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="32767"):
        functions.shape_seeds(torch.ones(32768, 1, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="32767"):
        functions.reconstruct(torch.zeros(1, 32768, dtype=torch.int32, device=dev), torch.zeros(1, 32768, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="equal shape"):
        functions.reconstruct(v, v[:1])
    with pytest.raises(ValueError, match="equal shape"):
        functions.reconstruct(v, v, mask=m[:, :8])
    with pytest.raises(ValueError, match="int32 or int64"):
        functions.reconstruct(v.float(), v)
    with pytest.raises(ValueError, match="_launches"):
        functions.reconstruct(v, v, _launches=0)
    # values out of range: counted by the kernel, raised by the wrapper; through the raw calls such a value counts as 0
    marker = np.zeros((2, 9, 7), np.int64)
    under = np.full((2, 9, 7), 5, np.int64)
    marker[1, 2, 3], marker[1, 4, 4], under[0, 0, 0] = ref.TOP + 1, -1, -7
    with pytest.raises(ValueError, match="outside"):
        functions.reconstruct(torch.from_numpy(marker).to(dev), torch.from_numpy(under).to(dev))
    got = raw_reconstruct(dev, marker, under)
    same(got, ref.reconstruct_batch(marker, under), "out of range")
    assert got["status"].tolist() == [1, 2]
    marker[1, 2, 3], marker[1, 4, 4], under[0, 0, 0] = ref.TOP, 0, 5   # the largest value there is, and no mask
    want = ref.reconstruct_batch(marker, under)
    same(wrapped_reconstruct(dev, marker, under, dtype=torch.int64), want, "2^30")
    assert (want["out"][1] == 5).all() and want["raised"].tolist() == [0, 62]


# ---- tester.split_by_shape and tester.segment(shape_split=...) -----------------------------------------------------------------

def split_by_hand(mask, h=2.0, min_radius=0.0, edge="ignore"):
    """tester.split_by_shape in numpy: the growth's restatement on the restatement's seeds."""
    seeds = ref.seeds(mask, h, min_radius, edge)[0]
    return split_ref.keep_orphans(split_ref.grow(seeds, mask)["out"], seeds, mask)


def test_split_by_shape(dev):
    import functions
    import tester
    two = (ref.disc(64, 72, 30, 25, 12) | ref.disc(64, 72, 30, 45, 12)).astype(np.uint8)
    t = torch.from_numpy(two).to(dev)
    got = tester.split_by_shape(t)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), split_by_hand(two))
    assert int(functions.label_cells(t)[1]) == 1 and sorted(np.unique(got.cpu().numpy())) == [0, 1, 2]
    assert sorted(np.unique(tester.split_by_shape(t, 5.0).cpu().numpy())) == [0, 1]
    name, m = cases(129, 127)[1]
    for kw in ({}, {"h": 0.5, "min_radius": 4}, {"edge": "background"}):
        got = tester.split_by_shape(torch.from_numpy(m).to(dev), **kw).cpu().numpy()
        assert np.array_equal(got, np.stack([split_by_hand(x, **kw) for x in m])), kw
        assert ((got != 0) == (m != 0)).all()                 # orphans='keep': every mask pixel has an id


def check_segment(dev, model, mask_expected=True, **kw):
    import tester
    x = torch.from_numpy(image(30, 1, 100, 130, blobs=9)[0]).to(dev)
    kw = dict(tile_size=188, max_batch=64, return_instances=True, **kw)
    m0, i0 = tester.segment(model, x, **kw)
    print("mask %d px, %d components" % (int((m0 != 0).sum()), int(i0.max())))
    assert bool((m0 != 0).any()) or not mask_expected
    for value, args in ((2.0, (2.0, 0.0)), ((0.5, 3), (0.5, 3.0)), (0, (0.0, 0.0))):
        m1, i1 = tester.segment(model, x, shape_split=value, **kw)
        assert torch.equal(m1, m0) and i1.dtype == torch.int32 and i1.shape == m0.shape
        assert torch.equal(i1, tester.split_by_shape(m1, *args))
        assert np.array_equal(i1.cpu().numpy(), split_by_hand(m1.cpu().numpy(), *args))
        assert ((i1 != 0) == (m1 != 0)).all()
        assert int(i1.max()) >= int(i0.max())                 # a split only adds cells


def test_segment_shape_split(dev, net):
    import tester
    check_segment(dev, net)
    x = torch.from_numpy(image(31, 1, 100, 130, blobs=9)[0]).to(dev)
    with pytest.raises(ValueError, match="return_instances"):
        tester.segment(net, x, tile_size=188, shape_split=2.0)
    with pytest.raises(ValueError, match="shape_split"):
        tester.segment(net, x, tile_size=188, return_instances=True, split=0.7, shape_split=2.0)
    for bad in (-1, "2", True, (2.0,), (2.0, -1), (2.0, 1, 1), (2.0, "1")):
        with pytest.raises(ValueError, match="shape_split"):
            tester.segment(net, x, tile_size=188, return_instances=True, shape_split=bad)


def test_segment_shape_split_with_views(dev, net):
    """The seed-0 two-class net leaves an empty mask under views='flips' (tests/test_split_gpu.py has the reason), so what this
    case holds is that shape_split runs after a views call, changes no mask and returns an instance map without ids."""
    check_segment(dev, net, mask_expected=False, views="flips")
