"""The 8-connected seeded sweeps on the device (unet_geodesic_sweeps_conn, unet_flood_sweeps_conn, unet_flood_assign_conn,
unet_reconstruct_sweeps_conn; functions.split_cells / watershed / reconstruct / shape_seeds and tester.split_instances /
split_by_shape / split_by_watershed / segment with connectivity=8) against the numpy restatement tests/conn_ref.py, which
tests/test_conn_cpu.py pins (and which it shows to differ between 4 and 8 on these inputs).  Everything is an integer and is
compared bit for bit.  Every pointer handed to the raw entry points is a poisoned guarded.Arena buffer."""
import functools

import numpy as np
import pytest
import torch

import conn_ref as ref
import flood_ref
import guarded
import shape_ref
import split_ref
from gpu_support import dev, net, image  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CODE = {torch.int64: 0, torch.float32: 1, torch.int32: 2, torch.uint8: 3}
UNSET = 0x5A5A5A5A                                           # int32 poison is -1, which the distance maps legitimately hold
GROW_KEYS = ("out", "dist") + split_ref.INTS
FLOOD_KEYS = flood_ref.MAPS + flood_ref.INTS


def same(got, want, keys, what):
    for k in keys:
        if k in got:
            assert np.array_equal(got[k], want[k]), (what, k)


def sweep(a, dev, entry, before, scratch, B, launches, limit):
    """A _conn sweep entry on guarded slots to its first idle launch -> (launches needed, launches enqueued, moved per image)."""
    import _hip
    slots = a.out((launches + 2, B), torch.int32, "changed")              # slot 0 and the last one are never named
    per_launch = []
    for _ in range(limit):
        _hip.run(entry, dev, *before, launches, a.ptr(slots), 1, a.ptr(scratch))
        c = slots.cpu().numpy()
        assert (c[0] == -1).all() and (c[-1] == -1).all() and (c[1:-1] >= 0).all()
        per_launch.extend(c[1:-1].astype(np.int64))
        if not c[1:-1].any(axis=1).all():
            break
    else:
        raise AssertionError("%s did not end" % entry)
    per_launch = np.stack(per_launch)
    first_idle = int(np.argmin(per_launch.any(axis=1)))
    assert not per_launch[first_idle:].any()                 # a launch that changed nothing: so did every one after it
    return first_idle + 1, len(per_launch), per_launch.sum(axis=0)


# ---- growth -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grow_cases(H, W):
    return split_ref.size_cases(H, W)


@functools.lru_cache(maxsize=None)
def grow_want(H, W, k, steps, conn=8):
    name, s, m = grow_cases(H, W)[k]
    return ref.grow_batch(s, m, steps, conn)


def raw_split(dev, seeds, mask, steps=None, conn=8, launches=8, entry="unet_geodesic_sweeps_conn"):
    """init, the sweep entry and finish on guarded buffers -> a dict like conn_ref.grow_batch's, plus launches and enqueued."""
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = seeds.shape
    s = a.inp(torch.from_numpy(seeds).to(torch.int32), "seeds")
    m = a.inp(torch.from_numpy(mask).to(torch.uint8), "mask")
    outside, status = a.out((B,), torch.int32, "seeds_outside"), a.out((B,), torch.int64, "status")
    unreached, far = a.out((B,), torch.int32, "unreached"), a.out((B,), torch.int32, "max_dist")
    scratch = a.scratch(L.unet_geodesic_scratch_bytes(B, H, W), "scratch")
    out, dist = a.out((B, H, W), torch.int32, "out"), a.out((B, H, W), torch.int32, "dist")
    dist.fill_(UNSET)
    st = -1 if steps is None else steps
    _hip.run("unet_geodesic_init", dev, a.ptr(s), a.ptr(m), 3, B, H, W, a.ptr(outside), a.ptr(status), a.ptr(scratch))
    before = (B, H, W, st) + (() if entry == "unet_geodesic_sweeps" else (conn,))
    needed, enqueued, lowered = sweep(a, dev, entry, before, scratch, B, launches, H * W + 2)
    _hip.run("unet_geodesic_finish", dev, B, H, W, st, a.ptr(out), a.ptr(dist), a.ptr(unreached), a.ptr(far), a.ptr(scratch))
    a.verify(out, unreached, far, outside, status)
    d = dist.cpu().numpy()
    assert (d != UNSET).all()
    return {"out": out.cpu().numpy(), "dist": d, "unreached": unreached.cpu().numpy().astype(np.int64),
            "seeds_outside": outside.cpu().numpy().astype(np.int64), "max_dist": far.cpu().numpy().astype(np.int64),
            "status": status.cpu().numpy(), "launches": needed, "enqueued": enqueued, "lowered": lowered}


def wrapped_split(dev, seeds, mask, steps=None, conn=8, **kw):
    import functions
    s, m = torch.from_numpy(seeds).to(dev).to(torch.int64), torch.from_numpy(mask).to(dev)
    labels, info, dist = functions.split_cells(s, m, max_steps=steps, return_distance=True, connectivity=conn, **kw)
    assert labels.dtype == torch.int32 and dist.dtype == torch.int32 and labels.shape == seeds.shape == dist.shape
    return {"out": labels.cpu().numpy(), "dist": dist.cpu().numpy(), "unreached": info.unreached, "seeds_outside": info.seeds_outside,
            "max_dist": info.max_distance, "launches": info.launches}


@pytest.mark.parametrize("H,W", ref.GROW_SIZES)
def test_growth_equals_the_restatement(dev, H, W):
    """Bit for bit at connectivity 8: every kind of image at this size and every max_steps through the raw _conn entry, one case
    through functions.split_cells; and connectivity 4 through the _conn entry is the entry without it."""
    for k, (name, s, m) in enumerate(grow_cases(H, W)):
        for steps in split_ref.STEPS:
            got = raw_split(dev, s, m, steps)
            same(got, grow_want(H, W, k, steps), GROW_KEYS, (name, steps))
            assert np.array_equal(got["lowered"] > 0, grow_want(H, W, k, steps)["max_dist"] > 0), (name, steps)
    k = len(grow_cases(H, W)) - 1
    name, s, m = grow_cases(H, W)[k]
    steps = split_ref.STEPS[(H + W) % 4]
    same(wrapped_split(dev, s, m, steps), grow_want(H, W, k, steps), GROW_KEYS, (name, steps, "wrapper"))
    old, new = raw_split(dev, s, m, None, entry="unet_geodesic_sweeps"), raw_split(dev, s, m, None, conn=4)
    same(new, old, GROW_KEYS + ("launches", "lowered"), (name, "4 through the _conn entry"))
    same(new, grow_want(H, W, k, None, 4), GROW_KEYS, (name, "4"))


def test_growth_across_tile_corners(dev):
    """The diagonal corridor and its mirror image (every step diagonal, two of them across a tile corner), the checkerboard
    (corners only), and the two-pixel regions at the four corners of the tile at (64, 64), along both diagonals."""
    for mirror in (False, True):
        s, m = ref.eye_corridor(mirror=mirror)
        got = raw_split(dev, s, m)
        same(got, ref.grow_batch(s, m, None, 8), GROW_KEYS, ("corridor", mirror))
        assert got["unreached"][0] == 0 and got["max_dist"][0] == 64 and got["launches"] >= 3
        same(raw_split(dev, s, m, conn=4), ref.grow_batch(s, m, None, 4), GROW_KEYS, ("corridor at 4", mirror))
    s, m = ref.checkerboard()
    got = raw_split(dev, s, m)
    same(got, ref.grow_batch(s, m, None, 8), GROW_KEYS, "checkerboard")
    assert got["unreached"][0] == 0 and got["max_dist"][0] == 66
    same(wrapped_split(dev, s, m, conn=4), ref.grow_batch(s, m, None, 4), GROW_KEYS, "checkerboard at 4")
    s, m = ref.corner_pairs()
    got = raw_split(dev, s, m)
    same(got, ref.grow_batch(s, m, None, 8), GROW_KEYS, "corner pairs")
    assert (got["unreached"] == 0).all() and (got["max_dist"] == 1).all()
    s, m = ref.diagonal_tie()
    assert wrapped_split(dev, s[None], m[None])["out"][0].tolist() == [[7, 7, 3], [7, 3, 3], [3, 3, 3]]


def test_orphans_keep(dev):
    import functions
    for H, W, k in ((129, 97, 3), (65, 63, 1), (5, 7, 2)):
        name, s, m = grow_cases(H, W)[k]
        for steps in (None, 5):
            grown = grow_want(H, W, k, steps)
            want = np.stack([ref.keep_orphans(o, sb, mb, 8) for o, sb, mb in zip(grown["out"], s, m)])
            want4 = np.stack([ref.keep_orphans(o, sb, mb, 4) for o, sb, mb in zip(grown["out"], s, m)])
            assert (want != grown["out"]).any() and ((want > 0) == (m != 0)).all() and (H * W < 64 or (want != want4).any())
            labels, info = functions.split_cells(torch.from_numpy(s).to(dev), torch.from_numpy(m).to(dev), max_steps=steps, orphans="keep",
                                                 connectivity=8)
            assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want), (name, steps)
            assert np.array_equal(info.unreached, grown["unreached"])


# ---- flood ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def flood_cases(H, W):
    return flood_ref.size_cases(H, W)


@functools.lru_cache(maxsize=None)
def flood_want(H, W, k, top, conn=8):
    name, s, im, m = flood_cases(H, W)[k]
    return ref.flood_batch(s, im, m, max_level=top, connectivity=conn)


def raw_flood(dev, seeds, image_, mask, top=None, conn=8, launches=8):
    """The four entry points on guarded buffers -> a dict like conn_ref.flood_batch's, plus launches (a pair) and enqueued."""
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = seeds.shape
    s = a.inp(torch.from_numpy(seeds).to(torch.int32), "seeds")
    im = a.inp(torch.from_numpy(image_).to(torch.int32), "image")
    m = None if mask is None else a.inp(torch.from_numpy(mask).to(torch.uint8), "mask")
    outside, status = a.out((B,), torch.int32, "seeds_outside"), a.out((2, B), torch.int64, "status")
    unreached, high = a.out((B,), torch.int32, "unreached"), a.out((B,), torch.int32, "max_level")
    scratch = a.scratch(L.unet_flood_scratch_bytes(B, H, W), "scratch")
    out, lev, dist = (a.out((B, H, W), torch.int32, k) for k in ("out", "pass_level", "dist"))
    lev.fill_(UNSET)
    dist.fill_(UNSET)
    t = -1 if top is None else top
    _hip.run("unet_flood_init", dev, a.ptr(s), a.ptr(im), 2, 0, a.ptr(m), 3, B, H, W, a.ptr(outside), a.ptr(status), a.ptr(scratch))
    n1, e1, _ = sweep(a, dev, "unet_flood_sweeps_conn", (B, H, W, t, conn), scratch, B, launches, H * W + 2)
    n2, e2, _ = sweep(a, dev, "unet_flood_assign_conn", (B, H, W, conn), scratch, B, launches, H * W + 2)
    _hip.run("unet_flood_finish", dev, B, H, W, a.ptr(out), a.ptr(lev), a.ptr(dist), a.ptr(unreached), a.ptr(high), a.ptr(scratch))
    a.verify(out, unreached, high, outside, status)
    lv, d = lev.cpu().numpy(), dist.cpu().numpy()
    assert (lv != UNSET).all() and (d != UNSET).all()
    st = status.cpu().numpy()
    return {"out": out.cpu().numpy(), "pass_level": lv, "dist": d, "unreached": unreached.cpu().numpy().astype(np.int64),
            "seeds_outside": outside.cpu().numpy().astype(np.int64), "max_level": high.cpu().numpy().astype(np.int64),
            "status": st[0], "bad_values": st[1], "launches": (n1, n2), "enqueued": (e1, e2)}


def wrapped_flood(dev, seeds, image_, mask, top=None, conn=8, **kw):
    import functions
    t = lambda x: None if x is None else torch.from_numpy(x).to(dev)
    labels, info, lev, dist = functions.watershed(t(seeds), t(image_), mask=t(mask), max_level=top, return_levels=True, connectivity=conn, **kw)
    assert labels.dtype == torch.int32 and labels.shape == seeds.shape
    return {"out": labels.cpu().numpy(), "pass_level": lev.cpu().numpy(), "dist": dist.cpu().numpy(), "unreached": info.unreached,
            "seeds_outside": info.seeds_outside, "max_level": info.max_level, "launches": info.launches}


@pytest.mark.parametrize("H,W", ref.FLOOD_SIZES)
def test_flood_equals_the_restatement(dev, H, W):
    """Bit for bit at connectivity 8: every image of flood_ref.size_cases at this size (every kind of landscape), without and
    with a max_level, through the raw _conn entries; one case through functions.watershed; 4 through the _conn entries."""
    for k, (name, s, im, m) in enumerate(flood_cases(H, W)):
        for top in (None, 2):
            same(raw_flood(dev, s, im, m, top), flood_want(H, W, k, top), FLOOD_KEYS, (name, top))
    k = len(flood_cases(H, W)) - 1
    name, s, im, m = flood_cases(H, W)[k]
    same(wrapped_flood(dev, s, im, m), flood_want(H, W, k, None), FLOOD_KEYS, (name, "wrapper"))
    same(raw_flood(dev, s, im, m, conn=4), flood_ref.flood_batch(s, im, m), FLOOD_KEYS, (name, "4 through the _conn entries"))


def test_flood_by_hand(dev):
    """A constant image gives split_cells(connectivity=8); the membrane leaks at 8 and holds at 4; the corridor under a ramp has
    parent links across a tile corner (tests/test_conn_cpu.py asserts that it has two)."""
    import functions
    for H, W in ((33, 31), (65, 63)):
        s, m = split_ref.busy(H, W)
        st, mt = torch.from_numpy(s).to(dev), torch.from_numpy(m).to(dev)
        grown, _, gd = functions.split_cells(st, mt, return_distance=True, connectivity=8)
        flooded, _, lev, fd = functions.watershed(st, torch.full((H, W), 3, dtype=torch.int32, device=dev), mask=mt, return_levels=True,
                                                  connectivity=8)
        assert torch.equal(grown, flooded) and torch.equal(gd[gd > 0], fd[gd > 0])
        assert np.array_equal(grown.cpu().numpy(), ref.grow(s, m, None, 8)["out"])
    s, im = ref.membrane()
    far = np.add.outer(np.arange(8), np.arange(8)) > 7
    for conn, level in ((4, 9), (8, 0)):
        got = raw_flood(dev, s[None], im[None], None, conn=conn)
        same(got, ref.flood_batch(s[None], im[None], connectivity=conn), FLOOD_KEYS, ("membrane", conn))
        assert (got["pass_level"][0][far] == level).all()
    s, im, m = ref.corner_flood()
    got = raw_flood(dev, s, im, m)
    same(got, ref.flood_batch(s, im, m, connectivity=8), FLOOD_KEYS, "corner flood")
    assert got["unreached"][0] == 0 and got["launches"][1] >= 3


# ---- reconstruction and seeds -----------------------------------------------------------------------------------------------

def raw_reconstruct(dev, marker, under, mask, conn=8, launches=8):
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = marker.shape
    mr, un = a.inp(torch.from_numpy(marker), "marker"), a.inp(torch.from_numpy(under).to(torch.int32), "under")
    m = None if mask is None else a.inp(torch.from_numpy(mask), "mask")
    status, raised = a.out((B,), torch.int64, "status"), a.out((B,), torch.int32, "raised")
    scratch = a.scratch(L.unet_reconstruct_scratch_bytes(B, H, W), "scratch")
    out = a.out((B, H, W), torch.int32, "out")
    _hip.run("unet_reconstruct_init", dev, a.ptr(mr), 0, a.ptr(un), 2, a.ptr(m), 3, B, H, W, a.ptr(status), a.ptr(scratch))
    needed, enqueued, _ = sweep(a, dev, "unet_reconstruct_sweeps_conn", (B, H, W, conn), scratch, B, launches, H * W + 2)
    _hip.run("unet_reconstruct_finish", dev, B, H, W, a.ptr(out), a.ptr(raised), a.ptr(scratch))
    a.verify(out, raised, status)
    return {"out": out.cpu().numpy(), "raised": raised.cpu().numpy().astype(np.int64), "status": status.cpu().numpy(),
            "launches": needed, "enqueued": enqueued}


@functools.lru_cache(maxsize=None)
def recon_want(H, W, with_mask, conn=8):
    return ref.reconstruct_batch(*shape_ref.recon_case(H, W, 2, with_mask=with_mask), conn)


@pytest.mark.parametrize("H,W", ref.RECON_SIZES)
def test_reconstruction_equals_the_restatement(dev, H, W):
    import functions
    for with_mask in (True, False):
        marker, under, mask = shape_ref.recon_case(H, W, 2, with_mask=with_mask)
        want = recon_want(H, W, with_mask)
        same(raw_reconstruct(dev, marker, under, mask), want, ("out", "raised", "status"), (with_mask, "raw"))
        t = lambda x: None if x is None else torch.from_numpy(x).to(dev)
        R, info = functions.reconstruct(t(marker), t(under), mask=t(mask), connectivity=8)
        assert R.dtype == torch.int32 and np.array_equal(R.cpu().numpy(), want["out"]) and np.array_equal(info.raised, want["raised"])
    same(raw_reconstruct(dev, marker, under, mask, conn=4), shape_ref.reconstruct_batch(marker, under, mask), ("out", "raised", "status"),
         "4 through the _conn entry")


def test_seeds_on_the_diagonal_discs(dev):
    import functions
    m = torch.from_numpy(ref.diagonal_discs()).to(dev)
    for conn, counts in ((8, [2, 2, 2, 2]), (4, [9, 3, 2, 2])):
        got = [functions.shape_seeds(m, h, connectivity=conn) for h in ref.DISC_HS]
        assert [int(n) for _, n in got] == counts
        for h, (ids, n) in zip(ref.DISC_HS, got):
            assert np.array_equal(ids.cpu().numpy(), ref.seeds(ref.diagonal_discs(), h, connectivity=conn)[0]), (conn, h)


@pytest.mark.parametrize("H,W", ref.SEED_SIZES)
def test_seeds_equal_the_restatement(dev, H, W):
    import functions
    for name, masks in shape_ref.size_cases(H, W)[-2:]:
        for h in ref.SEED_HS:
            ids, n = functions.shape_seeds(torch.from_numpy(masks).to(dev), h, connectivity=8)
            want, wn = ref.seeds_batch(masks, h, connectivity=8)
            assert ids.dtype == torch.int32 and np.array_equal(ids.cpu().numpy(), want) and np.array_equal(n.cpu().numpy(), wn), (name, h)


# ---- launches, determinism, errors ------------------------------------------------------------------------------------------

def test_batching_the_launches_changes_nothing(dev):
    """Any number of launches per call gives the same result after the same number of launches, in each of the four sweeps."""
    name, s, m = grow_cases(129, 97)[3]
    needed = None
    for launches in (1, 3, 8):
        got, w = raw_split(dev, s, m, launches=launches), wrapped_split(dev, s, m, _launches=launches)
        same(got, grow_want(129, 97, 3, None), GROW_KEYS, (name, launches))
        same(w, grow_want(129, 97, 3, None), GROW_KEYS, (name, launches, "wrapper"))
        needed = got["launches"] if needed is None else needed
        assert got["launches"] == w["launches"] == needed >= 2 and got["enqueued"] == -(-needed // launches) * launches
    name, s, im, m = flood_cases(65, 63)[3]
    needed = None
    for launches in (1, 3, 8):
        got, w = raw_flood(dev, s, im, m, launches=launches), wrapped_flood(dev, s, im, m, _launches=launches)
        same(got, flood_want(65, 63, 3, None), FLOOD_KEYS, (name, launches))
        same(w, flood_want(65, 63, 3, None), FLOOD_KEYS, (name, launches, "wrapper"))
        needed = got["launches"] if needed is None else needed
        assert got["launches"] == tuple(w["launches"]) == needed and min(needed) >= 2
        assert got["enqueued"] == tuple(-(-n // launches) * launches for n in needed)
    import functions
    marker, under, mask = shape_ref.recon_case(129, 127, 2)
    needed = None
    for launches in (1, 3, 8):
        got = raw_reconstruct(dev, marker, under, mask, launches=launches)
        same(got, recon_want(129, 127, True), ("out", "raised", "status"), ("reconstruct", launches))
        R, info = functions.reconstruct(torch.from_numpy(marker).to(dev), torch.from_numpy(under).to(dev), mask=torch.from_numpy(mask).to(dev),
                                        connectivity=8, _launches=launches)
        assert np.array_equal(R.cpu().numpy(), got["out"])
        needed = got["launches"] if needed is None else needed
        assert got["launches"] == info.launches == needed >= 2 and got["enqueued"] == -(-needed // launches) * launches


def test_determinism(dev):
    """One 129 x 97 busy case three times, once on a side stream: bit-identical, growth and flood."""
    import functions
    name, s, m = grow_cases(129, 97)[0]
    im = np.stack([flood_ref.landscape("random6", 129, 97, b) for b in range(len(s))])
    want, wantf = grow_want(129, 97, 0, None), ref.flood_batch(s, im, m, connectivity=8)
    st, mt, it = torch.from_numpy(s).to(dev), torch.from_numpy(m).to(dev), torch.from_numpy(im).to(dev)

    def run():
        labels, info, dist = functions.split_cells(st, mt, return_distance=True, connectivity=8)
        fl, finfo = functions.watershed(st, it, mask=mt, connectivity=8)
        return labels.cpu().numpy(), dist.cpu().numpy(), info.launches, fl.cpu().numpy(), finfo.launches
    runs = []
    for k in range(3):
        if k == 1:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                runs.append(run())
            torch.cuda.current_stream(dev).wait_stream(side)
        else:
            runs.append(run())
    for labels, dist, launches, fl, fl_launches in runs:
        assert np.array_equal(labels, want["out"]) and np.array_equal(dist, want["dist"]) and np.array_equal(fl, wantf["out"])
        assert launches == runs[0][2] and fl_launches == runs[0][4]


def test_errors(dev):
    """A bad connectivity is refused before anything is allocated, by every function; the raw entries return -2."""
    import _hip
    import functions
    import tester
    s = torch.zeros(2, 9, 7, dtype=torch.int32, device=dev)
    p = torch.zeros(2, 9, 7, device=dev)
    before = torch.cuda.memory_allocated(dev)
    for bad in (6, 0, "8"):
        for call in (lambda: functions.split_cells(s, s, connectivity=bad), lambda: functions.watershed(s, s, connectivity=bad),
                     lambda: functions.reconstruct(s, s, connectivity=bad), lambda: functions.shape_seeds(s, connectivity=bad),
                     lambda: tester.split_instances(s, p, 0.5, connectivity=bad), lambda: tester.split_by_shape(s, connectivity=bad),
                     lambda: tester.split_by_watershed(s, p, 0.5, connectivity=bad),
                     lambda: tester.segment(None, p, return_instances=True, connectivity=bad)):
            with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
                call()
    with pytest.raises(ValueError, match="return_instances"):
        tester.segment(None, p, connectivity=8)
    assert torch.cuda.memory_allocated(dev) == before        # nothing was allocated for any of them
    L = _hip.lib()
    q = _hip.ptr(torch.zeros(4096, dtype=torch.int32, device=dev))
    assert L.unet_geodesic_sweeps_conn(1, 8, 8, -1, 5, 1, q, 0, q, None) == -2 and b"connectivity" in L.unet_last_error()
    assert L.unet_flood_sweeps_conn(1, 8, 8, -1, 5, 1, q, 0, q, None) == -2 and b"connectivity" in L.unet_last_error()
    assert L.unet_flood_assign_conn(1, 8, 8, 5, 1, q, 0, q, None) == -2 and b"connectivity" in L.unet_last_error()
    assert L.unet_reconstruct_sweeps_conn(1, 8, 8, 5, 1, q, 0, q, None) == -2 and b"connectivity" in L.unet_last_error()


# ---- tester -----------------------------------------------------------------------------------------------------------------

def two_cells(dev):
    mask, prob, _ = flood_ref.two_cells()
    mask = mask.copy()
    mask[2, 70], mask[3, 71] = 1, 1                          # a cell without a core: two pixels that touch at a corner
    mask[20, 40], mask[21, 41] = 0, 0                        # and a dent of the same kind in the neck
    return mask, prob, torch.from_numpy(mask).to(dev), torch.from_numpy(prob).to(dev)


def test_tester_splits_equal_their_compositions(dev):
    import functions
    import tester
    mask, prob, mt, pt = two_cells(dev)
    high = 0.9
    cores, _ = functions.label_cells(pt >= high, connectivity=8)
    by_hand = functions.split_cells(cores, mt, orphans="keep", connectivity=8)[0]
    got = tester.split_instances(mt, pt, high, connectivity=8)
    assert torch.equal(got, by_hand)
    seeds = ndimage_label8(prob >= np.float32(high))
    assert np.array_equal(got.cpu().numpy(), ref.keep_orphans(ref.grow(seeds, mask, None, 8)["out"], seeds, mask, 8))
    assert int(got.max()) == 3 and not torch.equal(got, tester.split_instances(mt, pt, high))      # at 4 the orphan is two cells
    sh = functions.shape_seeds(mt, 2.0, connectivity=8)[0]
    assert torch.equal(tester.split_by_shape(mt, connectivity=8), functions.split_cells(sh, mt, orphans="keep", connectivity=8)[0])
    assert np.array_equal(sh.cpu().numpy(), ref.seeds(mask, 2.0, connectivity=8)[0])
    flooded = functions.watershed(cores, 1 - pt, mask=mt, levels=64, connectivity=8)[0]
    rest = functions.label_cells((mt != 0) & (flooded == 0), connectivity=8)[0]
    by_hand = torch.where(rest > 0, rest + cores.amax(), flooded)
    got = tester.split_by_watershed(mt, pt, high, connectivity=8)
    assert torch.equal(got, by_hand) and int(got.max()) == 3
    want = ref.flood(seeds, 1 - prob, mask, levels=64, connectivity=8)["out"]
    assert np.array_equal(got.cpu().numpy(), ref.keep_orphans(want, seeds, mask, 8))


def ndimage_label8(a):
    from scipy import ndimage
    return ndimage.label(a, ref.structure(8))[0].astype(np.int32)


def test_segment_with_connectivity(dev, net):
    """One 100 x 130 image at tile_size=188: the instance map is label_cells(mask, connectivity=8), with split= it is
    split_instances(..., connectivity=8); mask and probabilities are those of the call without it."""
    import functions
    import tester
    x = torch.from_numpy(image(30, 1, 100, 130, blobs=9)[0]).to(dev)
    kw = dict(tile_size=188, max_batch=64, return_probs=True, return_instances=True)
    m0, p0, i0 = tester.segment(net, x, **kw)
    m8, p8, i8 = tester.segment(net, x, connectivity=8, **kw)
    assert torch.equal(m8, m0) and torch.equal(p8, p0) and i8.dtype == torch.int32 and i8.shape == m0.shape
    assert torch.equal(i8, functions.label_cells(m0, connectivity=8)[0])
    assert np.array_equal(i8.cpu().numpy(), ndimage_label8(m0.cpu().numpy() != 0))
    m4, p4, i4 = tester.segment(net, x, connectivity=4, **kw)
    assert torch.equal(i4, i0) and torch.equal(m4, m0)
    inside = p0[m0 != 0]
    assert inside.numel() > 0
    high = float(inside.median())
    m1, p1, i1 = tester.segment(net, x, split=high, connectivity=8, **kw)
    assert torch.equal(m1, m0) and torch.equal(p1, p0)
    assert torch.equal(i1, tester.split_instances(m0, p0, high, connectivity=8))
    assert ((i1 != 0) == (m0 != 0)).all()
    m2, i2 = tester.segment(net, x, tile_size=188, max_batch=64, return_instances=True, split=high, connectivity=8)
    assert torch.equal(m2, m0) and torch.equal(i2, i1)
    m3, i3 = tester.segment(net, x, tile_size=188, max_batch=64, return_instances=True, shape_split=1.0, connectivity=8)
    assert torch.equal(i3, tester.split_by_shape(m0, 1.0, connectivity=8))
    m5, i5 = tester.segment(net, x, tile_size=188, max_batch=64, return_instances=True, split=high, watershed=True, connectivity=8)
    assert torch.equal(i5, tester.split_by_watershed(m0, p0, high, connectivity=8))


def test_segment_steps_compose(dev, net):
    """The same image and tiles: connectivity, measure, clean, split, watershed and views in the combinations no other test makes,
    each equal, bit for bit, to the composition of the plain call's mask and probabilities with the step's own function.  The
    one exception: the mean and std of measure=True, whose fp64 sums are not the same in two runs, are held to their rounding."""
    import functions
    import tester
    x = torch.from_numpy(image(30, 1, 100, 130, blobs=9)[0]).to(dev)
    kw = dict(tile_size=188, max_batch=64, return_probs=True, return_instances=True)
    m0, p0, i0 = tester.segment(net, x, **kw)
    assert bool((m0 != 0).any()) and bool((m0 == 0).any())   # foreground and background: nothing below is vacuous
    high = float(p0[m0 != 0].median())

    out = tester.segment(net, x, connectivity=8, measure=True, **kw)
    assert len(out) == 4
    m, p, inst, props = out
    assert torch.equal(m, m0) and torch.equal(p, p0) and torch.equal(inst, functions.label_cells(m0, connectivity=8)[0])
    want = functions.cell_props(inst, x)
    assert isinstance(props, functions.CellProps)
    for name in props._fields:
        if name not in ("mean", "std"):
            assert np.array_equal(getattr(props, name), getattr(want, name), equal_nan=True), name
    # mean and std of a float image are formed from fp64 sums whose adds round in an order that differs between two runs
    # (functions.cell_sums), so two calls on the same input need not agree in the last bits.  n values of magnitude <= v: each
    # run's sum is within n 2^-53 of sum |v| <= n v, so the means of two runs differ by at most n 2^-52 v (+ the division's
    # 2^-52 v) <= 2^-51 n v; likewise sum v^2 / n by (n + 1) 2^-52 v^2, mean^2 by 2 v 2^-51 n v + 2^-52 v^2, the subtraction adds
    # 2^-52 v^2: the variances differ by at most 2^-49 n v^2, and the square root and squaring it again stay within 2^-48 n v^2
    on = ~np.isnan(want.area)
    n, v = want.area[on], np.maximum(np.abs(want.min[on]), np.abs(want.max[on]))
    for name in ("mean", "std"):
        assert np.array_equal(np.isnan(getattr(props, name)), ~on) and np.array_equal(np.isnan(getattr(want, name)), ~on), name
    assert (np.abs(props.mean[on] - want.mean[on]) <= 2.0 ** -51 * n * v).all()
    assert (np.abs(props.std[on] ** 2 - want.std[on] ** 2) <= 2.0 ** -48 * n * v * v).all()

    clean = {"fill_holes": False, "min_area": 4}
    m, p, inst = tester.segment(net, x, connectivity=8, clean=clean, split=high, **kw)
    mc = functions.clean_mask(m0, fill_holes=False, min_area=4)
    assert torch.equal(m, mc) and torch.equal(p, p0)
    assert torch.equal(inst, tester.split_instances(mc, p0, high, connectivity=8))

    ny, nx, _, _ = tester.tile_grid(100, 130, 188)
    assert (ny * nx) % 64 != 0                               # so a chunk of 64 holds tiles of two views
    mv, pv, iv = tester.segment(net, x, views="flips", **kw)
    m, p, inst = tester.segment(net, x, views="flips", split=high, watershed=16, connectivity=8, **kw)
    assert torch.equal(m, mv) and torch.equal(p, pv)
    assert torch.equal(inst, tester.split_by_watershed(mv, pv, high, 16, connectivity=8))

    m, p, i4 = tester.segment(net, x, shape_split=1.0, connectivity=4, **kw)
    m, p, inst = tester.segment(net, x, shape_split=1.0, **kw)
    assert torch.equal(i4, inst)
