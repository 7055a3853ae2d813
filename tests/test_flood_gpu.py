"""The seeded watershed on the device (functions.watershed -> unet_flood_init / unet_flood_sweeps / unet_flood_assign /
unet_flood_finish; tester.split_by_watershed; tester.segment(split=, watershed=)) against the numpy restatement
tests/flood_ref.py, statement (a), which tests/test_flood_cpu.py pins to the level loop over the geodesic growth, to hand-worked
answers and to the inputs' power to catch the one-key shortcut.  Everything is an integer and is compared bit for bit: ids, pass
levels, plateau distances and every count.  Every pointer handed to the raw entry points is a poisoned guarded.Arena buffer."""
import functools

import numpy as np
import pytest
import torch

import flood_ref as ref
import guarded
import split_ref
from gpu_support import dev, net, image  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CODE = {torch.int64: 0, torch.float32: 1, torch.int32: 2, torch.uint8: 3}
KEYS = ref.MAPS + ref.INTS
UNSET = 0x5A5A5A5A                                           # int32 poison is -1, which the level and distance maps legitimately hold


@functools.lru_cache(maxsize=None)
def cases(H, W):
    return ref.size_cases(H, W)


@functools.lru_cache(maxsize=None)
def want_for(H, W, k, limit=None):
    name, s, im, m = cases(H, W)[k]
    return ref.flood_batch(s, im, m, max_level=limit)


def raw_flood(dev, seeds, img, mask, levels=None, limit=None, launches=8, mask_dtype=torch.uint8, image_dtype=torch.int32):
    """The four entry points on guarded buffers, with the wrapper's loop per stage: a dict like flood_ref.flood_batch's, plus
    "launches" (per stage, the launches up to and including the first that changed nothing), "enqueued" and "lowered"."""
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = seeds.shape
    s = a.inp(torch.from_numpy(seeds).to(torch.int32), "seeds")
    im = a.inp(torch.from_numpy(img).to(image_dtype), "image")
    m = None if mask is None else a.inp(torch.from_numpy(mask).to(mask_dtype), "mask")
    outside, status = a.out((B,), torch.int32, "seeds_outside"), a.out((2, B), torch.int64, "status")
    unreached, top = a.out((B,), torch.int32, "unreached"), a.out((B,), torch.int32, "max_level")
    slots = a.out((launches + 2, B), torch.int32, "changed")             # slot 0 and the last one are never named
    scratch = a.scratch(L.unet_flood_scratch_bytes(B, H, W), "scratch")
    out, lev, dist = (a.out((B, H, W), torch.int32, n) for n in ("out", "pass_level", "dist"))
    lev.fill_(UNSET)
    dist.fill_(UNSET)
    _hip.run("unet_flood_init", dev, a.ptr(s), a.ptr(im), CODE[image_dtype], levels or 0, a.ptr(m), CODE[mask_dtype], B, H, W, a.ptr(outside),
             a.ptr(status), a.ptr(scratch))
    a.verify(outside, status)
    res = {"launches": [], "enqueued": [], "lowered": []}
    for stage in (1, 2):
        per_launch = []
        for _ in range(H * W + 2):
            if stage == 1:
                _hip.run("unet_flood_sweeps", dev, B, H, W, -1 if limit is None else limit, launches, a.ptr(slots), 1, a.ptr(scratch))
            else:
                _hip.run("unet_flood_assign", dev, B, H, W, launches, a.ptr(slots), 1, a.ptr(scratch))
            c = slots.cpu().numpy()
            assert (c[0] == -1).all() and (c[-1] == -1).all() and (c[1:-1] >= 0).all()
            per_launch.extend(c[1:-1].astype(np.int64))
            if not c[1:-1].any(axis=1).all():
                break
        else:
            raise AssertionError("stage %d did not end" % stage)
        per_launch = np.stack(per_launch)
        first_idle = int(np.argmin(per_launch.any(axis=1)))
        assert not per_launch[first_idle:].any()             # a launch that changed nothing: so did every one after it
        res["launches"].append(first_idle + 1)
        res["enqueued"].append(len(per_launch))
        res["lowered"].append(per_launch.sum(axis=0))
    _hip.run("unet_flood_finish", dev, B, H, W, a.ptr(out), a.ptr(lev), a.ptr(dist), a.ptr(unreached), a.ptr(top), a.ptr(scratch))
    a.verify(out, unreached, top)
    maps = {"out": out.cpu().numpy(), "pass_level": lev.cpu().numpy(), "dist": dist.cpu().numpy()}
    assert (maps["pass_level"] != UNSET).all() and (maps["dist"] != UNSET).all()
    st = status.cpu().numpy()
    res.update(maps, unreached=unreached.cpu().numpy().astype(np.int64), seeds_outside=outside.cpu().numpy().astype(np.int64),
               max_level=top.cpu().numpy().astype(np.int64), status=st[0], bad_values=st[1], launches=tuple(res["launches"]))
    return res


def wrapped(dev, seeds, img, mask, levels=None, limit=None, mask_dtype=torch.uint8, image_dtype=torch.int32, seed_dtype=torch.int64, **kw):
    """functions.watershed -> a dict like raw_flood's (no status words)."""
    import functions
    s, im = torch.from_numpy(seeds).to(dev).to(seed_dtype), torch.from_numpy(img).to(dev).to(image_dtype)
    m = None if mask is None else torch.from_numpy(mask).to(dev).to(mask_dtype)
    labels, info, lev, dist = functions.watershed(s, im, mask=m, levels=levels, max_level=limit, return_levels=True, **kw)
    for t in (labels, lev, dist):
        assert t.dtype == torch.int32 and t.shape == seeds.shape and t.is_cuda
    for v in info[:3]:
        assert v.dtype == np.int64 and v.shape == (seeds.shape[0] if seeds.ndim == 3 else 1,)
    assert isinstance(info.launches, tuple) and len(info.launches) == 2
    two = functions.watershed(s, im, mask=m, levels=levels, max_level=limit, **kw)
    assert len(two) == 2 and torch.equal(two[0], labels) and two[1].launches == info.launches
    return {"out": labels.cpu().numpy(), "pass_level": lev.cpu().numpy(), "dist": dist.cpu().numpy(), "unreached": info.unreached,
            "seeds_outside": info.seeds_outside, "max_level": info.max_level, "launches": info.launches}


def same(got, want, what):
    for k in KEYS:
        if k in got:
            assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("H,W", ref.SIZES)
def test_flooding_equals_the_restatement(dev, H, W):
    """Bit for bit: every kind of image at this size (B 1-4; the batch of four holds an image without seeds, one with an empty mask
    and one with a full mask next to a busy one; the five landscapes rotate through the images), through the raw entry points and,
    with int64 seeds, through functions.watershed."""
    lowered = 0
    for k, (name, s, im, m) in enumerate(cases(H, W)):
        want = want_for(H, W, k)
        got = raw_flood(dev, s, im, m)
        same(got, want, name)
        assert np.array_equal(got["lowered"][0] > 0, (want["dist"] > 0).any(axis=(1, 2))), name
        lowered += int(got["lowered"][0].sum())
        w = wrapped(dev, s, im, m)
        same(w, want, (name, "wrapper"))
        assert w["launches"] == got["launches"]
    assert lowered > 0 or H * W < 4
    name, s, im, m = cases(H, W)[0]
    got = wrapped(dev, s[0], im[0], m[0])                     # [H,W]
    assert got["out"].shape == (H, W)
    same(got, {k: (v[0] if k in ref.MAPS else v[:1]) for k, v in want_for(H, W, 0).items()}, "[H,W]")


def test_the_built_cases(dev):
    """The hand-worked cases of tests/test_flood_cpu.py on the device: plateaus with an even and an odd gap, the ridge, the pit
    behind a pass, and the late low path, where the one-key shortcut gives another answer."""
    for name, (s, im, *m) in (("plateau 6", ref.plateau(6)), ("plateau 5", ref.plateau(5)), ("ridge", ref.ridge()), ("pit", ref.pit()),
                              ("late low path", ref.late_low_path())):
        m = m[0][None] if m else None
        want = ref.flood_batch(s[None], im[None], m)
        same(raw_flood(dev, s[None], im[None], m), want, name)
        same(wrapped(dev, s[None], im[None], m), want, (name, "wrapper"))
    s, im, m = ref.late_low_path()
    got = wrapped(dev, s, im, m)
    assert got["out"][0].tolist() == [1, 1, 2, 2, 0] and ref.naive(s, im, m)[0].tolist() == [1, 1, 2, 1, 0]
    s, im = ref.ridge()
    assert wrapped(dev, s, im, None)["out"].tolist() == [[7, 7, 7, 7, 7, 4, 4, 4]]


@pytest.mark.parametrize("dtype", (torch.uint8, torch.int64, torch.float32, torch.int32, torch.bool, None))
def test_mask_dtypes(dev, dtype):
    name, s, im, m = cases(65, 63)[2]
    if dtype is None:                                        # no mask: the whole image
        want = ref.flood_batch(s, im, None)
        same(raw_flood(dev, s, im, None), want, "no mask")
        same(wrapped(dev, s, im, None, seed_dtype=torch.int32), want, "no mask, wrapper")
        full = np.ones_like(m)
        same(wrapped(dev, s, im, full), want, "a full mask")
        return
    want = want_for(65, 63, 2)
    if dtype != torch.bool:
        same(raw_flood(dev, s, im, m, mask_dtype=dtype), want, dtype)
    same(wrapped(dev, s, im, m, mask_dtype=dtype, seed_dtype=torch.int32), want, (dtype, "wrapper"))


@pytest.mark.parametrize("dtype", (torch.uint8, torch.int32, torch.int64, torch.float32))
def test_image_dtypes(dev, dtype):
    """Integer images are read as they are; a float32 image is quantised by the rule, the product in fp32: random values from
    below 0 to above 1 with 6, 64 and 65536 levels, and the level centres (v + 0.5) / levels, which give v back."""
    name, s, im, m = cases(65, 63)[2]
    if dtype != torch.float32:
        im = im % 251 if dtype == torch.uint8 else im
        want = ref.flood_batch(s, im, m)
        assert want["max_level"].max() > (200 if dtype == torch.uint8 else 60000)
        same(raw_flood(dev, s, im, m, image_dtype=dtype), want, dtype)
        same(wrapped(dev, s, im, m, image_dtype=dtype), want, (dtype, "wrapper"))
        return
    rs = np.random.RandomState(11)
    f = (rs.rand(*im.shape) * 1.2 - 0.1).astype(np.float32)
    f[:, 0, :8] = (0.0, np.nextafter(np.float32(1 / 64), np.float32(0)), 1 / 64, 1.0, np.nextafter(np.float32(1), np.float32(2)), -0.25, -1e30, 3e38)
    for levels in (6, 64, 65536):
        want = ref.flood_batch(s, f, m, levels=levels)
        assert want["max_level"].max() == levels - 1
        same(raw_flood(dev, s, f, m, levels=levels, image_dtype=dtype), want, levels)
        same(wrapped(dev, s, f, m, levels=levels, image_dtype=dtype), want, (levels, "wrapper"))
    v = im % 64
    centres = ((v + 0.5) / 64).astype(np.float32)
    assert np.array_equal(ref.quantise(centres, 64)[0], v)
    same(wrapped(dev, s, centres, m, levels=64, image_dtype=dtype), ref.flood_batch(s, v, m), "level centres")


def test_a_constant_image_gives_split_cells(dev):
    """On a constant image the flood is the geodesic growth: functions.split_cells on the device, ids and distances, bit for bit."""
    import functions
    for H, W, k in ((129, 97, 3), (63, 65, 1)):
        name, s, _, m = cases(H, W)[k]
        st, mt = torch.from_numpy(s).to(dev), torch.from_numpy(m).to(dev)
        labels, info, dist = functions.split_cells(st, mt, return_distance=True)
        for value in (0, 9):
            got, finfo, lev, d = functions.watershed(st, torch.full_like(st, value), mask=mt, return_levels=True)
            assert torch.equal(got, labels) and torch.equal(d, dist), (name, value)
            assert np.array_equal(finfo.unreached, info.unreached) and np.array_equal(finfo.seeds_outside, info.seeds_outside)
            assert finfo.launches[0] <= info.launches            # the geodesic key holds the id too, which may fall later
            assert ((lev == value) | (lev == 0) | (lev == -1)).all() and ((lev == -1) == (got == 0)).all()
        assert int((labels > 0).sum()) > int((st > 0).sum())


@pytest.mark.parametrize("H,W", ((33, 31), (63, 65)))
def test_the_level_loop_on_the_device(dev, H, W):
    """The second statement, with the project's own geodesic growth in the place of its numpy restatement: for h = 0 .. 5,
    labels = split_cells(labels, region & (v <= h | labels > 0))."""
    import functions
    rs = np.random.RandomState(H)
    for k, (name, s, _, m) in enumerate(cases(H, W)):
        st, mt = torch.from_numpy(s).to(dev), torch.from_numpy(m).to(dev) != 0
        v = torch.from_numpy(rs.randint(0, 6, s.shape).astype(np.int32)).to(dev)
        labels = torch.where(mt, st, torch.zeros_like(st))
        for h in range(6):
            labels = functions.split_cells(labels, mt & ((v <= h) | (labels > 0)))[0]
        got, info = functions.watershed(st, v, mask=mt)
        assert torch.equal(got, labels), name
        assert int((got > 0).sum()) > int((st > 0).sum()) or not s.any() or not m.any()


def test_batching_the_launches_changes_nothing(dev):
    """Any number of launches per call gives the same planes after the same number of launches, in both stages: the test of the
    ping-pong between the two key planes and between the two id planes (an odd number of launches ends in the second one) and of
    the change counters."""
    for H, W, k in ((129, 97, 3), (63, 65, 0), (257, 255, 0)):
        name, s, im, m = cases(H, W)[k]
        want = want_for(H, W, k)
        needed = None
        for launches in (1, 3, 8):
            got = raw_flood(dev, s, im, m, launches=launches)
            same(got, want, (name, launches))
            w = wrapped(dev, s, im, m, _launches=launches)
            same(w, want, (name, launches, "wrapper"))
            needed = got["launches"] if needed is None else needed
            assert got["launches"] == w["launches"] == needed, (name, launches)
            assert got["enqueued"] == [-(-n // launches) * launches for n in needed], (name, launches)
        assert min(needed) >= 2                               # one launch that lowered something, one that found nothing to do


def test_max_level(dev):
    """0: the sources and what they reach on level 0; a middle level; the top level, which is no limit."""
    for H, W, k in ((63, 65, 0), (129, 97, 3)):
        name, s, _, m = cases(H, W)[k]
        im = np.stack([ref.landscape("random6", H, W, b) for b in range(len(s))])
        full = ref.flood_batch(s, im, m)
        reached = []
        for limit in (0, 3, 5):
            want = ref.flood_batch(s, im, m, max_level=limit)
            assert (want["max_level"] <= limit).all()
            same(raw_flood(dev, s, im, m, limit=limit), want, (name, limit))
            same(wrapped(dev, s, im, m, limit=limit), want, (name, limit, "wrapper"))
            reached.append(int((want["out"] > 0).sum()))
        same(want, full, "the top level")
        assert reached[0] < reached[1] < reached[2]


def test_the_serpentine(dev):
    """41 x 400: a valley of level 0 with a seed at each end, between walls of level 5 that are region pixels.  Inside a tile the
    keys first spread across the walls and must fall again when the valley path arrives, one tile per launch."""
    s, im, m = ref.serpentine()
    want = ref.flood_batch(s, im, m)
    assert want["max_level"][0] == 5 and want["unreached"][0] == 0 and want["dist"].max() > 4000
    got = raw_flood(dev, s, im, m)
    same(got, want, "serpentine")
    assert got["launches"][0] > 8 and got["enqueued"][0] == -(-got["launches"][0] // 8) * 8
    w = wrapped(dev, s, im, None)                            # the mask is full
    same(w, want, "serpentine, wrapper")
    assert w["launches"] == got["launches"]
    print("serpentine: launches (stage 1, stage 2) =", got["launches"])


def test_errors(dev):
    """Errors that need no device work are raised before any; a bad image value, a value that is not finite and an id of 2^24 are
    counted by the kernel."""
    import _hip
    import functions
    s = torch.zeros(2, 9, 7, dtype=torch.int32, device=dev)
    host, real = s.cpu(), s.float()
    before = torch.cuda.memory_allocated(dev)
    with pytest.raises(NotImplementedError):
        functions.watershed(host, s)
    with pytest.raises(NotImplementedError):
        functions.watershed(s, host)
    with pytest.raises(NotImplementedError):
        functions.watershed(s, s, mask=host)
    with pytest.raises(ValueError, match="equal shape"):
        functions.watershed(s, s[:1])
    with pytest.raises(ValueError, match="equal shape"):
        functions.watershed(s[0, 0], s[0, 0])
    with pytest.raises(ValueError, match="max_level"):
        functions.watershed(s, s, max_level=-1)
    with pytest.raises(ValueError, match="levels"):
        functions.watershed(s, real)
    with pytest.raises(ValueError, match="levels"):
        functions.watershed(s, real, levels=1 << 17)
    with pytest.raises(ValueError, match="levels"):
        functions.watershed(s, s, levels=8)
    with pytest.raises(ValueError, match="int32 or int64"):
        functions.watershed(real, s)
    assert torch.cuda.memory_allocated(dev) == before        # nothing was allocated for any of them
    bad = s.clone()
    bad[1, 2, 3] = -1
    with pytest.raises(ValueError, match="negative"):
        functions.watershed(bad, s)
    bad[1, 2, 3] = 1 << 24
    with pytest.raises(ValueError, match="2\\^24"):
        functions.watershed(bad, s)
    for value in (-1, 1 << 16):
        img = s.clone()
        img[0, 4, 4] = value
        with pytest.raises(ValueError, match="1 pixels hold an image value outside"):
            functions.watershed(s, img)
        with pytest.raises(ValueError, match="outside"):
            functions.watershed(s, img.long(), mask=torch.ones_like(s))
    for value in (float("nan"), float("inf"), float("-inf")):
        img = real.clone()
        img[1, 0, 6] = value
        with pytest.raises(ValueError, match="1 pixels hold an image value that is not finite"):
            functions.watershed(s, img, levels=16)
    assert functions.watershed(s, real + 3e38, levels=16)[1].max_level.tolist() == [0, 0]     # finite, no seeds: nothing to flood
    seeds = np.zeros((1, 3, 5), np.int32)
    seeds[0, 1] = (1 << 24, -3, 0, 0, 6)
    img = np.zeros((1, 3, 5), np.int32)
    img[0, 0, :3] = (70000, -1, 65535)
    got = raw_flood(dev, seeds, img, None)
    want = ref.flood_batch(seeds, img, None)
    same(got, want, "an id of 2^24 and bad image values")
    assert got["status"].tolist() == [2] and got["bad_values"].tolist() == [2] and set(np.unique(got["out"])) == {6}
    assert got["max_level"].tolist() == [65535]
    L = _hip.lib()
    q = _hip.ptr(torch.zeros(4096, dtype=torch.int32, device=dev))
    assert L.unet_flood_sweeps(1, 8, 8, -1, 0, q, 0, q, None) == -2
    assert L.unet_flood_assign(1, 8, 8, 0, q, 0, q, None) == -2
    assert L.unet_flood_init(q, q, 7, 0, q, 0, 1, 8, 8, q, q, q, None) == -2 and b"dtype" in L.unet_last_error()
    assert L.unet_flood_finish(1, 8, 8, q, None, q, q, q, None, None) == -2


# ---- tester.split_by_watershed and tester.segment(split=, watershed=) -----------------------------------------------------------

def by_hand(mask, fg_prob, high, levels):
    """tester.split_by_watershed in numpy: the restatement on the 4-connected components of fg_prob >= high and the landscape
    1 - fg_prob in float32, then split_cells' orphans='keep'."""
    from scipy import ndimage
    seeds = ndimage.label(fg_prob >= high, split_ref.CROSS)[0]
    out = ref.flood(seeds, np.float32(1) - fg_prob.astype(np.float32), mask, levels=levels)["out"]
    return split_ref.keep_orphans(out, seeds, mask)


def test_two_touching_cells_are_cut_where_the_probability_dips(dev):
    """A large and a small disc that overlap, the probability dip (the membrane) on the column x = 41: the watershed cuts there,
    the geodesic growth of plain split cuts halfway between the cores, about x = 35, through the large cell."""
    import tester
    mask, p, membrane = ref.two_cells()
    mt, pt = torch.from_numpy(mask).to(dev), torch.from_numpy(p).to(dev)
    xx = np.broadcast_to(np.arange(mask.shape[1]), mask.shape)
    # a membrane pixel is one step from both sides, a tie, the smaller id; at the column's two ends the left neighbour is background
    on_membrane = np.where(mask[:, membrane - 1:membrane] != 0, 1, 2)
    want = np.where(mask != 0, np.where(xx < membrane, 1, np.where(xx > membrane, 2, on_membrane)), 0)
    assert (on_membrane[mask[:, membrane] != 0] == 2).sum() == 2
    for levels in (64, 16, 1000):
        got = tester.split_by_watershed(mt, pt, 0.9, levels) if levels != 64 else tester.split_by_watershed(mt, pt, 0.9)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), levels
        assert np.array_equal(want, by_hand(mask, p, np.float32(0.9), levels))
    blind = tester.split_instances(mt, pt, 0.9).cpu().numpy()
    row = blind[20]
    cut = int(np.argmax(row == 2))
    print("row 20: the geodesic cut is at x = %d, the watershed's at x = %d" % (cut, membrane + 1))
    assert set(np.unique(blind)) == {0, 1, 2} and 30 <= cut <= 38 and ((blind == 2) & (want == 1)).sum() > 50
    both = np.stack([mask, mask[::-1].copy()])                # a batch, and a component without a core in it stays a cell
    pb = np.stack([p, np.where(p[::-1] > 0.9, 0.8, p[::-1]).astype(np.float32)])
    got = tester.split_by_watershed(torch.from_numpy(both).to(dev), torch.from_numpy(pb).to(dev), 0.9).cpu().numpy()
    assert np.array_equal(got[0], want) and np.array_equal(got[1], (both[1] != 0).astype(np.int32))
    assert np.array_equal(got[1], by_hand(both[1], pb[1], np.float32(0.9), 64))


def test_segment_split_watershed(dev, net):
    """segment(split=high, watershed=levels) is split_by_watershed of the call's own mask and probabilities, changes neither,
    and composes with clean and measure as split does."""
    import tester
    x = torch.from_numpy(image(30, 1, 100, 130, blobs=9)[0]).to(dev)
    kw = dict(tile_size=188, max_batch=64, return_instances=True)
    m0, p0, i0 = tester.segment(net, x, return_probs=True, **kw)
    inside = p0[m0 != 0]
    assert inside.numel() > 0 and len(torch.unique(inside)) > 1
    high = float(inside.median())
    m1, p1, i1 = tester.segment(net, x, return_probs=True, split=high, watershed=16, **kw)
    assert torch.equal(m1, m0) and torch.equal(p1, p0) and i1.dtype == torch.int32 and i1.shape == m0.shape
    assert torch.equal(i1, tester.split_by_watershed(m0, p0, high, 16))
    assert np.array_equal(i1.cpu().numpy(), by_hand(m0.cpu().numpy(), p0.cpu().numpy(), np.float32(high), 16))
    assert ((i1 != 0) == (m0 != 0)).all()
    m2, i2 = tester.segment(net, x, split=high, watershed=True, **kw)          # 64 levels, the probabilities formed internally
    assert torch.equal(m2, m0) and torch.equal(i2, tester.split_by_watershed(m0, p0, high))
    plain = tester.segment(net, x, split=high, watershed=None, **kw)
    assert torch.equal(plain[1], tester.split_instances(m0, p0, high))          # None: today's behaviour
    m3, i3, props = tester.segment(net, x, split=high, watershed=16, clean=dict(fill_holes=False, min_area=4), measure=True, **kw)
    mc = tester.segment(net, x, clean=dict(fill_holes=False, min_area=4), tile_size=188, max_batch=64)
    assert torch.equal(m3, mc) and torch.equal(i3, tester.split_by_watershed(mc, p0, high, 16))
    counts = torch.bincount(i3.flatten().long()).cpu().numpy()
    assert np.array_equal(np.nan_to_num(props.area, nan=0.0), counts.astype(np.float64))     # measured on the flooded instance map
    for kwargs, word in ((dict(watershed=16), "split"), (dict(watershed=16, split=high, shape_split=2.0), "shape_split"),
                         (dict(watershed=0, split=high), "watershed")):
        with pytest.raises(ValueError, match=word):
            tester.segment(net, x, **kw, **kwargs)
