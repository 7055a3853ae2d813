"""The per-cell table on the device (functions.cell_sums / cell_props / select_cells -> unet_cell_sums, unet_remap_labels;
tester.segment(measure=True)) against the numpy restatement tests/measure_ref.py (pinned to hand-worked answers and to
scipy.ndimage by tests/test_measure_cpu.py).  Every integer field is compared bit for bit and every case runs twice; the fp64 sums
of a float image are held to area 2^-52 sum |v| (the reference's own rounding, area 2^-53 sum |v|, plus the device's).  Every
pointer handed to the raw entry points is a poisoned guarded.Arena buffer."""
import functools

import numpy as np
import pytest
import torch

import guarded
import instances_ref
import measure_ref as ref
from gpu_support import dev, net, hip, image, rejected  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CODE = {torch.int64: 0, torch.float32: 1, torch.int32: 2, torch.uint8: 3}
EXACT = ("area", "bbox", "moments", "frame", "open", "contact", "present")


def raw_sums(dev, labels, images=None, n_max=None, ldtype=torch.int32, expect_status=(0, 0)):
    """unet_cell_sums on guarded buffers: a dict like measure_ref.sums_batch's; labels, images numpy [B,H,W]."""
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = labels.shape
    n_max = int(labels.max()) if n_max is None else n_max
    N = n_max + 1
    lab = a.inp(torch.from_numpy(labels).to(ldtype), "labels")
    img = None if images is None else a.inp(torch.from_numpy(images), "image")
    isfloat = img is not None and img.dtype == torch.float32
    area, bbox = a.out((B, N), torch.int64, "area"), a.out((B, N, 4), torch.int32, "bbox")
    moments, edges = a.out((B, N, 5), torch.int64, "moments"), a.out((B, N, 3), torch.int64, "edges")
    vsum = None if img is None else a.out((B, N, 2), torch.float64 if isfloat else torch.int64, "vsum")
    vrange = None if img is None else a.out((B, N, 2), torch.float32 if isfloat else torch.int32, "vrange")
    present, status = a.out((B, N), torch.uint8, "present"), a.out((B, 2), torch.int64, "status")
    scratch = a.scratch(L.unet_cell_sums_scratch_bytes(B, n_max), "scratch")
    _hip.run("unet_cell_sums", dev, a.ptr(lab), CODE[ldtype], a.ptr(img), 0 if img is None else CODE[img.dtype], B, H, W, n_max, a.ptr(area),
             a.ptr(bbox), a.ptr(moments), a.ptr(edges), a.ptr(vsum), a.ptr(vrange), a.ptr(present), a.ptr(status), a.ptr(scratch))
    a.verify(area, bbox, moments, edges, vsum, vrange, present, status)       # the scratch holds complements: 0xFF bytes are data there
    assert torch.equal(lab.cpu(), torch.from_numpy(labels).to(ldtype))
    assert status.cpu().sum(dim=0).tolist() == list(expect_status)
    e = edges.cpu().numpy()
    out = {"area": area.cpu().numpy(), "bbox": bbox.cpu().numpy(), "moments": moments.cpu().numpy(), "frame": e[..., 0], "open": e[..., 1],
           "contact": e[..., 2], "present": present.cpu().numpy().astype(bool), "v_sum": None, "v_sum2": None, "v_min": None, "v_max": None}
    assert set(np.unique(present.cpu().numpy()).tolist()) <= {0, 1}
    if img is not None:
        s, r = vsum.cpu().numpy(), vrange.cpu().numpy()
        out.update(v_sum=s[..., 0], v_sum2=s[..., 1], v_min=r[..., 0], v_max=r[..., 1])
    return out


def wrapped(dev, labels, images=None, n_max=None, ldtype=torch.int32):
    """functions.cell_sums as the same dict."""
    import functions
    lab = torch.from_numpy(labels).to(dev).to(ldtype)
    img = None if images is None else torch.from_numpy(images).to(dev)
    s = functions.cell_sums(lab, img, n_max=n_max)
    assert isinstance(s, functions.CellSums) and all(t is None or (t.is_cuda and t.shape[:2] == s.area.shape) for t in s)
    assert s.present.dtype == torch.bool
    return {k: None if t is None else t.cpu().numpy() for k, t in s._asdict().items()}


def same(got, want, labels, images, what):
    for k in EXACT:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    if images is None:
        assert all(got[k] is None for k in ("v_sum", "v_sum2", "v_min", "v_max")), what
        return
    for k in ("v_min", "v_max"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    if images.dtype.kind != "f":
        for k in ("v_sum", "v_sum2"):
            assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (what, k)
        return
    n_max = want["area"].shape[1] - 1
    for b in range(len(labels)):
        sabs, ssq = ref.abs_sums(labels[b], images[b], n_max)
        bound = want["area"][b] * 2.0 ** -52
        assert got["v_sum"].dtype == np.float64 and got["v_sum2"].dtype == np.float64
        assert (np.abs(got["v_sum"][b] - want["v_sum"][b]) <= bound * sabs).all(), (what, "v_sum", b)
        assert (np.abs(got["v_sum2"][b] - want["v_sum2"][b]) <= bound * ssq).all(), (what, "v_sum2", b)


def equal_runs(a, b, what):
    for k in EXACT + ("v_min", "v_max"):
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), (what, k, "two runs differ")
    if a["v_sum"] is not None and a["v_sum"].dtype.kind == "i":
        assert np.array_equal(a["v_sum"], b["v_sum"]) and np.array_equal(a["v_sum2"], b["v_sum2"]), (what, "two runs differ")


def check(dev, labels, images=None, n_max=None, ldtypes=(torch.int32, torch.int64), what=""):
    """Raw entry twice and the wrapper, for each label dtype, against measure_ref."""
    want = ref.sums_batch(labels, images, n_max)
    for ldtype in ldtypes:
        one = raw_sums(dev, labels, images, n_max, ldtype)
        two = raw_sums(dev, labels, images, n_max, ldtype)
        same(one, want, labels, images, (what, ldtype, "raw"))
        equal_runs(one, two, (what, ldtype))
        same(wrapped(dev, labels, images, n_max, ldtype), want, labels, images, (what, ldtype, "wrapper"))
    return want


def wrapped_rows(H, W):
    """The same id at the end of every row and at the start of the next."""
    m = np.zeros((H, W), np.int32)
    m[:, W - 1] = 3
    m[1:, 0] = 3
    return m


@functools.lru_cache(maxsize=None)
def maps(H, W):
    """The named id maps [B,H,W] of one size, B 1-3."""
    gt, pred = instances_ref.cells_case(H * 7 + W, 9, H, W, stride=3)
    out = [("cells", np.stack([gt, pred, gt[::-1, ::-1]]).astype(np.int32))]
    for kind, seed in (("discs", 1), ("speckle0.5", 2)):
        m = instances_ref.mask_batch(kind, seed + H + W, H, W)[:3]
        out.append((kind, np.stack([instances_ref.label(x)[0] for x in m])))
    out.append(("zeros", np.zeros((1, H, W), np.int32)))
    out.append(("one id", np.full((2, H, W), 7, np.int32)))
    g = ref.gaps_and_parts(H, W, 1000)
    out.append(("gaps", np.stack([g, g[::-1].copy(), g.T.reshape(H, W)]).astype(np.int32)))
    if W >= 2:
        out.append(("wrapped rows", wrapped_rows(H, W)[None]))
        two = np.ones((1, H, W), np.int32)
        two[:, :, W // 2:] = 2
        out.append(("two touching", two))
    return out


# ---- sizes, batches, label dtypes -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", ref.SIZES)
def test_sizes(dev, H, W):
    """Every map of the size, B 1-3, int32 and int64 labels, without an image: bit for bit, twice, raw and wrapped."""
    for name, m in maps(H, W):
        want = check(dev, m, what=(name, H, W))
        if name == "two touching":
            assert want["contact"][0, 1] == H == want["contact"][0, 2] and want["open"][0].sum() == 0
        if name == "one id":                                     # every side on the frame, nothing else; n_max above it would do too
            assert want["frame"][0, 7] == 2 * (H + W) and want["area"][0, 7] == H * W
    name, m = maps(H, W)[0]
    check(dev, m, n_max=int(m.max()) + 70, ldtypes=(torch.int32,), what="n_max above every id")


@pytest.mark.parametrize("H,W", [(64, 64), (65, 63)])
def test_every_pixel_its_own_id(dev, H, W):
    """More ids per tile (1024) than the LDS table holds (128 slots, 8 probes): most runs take the path straight to the global
    record, and the result is the same."""
    m = np.stack([ref.every_pixel_its_own(H, W), ref.every_pixel_its_own(W, H).T.copy()]).astype(np.int32)
    img = ref.int_image(5, m.shape)
    want = check(dev, m, img, what="own ids")
    assert (want["area"][:, 1:] == 1).all() and np.array_equal(want["v_sum"][0, 1:], img[0].ravel())
    check(dev, m, image(3, 2, H, W, blobs=4), ldtypes=(torch.int32,), what="own ids, float image")


def test_narrow_image_rows_break_runs(dev):
    """Width 5: a wave's 64 lanes hold one row and 59 lanes outside the image, and the id at the end of a row equals the id at the
    start of the next.  Width 1 and 2 likewise."""
    for W in (5, 2, 1):
        m = np.full((1, 40, W), 3, np.int32) if W == 1 else wrapped_rows(40, W)[None]
        want = check(dev, m, ref.int_image(W, m.shape, 256).astype(np.uint8), what=("narrow", W))
        assert want["bbox"][0, 3].tolist() == [0, 0, 40, W]


# ---- images -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("uint8", "int32", "float32"))
def test_images(dev, kind):
    for H, W in ((5, 17), (65, 63), (37, 300), (129, 97)):
        for name, m in maps(H, W)[:2] + maps(H, W)[4:6]:
            if kind == "uint8":
                img = ref.int_image(H, m.shape, 256).astype(np.uint8)
            elif kind == "int32":
                img = ref.int_image(W, m.shape)
                img[:, 0, 0], img[:, -1, -1] = 65535, 0
            else:
                img = image(H + W, len(m), H, W, blobs=5) - 60.0                     # both signs
                img = img.astype(np.float32)
            check(dev, m, img, ldtypes=(torch.int32,) if (H, W) != (65, 63) else (torch.int32, torch.int64), what=(name, H, W, kind))


def test_float_extremes_and_int64_images(dev):
    """min and max of a float image are exact over signs, zeros and denormals; an int64 image goes in as it is."""
    import functions
    m = np.array([[[1, 1, 1, 2, 2, 0, 0, 3]]], np.int32)
    img = np.array([[[-1.5, 2.0 ** -140, -0.0, 3.0e38, -3.0e38, 0.0, -(2.0 ** -149), 7.0]]], np.float32)
    want = check(dev, m, img, what="extremes")
    assert want["v_min"][0].tolist() == [np.float32(-(2.0 ** -149)), -1.5, np.float32(-3.0e38), 7.0]
    s = functions.cell_sums(torch.from_numpy(m).to(dev), torch.from_numpy(img).to(dev).clamp(0, 9).long())
    assert s.v_sum.dtype == torch.int64 and s.v_sum[0].tolist() == [0, 0, 9, 7] and s.v_max[0].tolist() == [0, 0, 9, 7]


# ---- errors -----------------------------------------------------------------------------------------------------------------

def test_status_counts_what_the_entry_refuses(dev):
    m = np.array([[[1, -1, 9, 2], [2, 2, 1, 0]]], np.int32)
    got = raw_sums(dev, m, n_max=2, expect_status=(2, 0))
    assert got["area"][0].tolist() == [1, 2, 3]                  # the refused pixels count nowhere
    img = np.array([[[1, 65536, 5, -1], [0, 0, 65535, 3]]], np.int32)
    got = raw_sums(dev, np.abs(m) % 3, img, n_max=2, expect_status=(0, 2))
    f = img.astype(np.float32)
    f[0, 0, 0], f[0, 1, 1] = np.nan, np.inf
    raw_sums(dev, np.abs(m) % 3, f, n_max=2, expect_status=(0, 2))


def test_errors(dev, hip):
    import functions
    lab = torch.tensor([[1, 2, 0], [2, 2, 5]], dtype=torch.int32, device=dev)
    img = torch.tensor([[1, 2, 3], [4, 5, 6]], dtype=torch.int32, device=dev)
    assert functions.cell_sums(lab, img).area.tolist() == [1, 1, 3, 0, 0, 1]
    bad = lab.clone()
    bad[0, 0] = -1
    with pytest.raises(ValueError, match="negative"):
        functions.cell_sums(bad)
    with pytest.raises(ValueError, match="outside"):
        functions.cell_sums(bad, n_max=5)
    with pytest.raises(ValueError, match="outside"):
        functions.cell_sums(lab, n_max=4)
    for v in (65536, -1):
        wrong = img.clone()
        wrong[1, 1] = v
        with pytest.raises(ValueError, match="65536"):
            functions.cell_sums(lab, wrong)
    nan = img.float()
    nan[0, 2] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        functions.cell_sums(lab, nan)
    with pytest.raises(ValueError, match="shape"):
        functions.cell_sums(lab, img[:1])
    with pytest.raises(ValueError):
        functions.cell_sums(lab.float())
    with pytest.raises(ValueError, match="n_max"):
        functions.cell_sums(lab, n_max=-1)
    with pytest.raises(NotImplementedError):
        functions.cell_sums(lab.cpu())
    with pytest.raises(NotImplementedError):
        functions.cell_sums(lab, img.cpu())
    with pytest.raises(NotImplementedError):
        functions.cell_props(lab.cpu())


def test_a_rejected_call_writes_nothing(dev, hip):
    L = hip.lib()
    a = guarded.Arena(dev)
    B, H, W, n_max = 2, 9, 11, 4
    N = n_max + 1
    lab = a.inp(torch.ones(B, H, W, dtype=torch.int32), "labels")
    img = a.inp(torch.ones(B, H, W, dtype=torch.int32), "image")
    area, bbox = a.out((B, N), torch.int64, "area"), a.out((B, N, 4), torch.int32, "bbox")
    moments, edges = a.out((B, N, 5), torch.int64, "moments"), a.out((B, N, 3), torch.int64, "edges")
    vsum, vrange = a.out((B, N, 2), torch.int64, "vsum"), a.out((B, N, 2), torch.int32, "vrange")
    present, status = a.out((B, N), torch.uint8, "present"), a.out((B, 2), torch.int64, "status")
    scratch = a.scratch(L.unet_cell_sums_scratch_bytes(B, n_max), "scratch")
    out_map, table = a.out((B, H, W), torch.int32, "out"), a.inp(torch.zeros(N, dtype=torch.int32), "map")
    st = hip.stream(dev)
    p = a.ptr
    good = dict(lab=p(lab), ld=2, img=p(img), idt=2, B=B, H=H, W=W, n=n_max, area=p(area), bbox=p(bbox), mom=p(moments), edges=p(edges),
                vsum=p(vsum), vrange=p(vrange), present=p(present), status=p(status), scratch=p(scratch))
    for bad in ({"ld": 1}, {"ld": 3}, {"ld": -1}, {"idt": 4}, {"idt": -1}, {"lab": None}, {"area": None}, {"bbox": None}, {"mom": None},
                {"edges": None}, {"vsum": None}, {"vrange": None}, {"present": None}, {"status": None}, {"scratch": None}, {"B": 0},
                {"H": 32769, "W": 1}, {"H": 1, "W": 32769}, {"B": 70000}, {"n": -1}, {"n": 1 << 24}):
        kw = dict(good, **bad)
        rc = L.unet_cell_sums(kw["lab"], kw["ld"], kw["img"], kw["idt"], kw["B"], kw["H"], kw["W"], kw["n"], kw["area"], kw["bbox"], kw["mom"],
                              kw["edges"], kw["vsum"], kw["vrange"], kw["present"], kw["status"], kw["scratch"], st)
        rejected(hip, rc, a, area, bbox, moments, edges, vsum, vrange, present, status, scratch)
        assert b"unet_cell_sums" in L.unet_last_error()
    good = dict(lab=p(lab), ld=2, B=B, H=H, W=W, map=p(table), n=n_max, stride=0, out=p(out_map), status=p(status))
    for bad in ({"ld": 1}, {"lab": None}, {"map": None}, {"out": None}, {"status": None}, {"W": 0}, {"H": 40000}, {"n": -1}, {"stride": 3},
                {"stride": -1}):
        kw = dict(good, **bad)
        rc = L.unet_remap_labels(kw["lab"], kw["ld"], kw["B"], kw["H"], kw["W"], kw["map"], kw["n"], kw["stride"], kw["out"], kw["status"], st)
        rejected(hip, rc, a, out_map, status)
        assert b"unet_remap_labels" in L.unet_last_error()


# ---- streams, props, select -------------------------------------------------------------------------------------------------

def test_side_stream_and_props(dev):
    """cell_sums and cell_props on the default stream and on another one: the integers identical; the properties those that
    props_from_sums makes of the reference table."""
    import functions
    gt = np.stack([instances_ref.cells_case(s, 40, 200, 260, stride=2)[0] for s in (4, 5)])
    img = image(9, 2, 200, 260, blobs=12)
    g, x = torch.from_numpy(gt).to(dev), torch.from_numpy(img).to(dev)
    s0 = functions.cell_sums(g, x)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        s1 = functions.cell_sums(g, x)
        p1 = functions.cell_props(g, x)
    torch.cuda.current_stream(dev).wait_stream(side)
    side.synchronize()
    want = ref.sums_batch(gt, img)
    for k in EXACT + ("v_min", "v_max"):
        assert torch.equal(getattr(s0, k), getattr(s1, k)) and np.array_equal(getattr(s1, k).cpu().numpy(), want[k]), k
    pw = functions.props_from_sums(functions.CellSums(**want))
    for f in ("area", "centroid", "moments_central", "axis_major", "axis_minor", "eccentricity", "orientation", "perimeter", "extent",
              "contact_fraction", "min", "max"):
        assert np.array_equal(getattr(p1, f), getattr(pw, f), equal_nan=True), f
    on = want["present"]
    assert np.allclose(p1.mean[on], pw.mean[on], rtol=1e-12, atol=0) and np.isnan(p1.mean[~on]).all() and on.sum() > 30 and (~on).sum() > 10
    single = functions.cell_props(g[0], x[0])
    assert single.area.shape == (int(gt[0].max()) + 1,) and np.array_equal(single.area, pw.area[0][:int(gt[0].max()) + 1], equal_nan=True)


def raw_remap(dev, labels, table, ldtype=torch.int32, expect_bad=0):
    import _hip
    a = guarded.Arena(dev)
    B, H, W = labels.shape
    lab, tab = a.inp(torch.from_numpy(labels).to(ldtype), "labels"), a.inp(torch.from_numpy(table.astype(np.int32)), "map")
    out, status = a.out((B, H, W), torch.int32, "out"), a.out((B,), torch.int64, "status")
    _hip.run("unet_remap_labels", dev, a.ptr(lab), CODE[ldtype], B, H, W, a.ptr(tab), table.shape[-1] - 1, table.shape[-1] if table.ndim == 2 else 0,
             a.ptr(out), a.ptr(status))
    a.verify(out, status)
    assert int(status.sum()) == expect_bad
    return out.cpu().numpy()


def test_select_cells(dev):
    import functions
    for H, W in ((1, 1), (5, 17), (65, 63), (129, 97)):
        name, m = maps(H, W)[0]
        n_max = int(m.max()) + 3
        rs = np.random.RandomState(H)
        for keep in (rs.rand(n_max + 1) < 0.5, rs.rand(len(m), n_max + 1) < 0.5, np.zeros(n_max + 1, bool), np.ones(n_max + 1, bool)):
            for ldtype in (torch.int32, torch.int64):
                lab, k = torch.from_numpy(m).to(dev).to(ldtype), torch.from_numpy(keep).to(dev)
                for renumber in (False, True):
                    got = functions.select_cells(lab, k, renumber=renumber)
                    want = ref.select(m, keep, renumber)
                    assert got.dtype == torch.int32 and got.shape == m.shape and np.array_equal(got.cpu().numpy(), want), (H, W, renumber)
                    if not renumber and keep.ndim == 1:
                        assert np.array_equal(want, np.where(keep[m] & (m > 0), m, 0))
            table = np.where(keep, np.arange(n_max + 1), 0)
            table[..., 0] = 0
            assert np.array_equal(raw_remap(dev, m, table), ref.select(m, keep))
        assert not functions.select_cells(torch.from_numpy(m).to(dev), torch.zeros(n_max + 1, dtype=torch.bool, device=dev)).any()
        one = functions.select_cells(torch.from_numpy(m[0]).to(dev), torch.ones(n_max + 1, dtype=torch.bool, device=dev))
        assert one.shape == (H, W) and np.array_equal(one.cpu().numpy(), m[0])
    m = np.array([[[0, 1, 5, -2, 2]]], np.int32)
    assert raw_remap(dev, m, np.arange(3) * 10, expect_bad=2).tolist() == [[[0, 10, 0, 0, 20]]]
    lab = torch.from_numpy(m).to(dev)
    with pytest.raises(ValueError, match="outside"):
        functions.select_cells(lab, torch.ones(3, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError, match="bool"):
        functions.select_cells(lab, torch.ones(3, device=dev))
    with pytest.raises(ValueError, match="images"):
        functions.select_cells(lab, torch.ones(2, 6, dtype=torch.bool, device=dev))
    with pytest.raises(NotImplementedError):
        functions.select_cells(lab, torch.ones(6, dtype=torch.bool))


def test_select_by_a_measured_property(dev):
    """The use the op is for: measure, decide on the host, drop on the device."""
    import functions
    gt = instances_ref.cells_case(2, 30, 150, 170)[0]
    lab = torch.from_numpy(gt).to(dev)
    p = functions.cell_props(lab)
    areas = np.bincount(gt.ravel())
    thr = int(np.median(areas[1:][areas[1:] > 0]))
    keep = np.nan_to_num(p.area, nan=0.0) >= thr
    out = functions.select_cells(lab, torch.from_numpy(keep).to(dev), renumber=True)
    kept = [i for i in range(1, len(areas)) if areas[i] >= thr]
    assert 0 < len(kept) < (areas[1:] > 0).sum() and int(out.max()) == len(kept)
    assert np.array_equal(np.bincount(out.cpu().numpy().ravel())[1:], areas[kept])


# ---- tester.segment(measure=True) -------------------------------------------------------------------------------------------

def test_segment_measure(dev, net):
    import functions
    import tester
    x = torch.from_numpy(image(30, 1, 100, 130, blobs=9)[0]).to(dev)
    kw = dict(tile_size=188, max_batch=64)
    with pytest.raises(ValueError, match="measure"):
        tester.segment(net, x, measure=True, **kw)
    with pytest.raises(ValueError, match="measure"):
        tester.segment(net, x, return_instances=True, measure="yes", **kw)
    m0, i0 = tester.segment(net, x, return_instances=True, **kw)
    out = tester.segment(net, x, return_instances=True, measure=True, **kw)
    assert len(out) == 3
    m1, i1, p1 = out
    assert torch.equal(m0, m1) and torch.equal(i0, i1) and isinstance(p1, functions.CellProps)
    counts = torch.bincount(i1.flatten().long()).cpu().numpy()
    assert int(i1.max()) >= 1 and p1.area.shape == counts.shape and np.array_equal(np.nan_to_num(p1.area, nan=0.0), counts.astype(np.float64))
    want = functions.cell_props(i1, x)
    assert np.array_equal(p1.centroid, want.centroid, equal_nan=True) and np.array_equal(p1.min, want.min) and np.array_equal(p1.max, want.max)
    out = tester.segment(net, x[None], return_probs=True, return_instances=True, measure=True, clean={"min_area": 5}, shape_split=2.0, **kw)
    assert len(out) == 4
    m2, pr2, i2, p2 = out
    counts = torch.bincount(i2.flatten().long()).cpu().numpy()
    assert p2.area.shape == (1, len(counts)) and np.array_equal(np.nan_to_num(p2.area[0], nan=0.0), counts.astype(np.float64))
