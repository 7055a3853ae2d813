"""The mask clean-up on the device (functions.clean_mask / fill_holes / remove_small -> unet_clean_mask;
functions.label_cells(connectivity=8) -> unet_label_components_conn; tester.segment(clean=...)) against the numpy/scipy
restatement tests/clean_ref.py (pinned to binary_fill_holes with the dual structure, ndimage.label, np.bincount and hand-worked
answers by tests/test_clean_cpu.py, which also asserts that the busy inputs hold a filled hole, one too large, a pocket open to
the frame, an island in a hole, a small, a border and a kept cell and a pixel the connectivity decides).  Everything is an integer
and is compared bit for bit.  Every pointer handed to the raw entry points is a poisoned guarded.Arena buffer."""
import functools
import itertools

import numpy as np
import pytest
import torch

import clean_ref as ref
import guarded
import instances_ref
from gpu_support import dev, net, hip, image, rejected  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CODE = {torch.int64: 0, torch.float32: 1, torch.int32: 2, torch.uint8: 3}
DTYPES = (torch.uint8, torch.int64, torch.float32, torch.int32)
FEW = ({}, {"max_hole_area": 6, "min_area": 5, "drop_border": True}, {"fill_holes": False, "min_area": 5})
EVERY = [dict(max_hole_area=a, min_area=s, drop_border=d) for a in ref.HOLE_AREAS for s in ref.MIN_AREAS for d in (False, True)] + \
        [dict(fill_holes=False, min_area=s, drop_border=d) for s in ref.MIN_AREAS for d in (False, True)]


@functools.lru_cache(maxsize=None)
def cases(H, W):
    return ref.size_cases(H, W)


def frozen(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def want_clean(H, W, k, conn, opts):
    return ref.clean_batch(cases(H, W)[k][1], connectivity=conn, **dict(opts))


@functools.lru_cache(maxsize=None)
def want_labels(H, W, k, conn, phase):
    return ref.label_batch(cases(H, W)[k][1], conn, phase)


def raw_clean(dev, mask, dtype=torch.uint8, connectivity=4, fill_holes=True, max_hole_area=None, min_area=0, drop_border=False,
              with_action=True):
    """unet_clean_mask on guarded buffers: a dict like clean_ref.clean_batch's (action None without it); mask numpy [B,H,W]."""
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = mask.shape
    m = a.inp(torch.from_numpy(mask).to(dtype), "mask")
    out = a.out((B, H, W), dtype, "out")
    action = a.out((B, H, W), torch.uint8, "action") if with_action else None
    info = a.out((B, 7), torch.int64, "info")
    scratch = a.scratch(L.unet_clean_mask_scratch_bytes(B, H, W), "scratch")
    _hip.run("unet_clean_mask", dev, a.ptr(m), CODE[dtype], B, H, W, connectivity, int(fill_holes), -1 if max_hole_area is None else max_hole_area,
             min_area, int(drop_border), a.ptr(out), a.ptr(action), a.ptr(info), a.ptr(scratch))
    a.verify(action)                                         # out may hold 0xFF.. only as a value of the input; info never does
    a.assert_written(info)
    assert torch.equal(m.cpu(), torch.from_numpy(mask).to(dtype))
    return {"out": out.cpu().numpy(), "action": None if action is None else action.cpu().numpy(), "info": info.cpu().numpy()}


def raw_labels(dev, mask, connectivity, phase, dtype=torch.uint8):
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = mask.shape
    m = a.inp(torch.from_numpy(mask).to(dtype), "mask")
    labels, n = a.out((B, H, W), torch.int32, "labels"), a.out((B,), torch.int32, "n")
    scratch = a.scratch(L.unet_label_components_conn_scratch_bytes(B, H, W), "scratch")
    _hip.run("unet_label_components_conn", dev, a.ptr(m), CODE[dtype], B, H, W, connectivity, phase, a.ptr(labels), a.ptr(n), a.ptr(scratch))
    a.verify(labels, n)
    return labels.cpu().numpy(), n.cpu().numpy()


def same(got, want, what):
    for k in ("info", "action", "out"):
        if got[k] is not None:
            assert got[k].dtype == want[k].dtype or k == "out", (what, k)
            assert np.array_equal(got[k], want[k].astype(got[k].dtype)), (what, k)


def wrapped(dev, mask, dtype=torch.uint8, **kw):
    """functions.clean_mask with everything returned, as a dict like raw_clean's."""
    import functions
    t = torch.from_numpy(mask).to(dev).to(dtype)
    out, info, action = functions.clean_mask(t, return_info=True, return_action=True, **kw)
    assert out.dtype == dtype and out.shape == mask.shape and out.is_cuda and action.dtype == torch.uint8 and action.shape == mask.shape
    assert isinstance(info, functions.CleanInfo) and all(v.dtype == np.int64 and v.shape == (mask.shape[0] if mask.ndim == 3 else 1,) for v in info)
    return {"out": out.cpu().numpy(), "action": action.cpu().numpy(), "info": np.stack(info, axis=1)}


def check_size(dev, H, W, ks, options):
    import functions
    seen = np.zeros(7, np.int64)
    for k in ks:
        name, m = cases(H, W)[k]
        for conn in (4, 8):
            for kw in options:
                want = want_clean(H, W, k, conn, frozen(kw))
                same(raw_clean(dev, m, connectivity=conn, **kw), want, (name, conn, kw))
                same(wrapped(dev, m, connectivity=conn, **kw), want, (name, conn, kw, "wrapper"))
                seen += want["info"].sum(axis=0)
            for phase in (0, 1):
                labels, n = raw_labels(dev, m, conn, phase)
                want_l, want_n = want_labels(H, W, k, conn, phase)
                assert np.array_equal(n, want_n) and np.array_equal(labels, want_l), (name, conn, phase)
            got, n = functions.label_cells(torch.from_numpy(m).to(dev), connectivity=conn)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want_labels(H, W, k, conn, 1)[0]), (name, conn)
            assert np.array_equal(n.cpu().numpy(), want_labels(H, W, k, conn, 1)[1])
    return seen


# ---- sizes, batches, options ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", ref.SIZES)
def test_sizes(dev, H, W):
    """out, action, info and the labels of both phases bit for bit at both connectivities, B 1-4 (the batch of four holds an empty
    and a full image), through the raw entry points and through the wrappers; [H,W] inputs too."""
    import functions
    seen = check_size(dev, H, W, range(4), FEW)
    assert seen.all() or H * W < 1000                        # every count was non-zero somewhere
    m = cases(H, W)[0][1][0]
    t = torch.from_numpy(m).to(dev)
    got = functions.clean_mask(t, connectivity=8)
    assert torch.is_tensor(got) and got.shape == (H, W) and np.array_equal(got.cpu().numpy(), want_clean(H, W, 0, 8, ())["out"][0])
    labels, n = functions.label_cells(t, connectivity=8)
    assert labels.shape == (H, W) and n.shape == (1,) and np.array_equal(labels.cpu().numpy(), want_labels(H, W, 0, 8, 1)[0][0])


def test_the_big_size_once(dev):
    H, W = ref.BIG
    assert check_size(dev, H, W, (2,), FEW[:2]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_options_and_dtypes(dev, dtype):
    """65 x 66, the batch of four: every max_hole_area x min_area x drop_border, and fill off, at both connectivities, for each mask
    dtype.  The masks hold values other than 1 (a kept pixel keeps its value, a filled one becomes 1)."""
    import functions
    name, m = cases(65, 66)[3]
    values = m * (1 + (np.arange(m.size).reshape(m.shape) % 3)).astype(np.uint8)       # 1, 2, 3 on the foreground
    for conn, kw in itertools.product((4, 8), EVERY):
        want = ref.clean_batch(values, connectivity=conn, **kw)
        assert np.array_equal(want["action"], want_clean(65, 66, 3, conn, frozen(kw))["action"])
        same(raw_clean(dev, values, dtype, conn, **kw), want, (conn, kw))
    same(wrapped(dev, values, dtype, connectivity=8, max_hole_area=6, min_area=5, drop_border=True),
         ref.clean_batch(values, connectivity=8, max_hole_area=6, min_area=5, drop_border=True), "wrapper")
    for conn in (4, 8):
        for phase in (0, 1):
            labels, n = raw_labels(dev, values, conn, phase, dtype)
            assert np.array_equal(labels, want_labels(65, 66, 3, conn, phase)[0]) and np.array_equal(n, want_labels(65, 66, 3, conn, phase)[1])
    if dtype == torch.float32:                               # foreground is any value != 0
        t = torch.from_numpy(m).to(dev).float() * -0.25
        got = functions.clean_mask(t, min_area=5)
        want = want_clean(65, 66, 3, 4, frozen({"min_area": 5}))
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), np.where(want["action"] == 1, -0.25, want["action"] == 2).astype(np.float32))


def test_bool_masks_and_the_thin_wrappers(dev):
    import functions
    name, m = cases(65, 66)[1]
    t = torch.from_numpy(m).to(dev)
    got = functions.clean_mask(t.bool(), min_area=5, drop_border=True)
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want_clean(65, 66, 1, 4, frozen({"min_area": 5, "drop_border": True}))["out"] != 0)
    for conn in (4, 8):
        assert np.array_equal(functions.fill_holes(t, connectivity=conn).cpu().numpy(), want_clean(65, 66, 1, conn, ())["out"])
        assert np.array_equal(functions.fill_holes(t, 6, conn).cpu().numpy(), want_clean(65, 66, 1, conn, frozen({"max_hole_area": 6}))["out"])
        assert np.array_equal(functions.remove_small(t, 5, conn).cpu().numpy(),
                              want_clean(65, 66, 1, conn, frozen({"fill_holes": False, "min_area": 5}))["out"])
    labels, n = functions.label_cells(t.bool(), connectivity=8)
    assert np.array_equal(labels.cpu().numpy(), want_labels(65, 66, 1, 8, 1)[0])


# ---- fixed cases --------------------------------------------------------------------------------------------------------------

def info_of(dev, m, **kw):
    got = raw_clean(dev, m[None], **kw)
    same(got, ref.clean_batch(m[None], **kw), kw)
    return dict(zip(ref.INFO, got["info"][0].tolist()))


def test_hand_worked_cases(dev):
    """The cases tests/test_clean_cpu.py works by hand, with the same numbers."""
    m = ref.checkerboard()
    i4, i8 = info_of(dev, m, connectivity=4), info_of(dev, m, connectivity=8)
    assert (i4["holes_filled"], i4["cells_kept"]) == (0, 2048) and (i8["holes_filled"], i8["pixels_filled"], i8["cells_kept"]) == (1922, 1922, 1)
    assert raw_labels(dev, m[None], 4, 1)[1].tolist() == [2048] and raw_labels(dev, m[None], 8, 1)[1].tolist() == [1]
    for anti in (False, True):                               # the two pairs across the corner of four tiles
        d = ref.diagonal(64, anti)
        labels, n = raw_labels(dev, d[None], 8, 1)
        assert n.tolist() == [1] and np.array_equal(labels[0], d.astype(np.int32))
        assert raw_labels(dev, d[None], 4, 1)[1].tolist() == [64]
        labels, n = raw_labels(dev, (1 - d)[None], 8, 0)     # the same pixels as the off phase
        assert n.tolist() == [1] and np.array_equal(labels[0], d.astype(np.int32))
    m = ref.diamond()
    i4, i8 = info_of(dev, m, connectivity=4), info_of(dev, m, connectivity=8)
    assert (i4["cells_kept"], i4["holes_filled"]) == (80, 0) and (i8["cells_kept"], i8["holes_filled"], i8["pixels_filled"]) == (1, 1, 761)
    m = ref.nested()
    i = info_of(dev, m)
    assert (i["holes_filled"], i["pixels_filled"], i["cells_kept"]) == (2, 380, 1)
    i = info_of(dev, m, max_hole_area=64)
    assert (i["holes_filled"], i["pixels_filled"], i["cells_kept"]) == (1, 60, 2)
    assert info_of(dev, m, min_area=1025)["cells_small"] == 1 and info_of(dev, m, min_area=1024)["cells_kept"] == 1
    i = info_of(dev, m, fill_holes=False, min_area=5)
    assert (i["cells_small"], i["pixels_small"]) == (1, 4)
    m = ref.diagonal_pocket()
    assert info_of(dev, m, connectivity=4)["holes_filled"] == 0 and info_of(dev, m, connectivity=8)["pixels_filled"] == 9
    m = ref.two_squares()
    i4, i8 = info_of(dev, m, drop_border=True, connectivity=4), info_of(dev, m, drop_border=True, connectivity=8)
    assert (i4["cells_border"], i4["pixels_border"], i4["cells_kept"]) == (1, 9, 1)
    assert (i8["cells_border"], i8["pixels_border"], i8["cells_kept"]) == (1, 18, 0)


@pytest.mark.parametrize("kind", ("serpentine", "comb"))
def test_long_chains_in_both_phases(dev, kind):
    """instances_ref's serpentine and comb at 129 x 127 and 65 x 66, as the foreground and as the background: the longest union
    chains an image allows, through every tile border."""
    for H, W in ((129, 127), (65, 66)):
        m = np.stack([getattr(instances_ref, kind)(H, W), getattr(instances_ref, kind)(W, H).T.copy()]).astype(np.uint8)
        for mask in (m, 1 - m):
            for conn in (4, 8):
                for phase in (0, 1):
                    labels, n = raw_labels(dev, mask, conn, phase)
                    want_l, want_n = ref.label_batch(mask, conn, phase)
                    assert np.array_equal(n, want_n) and np.array_equal(labels, want_l), (H, W, conn, phase)
                for kw in FEW[:2]:
                    same(raw_clean(dev, mask, connectivity=conn, **kw), ref.clean_batch(mask, connectivity=conn, **kw), (H, W, conn, kw))


# ---- consistency ------------------------------------------------------------------------------------------------------------------

def test_connectivity_4_is_the_existing_op(dev):
    """label_cells(m, connectivity=4) is label_cells(m), and the new entry at phase 1, connectivity 4 equals unet_label_components
    bit for bit."""
    import functions
    for H, W in ((65, 66), (129, 127)):
        for k, (name, m) in enumerate(cases(H, W)):
            t = torch.from_numpy(m).to(dev)
            old, new = functions.label_cells(t), functions.label_cells(t, connectivity=4)
            assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])
            labels, n = raw_labels(dev, m, 4, 1, torch.int64)
            assert np.array_equal(labels, old[0].cpu().numpy()) and np.array_equal(n, old[1].cpu().numpy()), name


def test_both_entry_points_give_the_same_labels_and_counts(dev):
    """unet_label_components and unet_label_components_conn(4, 1) on one float32 mask of 3 images, each on guarded buffers: the
    same labels and the same n_objects."""
    import _hip
    rng = np.random.default_rng(11)
    for H, W in ((65, 66), (31, 33)):
        m = (rng.random((3, H, W)) < 0.55).astype(np.float32)
        a = guarded.Arena(dev)
        t = a.inp(torch.from_numpy(m), "mask")
        labels, n = a.out((3, H, W), torch.int32, "labels"), a.out((3,), torch.int32, "n")
        scratch = a.scratch(_hip.lib().unet_label_components_scratch_bytes(3, H, W), "scratch")
        _hip.run("unet_label_components", dev, a.ptr(t), CODE[torch.float32], 3, H, W, a.ptr(labels), a.ptr(n), a.ptr(scratch))
        a.verify(labels, n)
        labels_conn, n_conn = raw_labels(dev, m, 4, 1, torch.float32)
        assert np.array_equal(n.cpu().numpy(), n_conn) and np.array_equal(labels.cpu().numpy(), labels_conn), (H, W)
        assert n_conn.min() > 1                              # the mask is no trivial one


def test_without_the_action_plane(dev):
    name, m = cases(129, 127)[3]
    for conn, kw in itertools.product((4, 8), FEW):
        got = raw_clean(dev, m, connectivity=conn, with_action=False, **kw)
        assert got["action"] is None
        same(got, want_clean(129, 127, 3, conn, frozen(kw)), (conn, kw))


def test_determinism(dev):
    """One 257 x 255 busy case five times, once on a side stream: bit-identical."""
    import functions
    H, W = ref.BIG
    name, m = cases(H, W)[2]
    kw = {"max_hole_area": 6, "min_area": 5, "drop_border": True}
    want, want_l = want_clean(H, W, 2, 8, frozen(kw)), want_labels(H, W, 2, 8, 1)
    t = torch.from_numpy(m).to(dev)
    call = lambda: (functions.clean_mask(t, connectivity=8, return_info=True, return_action=True, **kw), functions.label_cells(t, connectivity=8))
    runs = []
    for k in range(5):
        if k == 3:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                got = call()
            torch.cuda.current_stream(dev).wait_stream(side)
        else:
            got = call()
        runs.append(got)
    for (out, info, action), (labels, n) in runs:
        assert np.array_equal(out.cpu().numpy(), want["out"]) and np.array_equal(action.cpu().numpy(), want["action"])
        assert np.array_equal(np.stack(info, axis=1), want["info"])
        assert np.array_equal(labels.cpu().numpy(), want_l[0]) and np.array_equal(n.cpu().numpy(), want_l[1])


def test_a_rejected_call_writes_nothing(dev, hip):
    L = hip.lib()
    a = guarded.Arena(dev)
    B, H, W = 2, 33, 40
    m = a.inp(torch.ones(B, H, W, dtype=torch.uint8), "mask")
    out, action, info = a.out((B, H, W), torch.uint8, "out"), a.out((B, H, W), torch.uint8, "action"), a.out((B, 7), torch.int64, "info")
    labels, n = a.out((B, H, W), torch.int32, "labels"), a.out((B,), torch.int32, "n")
    scratch = a.scratch(L.unet_clean_mask_scratch_bytes(B, H, W), "scratch")
    st = hip.stream(dev)
    p = a.ptr
    good = dict(mask=p(m), dtype=3, B=B, H=H, W=W, conn=4, fill=1, hole=-1, small=0, border=0, out=p(out), action=p(action), info=p(info),
                scratch=p(scratch))
    for bad in ({"conn": 6}, {"conn": 0}, {"dtype": 4}, {"dtype": -1}, {"hole": -2}, {"small": -1}, {"mask": None}, {"out": None},
                {"info": None}, {"scratch": None}, {"B": 0}, {"H": 70000, "W": 1}, {"B": 70000}):
        kw = dict(good, **bad)
        rc = L.unet_clean_mask(kw["mask"], kw["dtype"], kw["B"], kw["H"], kw["W"], kw["conn"], kw["fill"], kw["hole"], kw["small"], kw["border"],
                               kw["out"], kw["action"], kw["info"], kw["scratch"], st)
        rejected(hip, rc, a, out, action, info, scratch)
    good = dict(mask=p(m), dtype=3, B=B, H=H, W=W, conn=8, phase=1, labels=p(labels), n=p(n), scratch=p(scratch))
    for bad in ({"conn": 6}, {"dtype": 4}, {"phase": 2}, {"phase": -1}, {"mask": None}, {"labels": None}, {"n": None}, {"scratch": None},
                {"W": 0}, {"H": 65535, "W": 65535}, {"B": 70000}):
        kw = dict(good, **bad)
        rc = L.unet_label_components_conn(kw["mask"], kw["dtype"], kw["B"], kw["H"], kw["W"], kw["conn"], kw["phase"], kw["labels"], kw["n"],
                                          kw["scratch"], st)
        rejected(hip, rc, a, labels, n, scratch)


def test_errors(dev):
    import functions
    m = torch.ones(2, 9, 7, dtype=torch.uint8, device=dev)
    with pytest.raises(NotImplementedError):
        functions.clean_mask(m.cpu())
    with pytest.raises(NotImplementedError):
        functions.label_cells(m.cpu(), connectivity=8)
    with pytest.raises(ValueError, match="connectivity"):
        functions.clean_mask(m, connectivity=6)
    with pytest.raises(ValueError, match="connectivity"):
        functions.label_cells(m, connectivity=6)
    with pytest.raises(ValueError, match="min_area"):
        functions.clean_mask(m, min_area=-1)
    with pytest.raises(ValueError, match="max_hole_area"):
        functions.clean_mask(m, max_hole_area=-1)


# ---- tester.segment(clean=...) and functions.shape_seeds --------------------------------------------------------------------------

def check_segment(dev, model, clean, kw_clean, mask_expected=True, **kw):
    import functions
    import tester
    x = torch.from_numpy(image(30, 1, 100, 130, blobs=9)[0]).to(dev)
    kw = dict(tile_size=188, max_batch=64, **kw)
    m0, p0 = tester.segment(model, x, return_probs=True, **kw)
    assert bool((m0 != 0).any()) or not mask_expected
    want = functions.clean_mask(m0, **kw_clean)
    assert np.array_equal(want.cpu().numpy(), ref.clean(m0.cpu().numpy(), **kw_clean)["out"])
    m1 = tester.segment(model, x, clean=clean, **kw)                                  # no return_instances needed
    assert torch.is_tensor(m1) and m1.dtype == m0.dtype and torch.equal(m1, want)
    m2, p2, i2 = tester.segment(model, x, clean=clean, return_probs=True, return_instances=True, **kw)
    assert torch.equal(m2, want) and torch.equal(p2, p0) and torch.equal(i2, functions.label_cells(want)[0])
    m3, i3 = tester.segment(model, x, clean=clean, return_instances=True, shape_split=2.0, **kw)
    assert torch.equal(m3, want) and torch.equal(i3, tester.split_by_shape(want, 2.0))
    return m0, want


def test_segment_clean(dev, net):
    import tester
    m0, m1 = check_segment(dev, net, True, {})
    print("mask %d px, cleaned %d px" % (int((m0 != 0).sum()), int((m1 != 0).sum())))
    check_segment(dev, net, {"min_area": 30, "drop_border": True, "connectivity": 8, "max_hole_area": 50},
                  {"min_area": 30, "drop_border": True, "connectivity": 8, "max_hole_area": 50})
    check_segment(dev, net, False, {"fill_holes": False})                             # off: the mask as it is
    x = torch.from_numpy(image(31, 1, 100, 130, blobs=9)[0]).to(dev)
    for bad in ("yes", {"h": 1}, {"min_area": -1}, {"connectivity": 5}):
        with pytest.raises(ValueError, match="clean"):
            tester.segment(net, x, tile_size=188, clean=bad)


def test_segment_clean_with_views(dev, net):
    """The seed-0 two-class net leaves an empty mask under views='flips' (tests/test_split_gpu.py has the reason), so what this
    case holds is that clean runs after a views call and returns what clean_mask makes of that call's mask."""
    check_segment(dev, net, {"min_area": 5}, {"min_area": 5}, mask_expected=False, views="flips")


def test_segment_clean_on_three_classes(dev):
    import functions
    import multiclass_ref
    import network
    import tester
    net3 = network.Unet(n_classes=3)
    net3.load_state_dict({k: torch.from_numpy(v) for k, v in multiclass_ref.head_params(3, seed=1).items()})
    net3 = net3.to(dev)
    x = torch.from_numpy((np.random.RandomState(3).rand(2, 130, 201) * 255).astype(np.float32)).to(dev)
    for fills in (True, {"min_area": 5}, {"fill_holes": True}):
        with pytest.raises(ValueError, match="class"):
            tester.segment(net3, x, tile_size=220, max_batch=3, clean=fills)
    kw = {"fill_holes": False, "min_area": 5, "drop_border": True}
    m0 = tester.segment(net3, x, tile_size=220, max_batch=3)
    m1 = tester.segment(net3, x, tile_size=220, max_batch=3, clean=kw)
    want = ref.clean_batch(m0.cpu().numpy(), **kw)
    assert np.array_equal(m1.cpu().numpy(), want["out"]) and torch.equal(m1, functions.clean_mask(m0, **kw))
    assert bool(((m1 == m0) | (m1 == 0)).all())                                      # a kept pixel keeps its class


def test_a_hole_over_splits_and_filling_it_mends_that(dev):
    import functions
    m = torch.from_numpy(ref.ring_cell()).to(dev)
    assert int(functions.shape_seeds(m, 2.0)[1]) > 1
    filled = functions.fill_holes(m)
    assert np.array_equal(filled.cpu().numpy(), ref.clean(ref.ring_cell())["out"]) and int(functions.shape_seeds(filled, 2.0)[1]) == 1
