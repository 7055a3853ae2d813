"""Boundary scores on the device (functions.mask_boundary / surface_sums / boundary_scores -> unet_mask_boundary, unet_surface_sums)
against the Python-integer restatement tests/boundary_ref.py (pinned to scipy, numpy.percentile and hand-worked answers by
tests/test_boundary_cpu.py).  Every integer word of the record, the contour planes and the d2 planes are compared bit for bit; the
fp64 sum must lie within (n + 2) 2^-53 of the fsum reference, relative: one rounding of up to 1 ulp per square root and 2^-53
relative per addition of non-negative terms.  Every case runs twice and must be bit-equal across the two runs.  Every pointer
handed to the raw entry points is a poisoned guarded.Arena buffer, and the inputs must be unchanged afterwards.  The d2 planes hold
-1 off the contour, which as an int32 is the arena's poison: they start from a second pattern, UNWRITTEN, and none of it may be left."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import boundary_ref as ref
import guarded
import shape_ref
from gpu_support import dev, hip, rejected  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CODE = {torch.int64: 0, torch.float32: 1, torch.int32: 2, torch.uint8: 3}
EDGE = {"ignore": 0, "background": 1}
U8 = torch.uint8
UNWRITTEN = 0x5A5A5A5A
_want = {}


def want(pred, gt, tolerances=(1.0,), percentile=95, select=None, connectivity=4, edge="background"):
    """boundary_ref.surface of every image of [B,H,W] masks, computed once per input and rule"""
    key = (pred.tobytes(), gt.tobytes(), pred.shape, str(pred.dtype), tuple(tolerances), percentile, select, connectivity, edge)
    if key not in _want:
        _want[key] = [ref.surface(p, g, tolerances, percentile, select, connectivity, edge) for p, g in zip(pred, gt)]
    return _want[key]


def raw_contour(dev, mask, dtype=U8, select=None, connectivity=4, edge="background"):
    """unet_mask_boundary on guarded buffers -> uint8 [B,H,W]"""
    import _hip
    a = guarded.Arena(dev)
    B, H, W = mask.shape
    src = torch.from_numpy(mask).to(dtype)
    m, out = a.inp(src, "mask"), a.out((B, H, W), U8, "contour")
    _hip.run("unet_mask_boundary", dev, a.ptr(m), CODE[dtype], -1 if select is None else select, B, H, W, connectivity, EDGE[edge], a.ptr(out))
    a.verify(out)
    assert torch.equal(m.cpu(), src)
    return out.cpu().numpy()


def raw_sums(dev, pred, gt, dtypes=(U8, U8), tolerances=(1.0,), percentile=95, select=None, connectivity=4, edge="background", maps=(True, True)):
    """unet_surface_sums on guarded buffers -> (record int64 [B,2,10], [d2 pred -> gt, d2 gt -> pred] int32 [B,H,W] or None)"""
    import _hip
    L = _hip.lib()
    a = guarded.Arena(dev)
    B, H, W = pred.shape
    srcs = [torch.from_numpy(m).to(t) for m, t in zip((pred, gt), dtypes)]
    p, g = a.inp(srcs[0], "pred"), a.inp(srcs[1], "gt")
    record = a.out((B, 2, 10), torch.int64, "record")
    planes = [a.out((B, H, W), torch.int32, "d2 %d" % i) if on else None for i, on in enumerate(maps)]
    for t in planes:                                            # -1, which these planes hold off the contour, is the arena's poison as
        if t is not None:                                       # an int32: they start from another pattern that no d2 of these sizes is
            t.fill_(UNWRITTEN)
    scratch = a.scratch(L.unet_surface_sums_scratch_bytes(B, H, W), "scratch")
    t2 = ref.t2_of(tolerances)
    q_num, q_den = ref.fraction_of(percentile)
    k = -1 if select is None else select
    _hip.run("unet_surface_sums", dev, a.ptr(p), CODE[dtypes[0]], k, a.ptr(g), CODE[dtypes[1]], k, B, H, W, connectivity, EDGE[edge], q_num, q_den,
             (C.c_int * 4)(*(t2 + [-7] * (4 - len(t2)))) if t2 else None, len(t2), a.ptr(record), a.ptr(planes[0]), a.ptr(planes[1]), a.ptr(scratch))
    a.verify(record)                                            # the record is written, every guard of every buffer is intact
    assert not any(bool((t == UNWRITTEN).any()) for t in planes if t is not None)
    assert torch.equal(p.cpu(), srcs[0]) and torch.equal(g.cpu(), srcs[1])
    return record.cpu().numpy(), [None if t is None else t.cpu().numpy() for t in planes]


def same_record(got, each, what):
    """got int64 [B,2,10] against boundary_ref.surface's records"""
    for b, s in enumerate(each):
        for d in range(2):
            r = s["record"][d]
            assert got[b, d, :9].tolist() == r[:9], (what, b, d, got[b, d, :9].tolist(), r[:9])
            total = float(got[b, d, 9:].copy().view(np.float64)[0])
            bound = (r[0] + 2) * 2.0 ** -53 * r[9]
            print("%s image %d dir %d: n %d sum %r reference %r bound %.3g" % (what, b, d, r[0], total, r[9], bound))
            assert abs(total - r[9]) <= bound and (r[9] != 0.0 or got[b, d, 9] == 0), (what, b, d, total, r[9])


def check(dev, pred, gt, what, dtypes=(U8, U8), maps=(True, True), contours=True, **rule):
    """The raw entry points twice on [B,H,W] (or [H,W]) numpy masks against the reference; returns the record."""
    if pred.ndim == 2:
        pred, gt = pred[None], gt[None]
    each = want(pred, gt, **rule)
    one, two = raw_sums(dev, pred, gt, dtypes, maps=maps, **rule), raw_sums(dev, pred, gt, dtypes, maps=maps, **rule)
    same_record(one[0], each, what)
    assert np.array_equal(one[0], two[0]), (what, "two runs")
    for d in range(2):
        assert (one[1][d] is None) == (not maps[d])
        if maps[d]:
            plane = np.stack([s["d2"][d] for s in each]).astype(np.int32)
            assert one[1][d].dtype == np.int32 and np.array_equal(one[1][d], plane) and np.array_equal(one[1][d], two[1][d]), (what, "d2", d)
    if contours:
        sel = {k: v for k, v in rule.items() if k in ("select", "connectivity", "edge")}
        for i, (m, t) in enumerate(zip((pred, gt), dtypes)):
            bits = np.stack([s["bits"] >> i & 1 for s in each]).astype(np.uint8)
            first = raw_contour(dev, m, t, **sel)
            assert np.array_equal(first, bits) and np.array_equal(raw_contour(dev, m, t, **sel), first), (what, "contour", i)
    return one[0]


CASES = {name: (p, g) for name, p, g in ref.named_cases()}


# ---- shapes, connectivities, edge conventions -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_named_cases(dev, name):
    """Every named case of boundary_ref (the sizes around the column pass's 4 segments and 64 columns and the row pass's 256 threads,
    the far corners, the strips, the equal distances, the empties) with both connectivities and both edge conventions."""
    p, g = CASES[name]
    for conn in (4, 8):
        for edge in ("background", "ignore"):
            rec = check(dev, p, g, (name, conn, edge), connectivity=conn, edge=edge)
            if name == "corners":
                assert rec[0, :, 1].tolist() == [69 ** 2 + 299 ** 2] * 2 and rec[0, :, 0].tolist() == [1, 1]
            if name == "equal":
                assert rec[0, 0, :5].tolist() == [2, 9, 9, 9, 19] and rec[0, 1, :5].tolist() == [1, 9, 9, 9, 0]
            if name.startswith("strip"):
                assert rec[0, 0, :5].tolist() == [4, 1449 ** 2, 1030 ** 2, 1449 ** 2, 17]
            if name == "empty pred":
                assert rec[0, 0].tolist() == [0] * 10 and rec[0, 1, 0] > 0 and rec[0, 1, 1:].tolist() == [0] * 9


def test_dtypes_and_select(dev):
    """All four mask dtypes on either side, and select on class maps of every dtype (the int32 one first)."""
    p, g = CASES["random 6x65"]
    for dp, dg in ((torch.int64, torch.float32), (torch.float32, torch.int32), (torch.int32, U8), (U8, torch.int64)):
        check(dev, p * 3, g * 200, ("dtypes", dp, dg), dtypes=(dp, dg), connectivity=8)
    rs = np.random.RandomState(5)
    cp = rs.randint(0, 4, (2, 7, 66)).astype(np.uint8)
    cg = np.where(rs.rand(2, 7, 66) < 0.2, rs.randint(0, 4, (2, 7, 66)), cp).astype(np.uint8)
    for dp, dg in ((torch.int32, torch.int32), (torch.int64, U8), (torch.float32, torch.int64), (U8, torch.float32)):
        for k in (0, 2, 3):
            check(dev, cp, cg, ("select", k, dp, dg), dtypes=(dp, dg), select=k, edge="ignore" if k == 3 else "background")
    rec = check(dev, cp, cg, "a class that is absent", dtypes=(torch.int32, torch.int32), select=9)
    assert not rec.any()


def test_percentiles_tolerances_and_null_maps(dev):
    """q = 0, 50, 95, 100 and 3/7; 0, 1 and 4 tolerances; either, both or no d2 plane asked for."""
    plans = [(0, (), (False, False)), (50, (1.0,), (True, False)), (95, (0, 1.5, 3, 40.25), (False, True)), (100, (2,), (True, True)),
             (Fraction(300, 7), (1030, 1448.9, 1449, 5), (False, False))]
    for name in ("strip 1", "strip 2", "random 6x65", "equal", "random 3x257", "square"):
        p, g = CASES[name]
        for pct, tol, maps in plans:
            rec = check(dev, p, g, (name, pct, tol), maps=maps, contours=False, percentile=pct, tolerances=tol)
            if name == "strip 2" and pct == 50:
                assert rec[0, 0, 2:5].tolist() == [25, 1030 ** 2, 1]               # lo and hi in different top digits
            if name == "strip 1" and pct == Fraction(300, 7):
                assert rec[0, 0, 2:9].tolist() == [25, 1030 ** 2, 2, 3, 3, 4, 2]    # j = floor(9 / 7) = 1, rem 2


def test_batch_of_empty_full_and_ordinary(dev):
    """Per-image state does not leak: B = 3 with an empty, a full and an ordinary image, in every order."""
    p, g = ref.batch_case()
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        for edge in ("background", "ignore"):
            rec = check(dev, p[list(order)], g[list(order)], ("batch", order, edge), tolerances=(1, 2), edge=edge)
            e, f = order.index(0), order.index(1)
            assert rec[e, 0].tolist() == [0] * 10 and rec[e, 1, 1:].tolist() == [0] * 9
            assert rec[f, 0, 0] == (42 if edge == "background" else 0)             # the frame of 9 x 14, or nothing


def test_cells(dev):
    p, g = ref.cells_pair()
    assert p.shape == (64, 80) and 100 < ref.contour(p).sum() < 2000
    rec = check(dev, p, g, "cells", tolerances=(1, 2, 3), percentile=95)
    assert rec[0, 0, 1] > 16 and rec[0, 0, 5] < rec[0, 0, 6] < rec[0, 0, 7] < rec[0, 0, 0]
    check(dev, p, g, "cells 8", connectivity=8, edge="ignore", contours=False)


# ---- the wrappers -----------------------------------------------------------------------------------------------------------

def close(got, ref_value, n):
    return got == ref_value or abs(got - ref_value) <= (n + 6) * 2.0 ** -53 * abs(ref_value)


def test_boundary_scores_against_the_reference(dev):
    """functions.boundary_scores on the named cases, singly and as batches of equal size: the distances that are square roots of
    integers and the ratios of integers are bit-equal, assd within the bound of the two fp64 sums and one division."""
    import functions
    n = 0
    for name, (p, g) in CASES.items():
        for spacing, tol in ((1.0, (1.0, 2.0)), (0.5, (0.5, 1.0, 1.25))):
            s = ref.surface(p, g, [Fraction(t) / Fraction(spacing) for t in tol], 95)
            w = ref.scores(s, spacing)
            got = functions.boundary_scores(torch.from_numpy(p).to(dev), torch.from_numpy(g).to(dev), tolerances=tol, spacing=spacing)
            assert isinstance(got, functions.BoundaryScores) and got.nsd.shape == (len(tol),)
            assert got.hausdorff == w["hausdorff"] and got.hd_percentile == w["hd_percentile"], (name, got, w)
            assert close(got.assd, w["assd"], w["n_pred"] + w["n_gt"]), (name, got.assd, w["assd"])
            for f in ("nsd", "precision", "recall", "boundary_f1"):
                assert np.array_equal(getattr(got, f), np.array(w[f]), equal_nan=True), (name, f)
            assert (got.n_pred, got.n_gt) == (w["n_pred"], w["n_gt"])
            n += 1
    assert n == 2 * len(CASES)
    p, g = ref.batch_case()
    tp, tg = torch.from_numpy(p).to(dev), torch.from_numpy(g).to(dev)
    got = functions.boundary_scores(tp.int(), tg.float(), tolerances=(1,), percentile=50, connectivity=8)
    for b in range(3):
        w = ref.scores(ref.surface(p[b], g[b], (1,), 50, None, 8))
        assert got.hausdorff[b] == w["hausdorff"] and got.hd_percentile[b] == w["hd_percentile"] and close(got.assd[b], w["assd"], 300)
        assert np.array_equal(got.nsd[b], w["nsd"]) and np.array_equal(got.precision[b], w["precision"], equal_nan=True)


def test_surface_sums_and_mask_boundary_wrappers(dev):
    import functions
    p, g = ref.cells_pair()
    both = np.stack([p, g]), np.stack([g, p])
    tp, tg = torch.from_numpy(both[0]).to(dev), torch.from_numpy(both[1]).to(dev)
    each = want(both[0], both[1], (1.0, 2.5), 95)
    s = functions.surface_sums(tp, tg, tolerances=(1.0, 2.5), return_maps=True)
    assert isinstance(s, functions.SurfaceSums) and s.record.is_cuda and s.d2_pred.is_cuda and s.d2_gt.is_cuda
    assert (s.t2, s.q_num, s.q_den) == ((1, 6), 19, 20) and s.record.shape == (2, 2, 10) and s.d2_pred.dtype == torch.int32
    same_record(s.record.cpu().numpy(), each, "surface_sums")
    assert np.array_equal(s.d2_pred.cpu().numpy(), np.stack([e["d2"][0] for e in each])) and np.array_equal(s.d2_gt.cpu().numpy(), np.stack([e["d2"][1] for e in each]))
    assert torch.equal(s.record[0, 0], s.record[1, 1]) and torch.equal(s.record[0, 1], s.record[1, 0])      # the masks swapped
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        t = functions.surface_sums(tp.bool(), tg.long(), tolerances=(1.0, 2.5))
    side.synchronize()
    assert torch.equal(s.record, t.record) and t.d2_pred is None and t.d2_gt is None
    one = functions.surface_sums(tp[0], tg[0], tolerances=(1.0, 2.5), return_maps=True)
    assert one.record.shape == (2, 10) and torch.equal(one.record, s.record[0]) and torch.equal(one.d2_gt, s.d2_gt[0])
    for conn in (4, 8):
        for edge in ("background", "ignore"):
            c = functions.mask_boundary(tp, connectivity=conn, edge=edge)
            assert c.dtype == U8 and c.is_cuda and np.array_equal(c.cpu().numpy(), np.stack([ref.contour(m != 0, conn, edge) for m in both[0]]))
    lab = torch.from_numpy(p * 2 + g).to(dev)
    assert np.array_equal(functions.mask_boundary(lab[:, :33].long(), select=3).cpu().numpy(), ref.contour((p * 2 + g)[:, :33] == 3))
    assert functions.mask_boundary(lab).shape == (64, 80)
    with pytest.raises(NotImplementedError):
        functions.surface_sums(tp, tg.cpu())


# ---- what the entries refuse ------------------------------------------------------------------------------------------------

def test_a_rejected_call_writes_nothing(dev, hip):
    L = hip.lib()
    a = guarded.Arena(dev)
    B, H, W = 2, 9, 11
    m = np.ones((B, H, W), np.uint8)
    pm, gm = a.inp(torch.from_numpy(m), "pred"), a.inp(torch.from_numpy(m), "gt")
    record, d0, d1 = a.out((B, 2, 10), torch.int64, "record"), a.out((B, H, W), torch.int32, "d2 0"), a.out((B, H, W), torch.int32, "d2 1")
    scratch = a.scratch(L.unet_surface_sums_scratch_bytes(B, H, W), "scratch")
    out = a.out((B, H, W), U8, "contour")
    st = hip.stream(dev)
    p = a.ptr
    t2 = (C.c_int * 4)(1, 4, 9, 16)
    good = dict(p=p(pm), pd=3, ps=-1, g=p(gm), gd=3, gs=-1, B=B, H=H, W=W, conn=4, edge=1, qn=19, qd=20, t2=t2, nt=4, rec=p(record), d0=p(d0),
                d1=p(d1), scratch=p(scratch))
    for bad in ({"p": None}, {"g": None}, {"rec": None}, {"scratch": None}, {"pd": 4}, {"pd": -1}, {"gd": 7}, {"ps": -2}, {"gs": -5}, {"B": 0}, {"H": 0},
                {"W": -1}, {"H": 32768, "W": 1}, {"H": 1, "W": 32768}, {"B": 65536}, {"conn": 6}, {"conn": 0}, {"edge": 2}, {"edge": -1}, {"qn": -1},
                {"qn": 21}, {"qd": 0}, {"qd": 1 << 20, "qn": 5}, {"nt": 5}, {"nt": -1}, {"t2": None}, {"t2": (C.c_int * 4)(1, -4, 9, 16)}):
        kw = dict(good, **bad)
        rc = L.unet_surface_sums(kw["p"], kw["pd"], kw["ps"], kw["g"], kw["gd"], kw["gs"], kw["B"], kw["H"], kw["W"], kw["conn"], kw["edge"], kw["qn"],
                                 kw["qd"], kw["t2"], kw["nt"], kw["rec"], kw["d0"], kw["d1"], kw["scratch"], st)
        rejected(hip, rc, a, record, d0, d1, scratch)
        assert b"unet_surface_sums" in L.unet_last_error(), bad
    good = dict(m=p(pm), d=3, s=-1, B=B, H=H, W=W, conn=8, edge=0, out=p(out))
    for bad in ({"m": None}, {"out": None}, {"d": 4}, {"d": -1}, {"s": -2}, {"B": 0}, {"H": -3}, {"W": 0}, {"H": 40000}, {"W": 32768}, {"B": 70000},
                {"conn": 5}, {"edge": 2}):
        kw = dict(good, **bad)
        rc = L.unet_mask_boundary(kw["m"], kw["d"], kw["s"], kw["B"], kw["H"], kw["W"], kw["conn"], kw["edge"], kw["out"], st)
        rejected(hip, rc, a, out)
        assert b"unet_mask_boundary" in L.unet_last_error(), bad


# ---- the existing op that shares the column pass ----------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(1, 65), (65, 66), (129, 127)])
def test_distance_map_is_unchanged(dev, H, W):
    """functions.distance_map, whose column pass is now the shared one, bit-equal to shape_ref on three of its shapes."""
    import functions
    for name, m in shape_ref.size_cases(H, W):
        for edge in shape_ref.EDGES:
            expect = np.stack([shape_ref.distance2(x, edge) for x in m]).astype(np.int32)
            for dtype in (U8, torch.float32, torch.int32, torch.int64):
                got = functions.distance_map(torch.from_numpy(m).to(dev).to(dtype), edge=edge)
                assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), expect), (name, edge, dtype)
