"""Nearest-cell growth, the foreground pair table and the Rand / information scores without a GPU: the C ABI and the Python
surface are there, the two-pass restatement tests/rand_ref.grow (what the GPU tests compare the device with) equals the all-pairs
definition, the scores give the answers worked by hand below, and the host half functions.rand_from_pairs agrees with the
restatement.  The properties the GPU tests assert of the seeded cell images are first shown to hold of the restatement here."""
import math
import os
import re

import numpy as np
import pytest
import torch

import instances_ref
import prepare_ref
import rand_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_grow_labels_scratch_bytes", "unet_grow_labels", "unet_partition_pairs_scratch_bytes", "unet_partition_pairs")
SMALL = [(1, 1), (1, 2), (2, 1), (1, 40), (17, 5), (33, 31)]


def test_abi_declares_and_exports_the_new_entry_points():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(L, name), name
    assert L.unet_abi_version() == 4
    assert L.unet_grow_labels_scratch_bytes(2, 33, 31) >= 2 * 33 * 31 * 8
    assert L.unet_grow_labels_scratch_bytes(2, 0, 31) == 0
    assert L.unet_partition_pairs_scratch_bytes(2, 1024) >= 1024 * 12
    assert L.unet_partition_pairs_scratch_bytes(2, 0) == 0


@pytest.mark.parametrize("H,W", SMALL)
def test_two_pass_growth_equals_the_all_pairs_definition(H, W):
    n = 0
    for name, maps in ref.id_cases(H, W, 0):
        for d in ref.DISTANCES:
            m = ref.dist2(d)
            for img in maps:
                want = ref.grow_brute(img, m)
                assert np.array_equal(ref.grow(img, m), want), (name, d)
                n += int((want != img).sum())
    if H * W > 2:
        assert n > 0                                        # something grew


def test_every_tie_order_against_the_definition():
    """All 24 orders of four ids on the corners of a square: the centre takes the smallest, whichever corner holds it."""
    t = ref.tie_maps(9, 12)
    assert len(t) == 24 and len({tuple(m[m > 0]) for m in t}) == 24
    for m in t:
        got = ref.grow(m)
        assert np.array_equal(got, ref.grow_brute(m))
        assert got[1, 1] == 2 and got[0, 1] == min(m[0, 0], m[0, 2]) and got[1, 0] == min(m[0, 0], m[2, 0])
        for lim in (0, 1, 2, 3):
            assert np.array_equal(ref.grow(m, lim), ref.grow_brute(m, lim))
        assert ref.grow(m, 1)[1, 1] == 0 and ref.grow(m, 2)[1, 1] == 2          # d^2 = 2: at the limit, and one short of it


def test_the_limit_is_inclusive():
    m = np.zeros((21, 23), np.int32)
    m[10, 11] = 6
    yy, xx = np.mgrid[0:21, 0:23]
    d2 = (yy - 10) ** 2 + (xx - 11) ** 2
    for d in ref.DISTANCES[1:]:
        lim = ref.dist2(d)
        assert np.array_equal(ref.grow(m, lim), np.where(d2 <= lim, 6, 0))
    assert [ref.dist2(d) for d in ref.DISTANCES] == [None, 0, 1, 2, 4, 16, 53]
    g = ref.grow(m, 53)
    assert g[10 + 2, 11 + 7] == 6 and g[10 + 3, 11 + 7] == 0 and ref.grow(m, 4)[10, 13] == 6 and ref.grow(m, 4)[11, 13] == 0


def one(gt, pred, alpha=0.5):
    r = ref.scores(np.array(pred)[None, None], np.array(gt)[None, None], alpha)
    return {k: (v[0] if np.ndim(v) else v) for k, v in r.items()}


def test_hand_worked_scores():
    r = one([1, 1, 2, 2], [1, 1, 1, 1])
    assert [r[k] for k in ref.INTS] == [4, 8, 16, 8, 0]
    assert r["rand_merge"] == 0.5 and r["rand_split"] == 1.0 and r["rand_error"] == 1 / 3 and r["v_rand"] == 2 / 3
    assert np.isnan(r["info_split"]) and r["info_merge"] == 0.0 and r["v_info"] == 0.0
    assert r["voi_merge"] == math.log(2) and r["voi_split"] == 0.0
    a = one([1, 1, 2, 2], [1, 2, 3, 4])
    assert a["rand_split"] == 0.5 and a["rand_merge"] == 1.0 and [a[k] for k in ref.INTS] == [4, 4, 4, 8, 0]
    assert a["voi_split"] == math.log(2) and a["voi_merge"] == 0.0 and a["info_split"] == 0.5 and a["info_merge"] == 1.0
    z = one([1, 1, 2, 2], [0, 0, 0, 0])                     # predicted background: four singletons, the same numbers
    assert [z[k] for k in ref.INTS] == [4, 4, 4, 8, 4]
    assert all(z[k] == a[k] for k in ref.SCORES)
    e = one([1, 1, 2, 2, 0, 0], [5, 5, 9, 9, 9, 0])         # equal on gt foreground; gt background is not looked at
    assert e["rand_error"] == 0.0 and e["v_rand"] == 1.0 and e["v_info"] == 1.0 and e["voi_split"] == 0.0 and e["voi_merge"] == 0.0
    n = one([0, 0, 0, 0], [1, 2, 0, 0])
    assert all(np.isnan(n[k]) for k in ref.SCORES) and [n[k] for k in ref.INTS] == [0, 0, 0, 0, 0]
    # alpha weighs the two sides: alpha = 1 is rand_merge, alpha = 0 rand_split
    assert one([1, 1, 2, 2], [1, 1, 1, 1], 1.0)["v_rand"] == 0.5 and one([1, 1, 2, 2], [1, 1, 1, 1], 0.0)["v_rand"] == 1.0
    b = ref.scores(np.array([[[1, 1, 2, 2]], [[0, 0, 0, 0]], [[1, 1, 2, 2]]]), np.array([[[1, 1, 2, 2]], [[0, 0, 0, 0]], [[1, 1, 1, 1]]]))
    assert np.isnan(b["rand_error"][1]) and b["rand_error_mean"] == b["rand_error"][[0, 2]].mean() and b["v_info_mean"] == 0.5


def test_rand_from_pairs_is_the_restatement():
    import functions
    assert functions.RandScores._fields == ref.SCORES + ("rand_error_mean", "v_info_mean") + ref.INTS
    gt = np.array([[[1, 1, 2, 2, 0, 0]], [[1, 1, 2, 2, 0, 0]], [[1, 1, 2, 2, 0, 0]], [[1, 1, 2, 2, 3, 3]], [[0, 0, 0, 0, 0, 0]]])
    pred = np.array([[[1, 1, 1, 1, 1, 1]], [[1, 2, 3, 4, 4, 4]], [[0, 0, 0, 0, 7, 7]], [[6, 6, 5, 5, 4, 4]], [[1, 2, 3, 0, 0, 0]]])
    for alpha in (0.5, 0.25, 1.0):
        got = functions.rand_from_pairs(*ref.pairs(pred, gt), len(gt), alpha)
        ref.check_scores(got, ref.scores(pred, gt, alpha))
    r = functions.rand_from_pairs(*ref.pairs(pred, gt), len(gt))
    assert r.rand_error[0] == 1 / 3 and np.isnan(r.info_split[0]) and r.voi_merge[0] == math.log(2)
    assert np.isnan(r.rand_error[4]) and np.isnan(r.v_info[4]) and r.N.tolist() == [4, 4, 4, 6, 0] and r.c.tolist() == [0, 0, 4, 0, 0]
    assert r.rand_error[3] == 0.0 and r.v_info[3] == 1.0
    # the order of the table does not matter, and an image without an entry is all nan
    b, g, p, n = ref.pairs(pred, gt)
    o = np.random.RandomState(0).permutation(len(b))
    ref.check_scores(functions.rand_from_pairs(b[o], g[o], p[o], n[o], len(gt)), ref.scores(pred, gt))
    # random tables: many ids, large counts (squares near 2^60 in the sums)
    rs = np.random.RandomState(1)
    for trial in range(6):
        B, ng, npred = 3, int(rs.randint(2, 60)), int(rs.randint(2, 80))
        tabs = [{(int(g_), int(p_)): int(rs.randint(1, 1 << (8 + 3 * trial))) for g_, p_ in zip(rs.randint(1, ng + 1, 200), rs.randint(0, npred + 1, 200))}
                for _ in range(B)]
        per = [ref.scores_of_table(t, 0.5) for t in tabs]
        assert all(r_["H_pred"] > 0.1 and r_["H_gt"] > 0.1 for r_ in per)
        flat = [(i, g_, p_, n_) for i, t in enumerate(tabs) for (g_, p_), n_ in t.items()]
        got = functions.rand_from_pairs(*(np.array(c) for c in zip(*flat)), B)
        want = {k: np.array([r_[k] for r_ in per]) for k in ref.SCORES + ref.INTS}
        want.update({k + "_mean": want[k].mean() for k in ("rand_error", "v_info")})
        ref.check_scores(got, want)


def test_the_seeded_score_cases_are_well_conditioned():
    """H_pred, H_gt > 0.1 on every image the GPU test compares information scores on to 1e-12 (no quotient amplifies the last
    roundings), and the scores are no corner case: strictly inside (0, 1)."""
    for name, pred, gt in ref.seeded_pairs() + [("speckle",) + tuple(a[[0, 2]] for a in ref.speckle_pairs())]:
        r = ref.scores(pred, gt)
        assert (r["H_pred"] > 0.1).all() and (r["H_gt"] > 0.1).all(), name
        assert ((r["rand_error"] > 0) & (r["rand_error"] < 1) & (r["v_info"] > 0) & (r["v_info"] < 1)).all(), name
    b, g, p, n = ref.pairs(*ref.speckle_pairs())
    assert len(b) > 5000 and (p == 0).any() and not (b == 1).any() and len(np.unique(g)) > 250


def test_growth_hands_the_carved_rim_back():
    """The property the GPU test asserts of the device, shown of the restatement first: on these cell images, growing the
    instances of the carved target by the carve's reach does not lower SEG, and unlimited growth does not raise the Rand error.
    The second holds widely (the Rand scores look at ground-truth foreground only).  The first is a property of the image, not of
    the growth: a cell also grows 4 px into true background, and SEG rises only where the rims carved between touching cells
    cost more than that.  It holds of the seeds of E2E; of cells_case(1, 9, 128, 128), whose 9 cells mostly lie apart, SEG goes
    0.6004 -> 0.5931 while the Rand error goes 0.2114 -> 0.0283 (shown below, so the choice of seeds hides nothing)."""
    for seed, n, H, W in ref.E2E:
        gt = instances_ref.cells_case(seed, n, H, W)[0][None]
        pred = ref.carved_prediction(gt)
        grown = ref.grow_batch(pred, (16, None))
        s0, s1 = instances_ref.seg(gt, pred)["seg"], instances_ref.seg(gt, grown[16])["seg"]
        e0, e1 = ref.scores(pred, gt)["rand_error"][0], ref.scores(grown[None], gt)["rand_error"][0]
        print("%d x %d, seed %d: SEG %.4f -> %.4f, Rand error %.4f -> %.4f" % (H, W, seed, s0, s1, e0, e1))
        assert s1 >= s0 and e1 <= e0 and e0 > 0
    gt = instances_ref.cells_case(1, 9, 128, 128)[0][None]
    pred = ref.carved_prediction(gt)
    grown = ref.grow_batch(pred, (16, None))
    assert instances_ref.seg(gt, grown[16])["seg"] < instances_ref.seg(gt, pred)["seg"]
    assert ref.scores(grown[None], gt)["rand_error"][0] < ref.scores(pred, gt)["rand_error"][0]


def test_host_errors():
    import functions
    t = torch.ones(4, 4, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="device"):
        functions.grow_cells(t)
    with pytest.raises(NotImplementedError, match="device"):
        functions.pair_table(t, t)
    with pytest.raises(NotImplementedError, match="device"):
        functions.rand_scores(t, t, grow=True)
    for bad in (torch.ones(4, dtype=torch.int32), torch.ones(1, 1, 4, 4, dtype=torch.int32), t.float(), t.bool(), t[:0]):
        with pytest.raises(ValueError):
            functions.grow_cells(bad)
        with pytest.raises(ValueError):
            functions.pair_table(bad, bad)
        with pytest.raises(ValueError):
            functions.rand_scores(bad, bad)
    with pytest.raises(ValueError, match="equal shape"):
        functions.pair_table(t, t[:2])
    with pytest.raises(ValueError, match="equal shape"):
        functions.rand_scores(t[None], t)
