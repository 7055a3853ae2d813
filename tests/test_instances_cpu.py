"""Instances and the SEG measure without a GPU: the C ABI and the Python surface are there, and the numpy/scipy restatement
tests/instances_ref.py (what the GPU tests compare the device with) gives the answers worked by hand below."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import instances_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("unet_label_components_scratch_bytes", "unet_label_components", "unet_instance_overlap_scratch_bytes",
       "unet_instance_overlap")


def test_abi_declares_and_exports_the_new_entry_points():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(L, name), name
    assert L.unet_abi_version() == 4
    # the size exports answer without a device
    assert L.unet_label_components_scratch_bytes(2, 33, 31) >= 2 * 33 * 31 * 4
    assert L.unet_label_components_scratch_bytes(0, 33, 31) == 0
    assert L.unet_instance_overlap_scratch_bytes(2, 10, 10, 1024) >= 1024 * 12
    assert L.unet_instance_overlap_scratch_bytes(2, 10, 10, 0) == 0


def test_python_surface():
    import functions
    import tester
    with pytest.raises(NotImplementedError, match="device"):
        functions.label_cells(torch.ones(4, 4, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="device"):
        functions.seg_measure(torch.ones(4, 4, dtype=torch.int32), torch.ones(4, 4, dtype=torch.int32))
    p = inspect.signature(tester.segment).parameters["return_instances"]
    assert p.default is False
    assert functions.SegMeasure._fields == ("seg", "jaccard_sum", "n_gt", "n_matched", "n_pred", "per_image", "jaccard")


def test_two_squares_against_one_shifted_prediction():
    """GT 1 = 4 x 4 at rows 1-4, columns 1-4, GT 2 = 4 x 4 at rows 6-9, columns 6-9; the one prediction is GT 1 moved one column
    right: it shares 4 x 3 = 12 of GT 1's 16 pixels (24 > 16: matched), J = 12 / (16 + 16 - 12) = 0.6; GT 2 has nothing: 0."""
    gt = np.zeros((12, 12), np.int32); pred = np.zeros((12, 12), np.int32)
    gt[1:5, 1:5] = 1; gt[6:10, 6:10] = 2
    pred[1:5, 2:6] = 1
    area_gt, area_pred, match, inter, bad, npairs = ref.overlaps(gt, pred)
    assert area_gt.tolist() == [144 - 32, 16, 16] and area_pred.tolist() == [144 - 16, 16]
    assert match.tolist() == [0, 1, 0] and inter.tolist() == [0, 12, 0] and bad == 0 and npairs == 1
    r = ref.seg(gt[None], pred[None])
    assert r["jaccard"][0].tolist() == [0.6, 0.0] and r["seg"] == 0.3 and r["per_image"].tolist() == [0.3]
    assert (r["n_gt"], r["n_matched"], r["n_pred"], r["jaccard_sum"]) == (2, 1, 1, 0.6)


def test_exactly_half_is_not_a_match():
    gt = np.zeros((6, 6), np.int32); pred = np.zeros((6, 6), np.int32)
    gt[1:5, 1:5] = 1
    pred[1:5, 1:3] = 1                                  # 8 of 16 pixels: 2 * 8 > 16 is false
    _, _, match, inter, _, _ = ref.overlaps(gt, pred)
    assert match.tolist() == [0, 0] and inter.tolist() == [0, 0]
    assert ref.seg(gt[None], pred[None])["seg"] == 0.0
    pred[1, 3] = 1                                      # 9 of 16: matched, J = 9 / (16 + 9 - 9)
    _, _, match, inter, _, _ = ref.overlaps(gt, pred)
    assert match.tolist() == [0, 1] and inter.tolist() == [0, 9]
    assert ref.seg(gt[None], pred[None])["seg"] == 9 / 16


def test_absent_and_non_consecutive_ground_truth_ids():
    """ids 5 and 9 only: 1-4 and 6-8 have no pixel and are no cells.  5 = 2 x 3 covered fully by a 2 x 4 prediction:
    J = 6 / 8; 9 = 1 x 2 with no prediction."""
    gt = np.zeros((5, 8), np.int32); pred = np.zeros((5, 8), np.int32)
    gt[0:2, 0:3] = 5; gt[4, 6:8] = 9
    pred[0:2, 0:4] = 3
    area_gt, area_pred, match, inter, bad, npairs = ref.overlaps(gt, pred, ng_max=12, np_max=4)
    assert len(area_gt) == 13 and len(area_pred) == 5 and np.flatnonzero(area_gt[1:]).tolist() == [4, 8]
    assert match[5] == 3 and inter[5] == 6 and match[9] == 0 and bad == 0 and npairs == 1
    r = ref.seg(gt[None], pred[None])
    assert r["jaccard"][0].tolist() == [0.75, 0.0] and r["n_gt"] == 2 and r["seg"] == 0.375


def test_a_prediction_across_two_cells_matches_only_the_one_it_covers_by_more_than_half():
    """GT 1 = columns 0-3, GT 2 = columns 4-7 of one row; the prediction, columns 1-4, holds 3 of GT 1 (6 > 4) and 1 of GT 2."""
    gt = np.array([[1, 1, 1, 1, 2, 2, 2, 2]], np.int32)
    pred = np.array([[0, 7, 7, 7, 7, 0, 0, 0]], np.int32)
    _, _, match, inter, _, npairs = ref.overlaps(gt, pred)
    assert match.tolist() == [0, 7, 0] and inter.tolist() == [0, 3, 0] and npairs == 2
    assert ref.seg(gt[None], pred[None])["jaccard"][0].tolist() == [3 / 5, 0.0]


def test_ids_out_of_range_are_counted_apart():
    gt = np.array([[1, 1, 4, -1, 0, 1]], np.int32)
    pred = np.array([[1, 1, 1, 1, 9, 1]], np.int32)
    area_gt, area_pred, match, inter, bad, _ = ref.overlaps(gt, pred, ng_max=3, np_max=2)
    assert bad == 3 and area_gt.tolist() == [0, 3, 0, 0] and area_pred.tolist() == [0, 3, 0]
    assert match.tolist() == [0, 1, 0, 0] and inter.tolist() == [0, 3, 0, 0]


def test_empty_ground_truth_is_nan():
    z = np.zeros((1, 4, 4), np.int32)
    r = ref.seg(z, np.ones((1, 4, 4), np.int32))
    assert np.isnan(r["seg"]) and np.isnan(r["per_image"][0]) and r["n_gt"] == 0 and r["n_pred"] == 1 and len(r["jaccard"][0]) == 0


def test_seg_from_counts_is_the_restatement():
    """The host half of functions.seg_measure on the restatement's integers gives the restatement's floats, bit for bit."""
    import functions
    gts, preds = zip(*(ref.cells_case(s, n, 96, 120, stride=st) for s, n, st in ((1, 9, 1), (2, 20, 3))))
    ng, npm = max(int(g.max()) for g in gts), max(int(p.max()) for p in preds)
    ints = [ref.overlaps(g, p, ng, npm)[:4] for g, p in zip(gts, preds)]
    got = functions.seg_from_counts(*(np.stack([i[k] for i in ints]) for k in range(4)))
    want = ref.seg(gts, preds)
    assert got.seg == want["seg"] and 0 < got.seg < 1 and np.array_equal(got.per_image, want["per_image"])
    assert all(np.array_equal(a, b) for a, b in zip(got.jaccard, want["jaccard"]))
    assert (got.jaccard_sum, got.n_gt, got.n_matched, got.n_pred) == tuple(want[k] for k in ("jaccard_sum", "n_gt", "n_matched", "n_pred"))
    empty = functions.seg_from_counts(np.array([[16, 0]]), np.array([[0, 16]]), np.zeros((1, 2)), np.zeros((1, 2)))
    assert np.isnan(empty.seg) and empty.n_gt == 0 and empty.n_pred == 1


def test_the_seeded_cases_exercise_both_branches():
    """The id maps of the GPU tests: each has matched cells, the two larger ones unmatched cells too."""
    for seed, n, H, W in ((1, 9, 128, 128), (2, 37, 256, 256), (3, 99, 388, 388)):
        gt, pred = ref.cells_case(seed, n, H, W)
        r = ref.seg(gt[None], pred[None])
        assert r["n_matched"] >= 1 and 0 < r["seg"] < 1
        if n > 9:
            assert r["n_matched"] < r["n_gt"]


def test_mask_generators():
    lab, n = ref.label(ref.serpentine(70, 45))
    assert n == 1 and lab.max() == 1
    lab, n = ref.label(ref.comb(40, 41))
    assert n == 1 + 10 and lab[0, 0] == 1 and lab[0, 4] == 1 and lab[0, 40] == 1 and [lab[0, x] for x in (2, 6, 38)] == [2, 3, 11]
