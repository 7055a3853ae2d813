"""The oracle of the border weight map: tests/weighted_map_ref.py (a plain numpy/scipy restatement by the reference's own
per-component method) reproduces tests/golden/weighted_map_golden.npz, made by running the reference's weighted_map
(functions.py:7-78).  CPU only; the GPU tests compare the device op with this same restatement."""
import numpy as np
import pytest
from scipy import ndimage

import weighted_map_ref as ref
from weighted_map_ref import golden_cases


def test_restatement_reproduces_reference_golden(golden_dir):
    names = []
    for name, lab, w_ref in golden_cases(golden_dir):
        w, n = ref.weighted_map_batch(lab)
        assert w.dtype == np.float32 and w.shape == w_ref.shape
        assert np.all(np.abs(w - w_ref) <= 1e-6 * np.maximum(1.0, np.abs(w_ref))), name
        assert np.array_equal(w[lab != 0], np.ones(int((lab != 0).sum()), np.float32)), name
        names.append(name)
    assert len(names) == 9


def test_golden_covers_the_contract(golden_dir):
    """The cases the device op is held to: integer (truncated) and float class terms, one component (d2 = 0), 4-connectivity
    splitting a diagonal, a hole, objects on the edge, objects farther apart than the 73 px reach, speckle, a batch."""
    cases = {name: (lab, w) for name, lab, w in golden_cases(golden_dir)}
    lab, w = cases["cells_i64"]
    for b in range(2):
        n1 = int(lab[b].sum()); n0 = lab[b].size - n1
        assert n1 < n0 and w[b][lab[b] == 0].min() == 0.0          # background class term trunc(n1/n0) = 0
    lab, w = cases["cells_f32"]
    n1 = int(lab[0].sum())
    assert abs(w[0][lab[0] == 0].min() - np.float32(n1) / np.float32(lab[0].size - n1)) < 1e-6
    assert ndimage.label(cases["single"][0][0], ref.CROSS)[1] == 1
    assert ndimage.label(cases["diagonal"][0][0], ref.CROSS)[1] == 48 + 40 - 3
    assert ndimage.label(cases["speckle96"][0][0], ref.CROSS)[1] > 500
    assert cases["batch3"][0].shape[0] == 3
    lab, w = cases["far"]
    d1, d2, n = ref.distances(lab[0])
    assert n == 2 and np.isinf(d2[lab[0] == 0]).any()              # pixels with only one component within reach


def test_restatement_one_class_raises():
    with pytest.raises(IndexError):
        ref.weighted_map(np.zeros((5, 7), np.int64))
    with pytest.raises(IndexError):
        ref.weighted_map(np.ones((4, 4), np.float32))


# ---- the label batches of tests/test_weighted_map_ops_gpu.py are well-posed -------------------------------------------------

def test_reaches_are_the_stated_numbers():
    assert [ref.reach_of(s) for _, s in ref.PARAMS] == ref.REACHES == [21, 73, 204, 1020]
    assert ref.reach_of(25) == ref.REACH and ref.reach_of(6000) > 1024 >= ref.reach_of(5000)


@pytest.mark.parametrize("dtype", [np.int64, np.float32])
def test_threshold_label_batches_have_both_classes(dtype):
    assert ref.THRESHOLD_SHAPES == [(1, 1, 2), (2, 33, 65), (1, 5, 257), (3, 64, 32), (2, 31, 256)]
    for B, H, W in ref.THRESHOLD_SHAPES:
        lab = ref.threshold_labels(B, H, W, dtype)
        assert lab.shape == (B, H, W) and lab.dtype == dtype and set(np.unique(lab)) == {0, 1}
        for b in range(B):
            assert lab[b].any() and not lab[b].all()
        ref.weighted_map_batch(lab)                                 # no one-class image


def test_parameter_label_batches_are_what_they_claim():
    shapes = {}
    for name in ref.PARAM_CASES:
        lab = ref.param_labels(name, np.int64)
        shapes[name] = lab.shape
        assert max(lab.shape[1:]) <= ref.REACH + 1                  # every grown box is the whole image: exact at any reach
        for b in range(lab.shape[0]):
            assert lab[b].any() and not lab[b].all()
        assert np.array_equal(ref.param_labels(name, np.float32), lab.astype(np.float32))
    assert shapes == {"blobs+far": (2, 40, 70), "speckle+single": (2, 40, 70), "tall-single": (1, 74, 9), "tall-speckle": (1, 74, 9)}
    far = ref.param_labels("blobs+far", np.int64)[1]
    lab, n = ref.components(far)
    assert n == 2
    apart = ndimage.distance_transform_edt(lab != 1)[lab == 2].min()
    assert apart > ref.reach_of(2) and apart <= ref.reach_of(25)    # out of reach at sig2 = 2, within it at 25
    d1, d2, _ = ref.distances(far)
    assert ((far == 0) & (d1 > ref.reach_of(2))).any()              # background that must be exactly w_c at sig2 = 2
    assert ref.components(ref.param_labels("blobs+far", np.int64)[0])[1] > 2
    assert ref.components(ref.param_labels("speckle+single", np.int64)[0])[1] > 100
    assert ref.components(ref.param_labels("speckle+single", np.int64)[1])[1] == 1
    assert ref.components(ref.param_labels("tall-single", np.int64)[0])[1] == 1
    assert ref.components(ref.param_labels("tall-speckle", np.int64)[0])[1] > 20
    one = ref.param_labels("tall-single", np.int64)[0]
    assert ((one == 0) & (ref.distances(one)[0] > ref.reach_of(2))).any()


def test_border_term_is_visible_beyond_a_shorter_reach():
    """With a class term of 0 the border term is at least 2^-100 at pixels whose d1 + d2 exceeds ceil(sqrt(2 sig2 * 52)), the
    reach of half the exponent: there a reach cut short shows as an exact 0."""
    for name, (w0, sig2) in (("tall-single", (20, 2)), ("blobs+far", (20, 2))):
        assert ref.param_dtype(name, w0, sig2) == np.int64
        lab = ref.param_labels(name, np.int64)
        w_ref, _ = ref.weighted_map_batch(lab, w0, sig2)
        seen = ref.visible_border(lab, w_ref)
        short = int(np.ceil(np.sqrt(2.0 * sig2 * 52.0)))
        beyond = np.zeros(lab.shape, bool)
        for b in range(lab.shape[0]):
            d1, d2, n = ref.distances(lab[b])
            s = d1 + (d2 if n > 1 else 0)
            beyond[b] = seen[b] & (s > short) & (s <= ref.reach_of(sig2))
        assert beyond.any(), name
    assert not ref.visible_border(ref.param_labels("blobs+far", np.float32), w_ref).any()
