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
