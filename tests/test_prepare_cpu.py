"""The restatement tests/prepare_ref.py against the reference's own outputs (tests/golden/prepare_golden.npz, made by
make_golden_prepare.py from the reference's preprocess_gt and ImageDataset statements) and against hand-worked answers; and the
host half of the package's crop distribution (data.crop_probabilities, data.draw_crop) against the same fixture.  No GPU."""
import os

import numpy as np
import pytest

import prepare_ref as ref


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "prepare_golden.npz"))


def test_both_restatements_equal_the_reference(golden):
    for name in golden["names"]:
        ids = golden[name + "_ids"]
        for form in (ref.carve_literal, ref.carve_fast):
            gt, edges, binary, bad = form(ids)
            assert bad == 0
            assert np.array_equal(gt, golden[name + "_gt"]), (name, form.__name__)
            assert np.array_equal(edges, golden[name + "_mask_global"]), (name, form.__name__)
            assert np.array_equal(binary, golden[name + "_bin"]), (name, form.__name__)
    assert golden["discs_hi_mask_global"].max() >= 510 and golden["speckle_mask_global"].max() >= 40 * 255


def test_restatements_agree_at_other_reaches():
    for kind in ref.KINDS:
        ids = ref.ids_case(kind, 3, 33, 31)
        for reach in (0, 1, 8):
            a, b = ref.carve_literal(ids, reach), ref.carve_fast(ids, reach)
            assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])), (kind, reach)
            if reach == 0:
                assert np.array_equal(a[0], ids) and not a[1].any()


def two_cells(d):
    """two 3 x 3 cells in a 12 x 24 image, rows 4..6: cell 1 in columns 2..4, cell 2 in columns 4 + d .. 6 + d, so the facing
    edge columns are d apart and d - 1 background columns lie between them"""
    ids = np.zeros((12, 24), np.int64)
    ids[4:7, 2:5] = 1
    ids[4:7, 4 + d:7 + d] = 2
    return ids


def test_two_cells_at_hand_worked_distances():
    """The 9 x 9 dilation of cell 1 covers columns 0..8 (clipped at the image edge), that of cell 2 columns d .. 10 + d, rows
    0..10 both.  Facing edges 9 apart (8 background columns between): the dilations do not reach each other.  8 and 7 apart:
    the two rings share 1 and 2 columns of background, where mask_global is 510; no CELL pixel is within 4 of the other cell, so
    gt is still the input.  Within the reach (4 and 3 apart) a band of each cell lies in the other's dilation and is carved:
    1 - 255 and 2 - 255 clip to 0."""
    for form in (ref.carve_literal, ref.carve_fast):
        for d in (9, 8, 7):
            ids = two_cells(d)
            gt, edges, binary, _ = form(ids)
            assert np.array_equal(gt, ids) and np.array_equal(binary, 255 * (ids > 0))
            ring = np.zeros_like(ids)
            ring[0:11, 0:9] = 255
            ring[0:11, d:11 + d] += 255
            ring[ids > 0] = 0
            assert np.array_equal(edges, ring)
            assert (edges == 510).sum() == 11 * (9 - d) and (edges[5, d:9] == 510).all()
        gt, edges, _, _ = form(two_cells(4))                 # cell 2 = columns 8..10, dilated 4..14
        want = two_cells(4)
        want[4:7, 4] = 0                                     # cell 1's last column lies in cell 2's dilation
        want[4:7, 8] = 0                                     # cell 2's first column lies in cell 1's (0..8)
        assert np.array_equal(gt, want) and (edges[4:7, 4] == 255).all() and (edges[4:7, 8] == 255).all()
        gt = form(two_cells(3))[0]                           # cell 2 = columns 7..9, dilated 3..13
        assert (gt[4:7, 3:5] == 0).all() and (gt[4:7, 2] == 1).all()
        assert (gt[4:7, 7:9] == 0).all() and (gt[4:7, 9] == 2).all()


def test_ids_above_255_survive_one_neighbour():
    """A cell of id 600 (columns 0..4) touching a cell of id 7 (columns 5..9): within 4 columns of the other cell the
    600-pixels become 600 - 255 = 345 and stay foreground, the 7-pixels become 0; columns 0 and 9 are out of reach."""
    ids = np.zeros((6, 10), np.int64)
    ids[:, :5] = 600
    ids[:, 5:] = 7
    want = np.zeros_like(ids)
    want[:, 0] = 600
    want[:, 1:5] = 345
    want[:, 9] = 7
    for form in (ref.carve_literal, ref.carve_fast):
        gt, edges, binary, _ = form(ids)
        assert np.array_equal(gt, want)
        assert all(row.tolist() == [0, 255, 255, 255, 255, 255, 255, 255, 255, 0] for row in edges)
        assert np.array_equal(binary, 255 * (want > 0))


def test_one_by_one_and_out_of_range():
    for form in (ref.carve_literal, ref.carve_fast):
        for v in (0, 9):
            gt, edges, binary, bad = form(np.array([[v]]))
            assert gt.tolist() == [[v]] and edges.tolist() == [[0]] and binary.tolist() == [[255 if v else 0]] and bad == 0
        ids = np.array([[5, -1, 5, 1 << 24, 5, 0, 0, 0, 0, 0, 6]])
        gt, edges, binary, bad = form(ids)
        assert bad == 2 and gt.tolist() == [[5, 0, 5, 0, 5, 0, 0, 0, 0, 0, 6]]      # 6 is 6 columns from the last 5: out of reach
    assert ref.clean(np.array([[np.nan, 2.0, -0.5]]))[1] == 2


def test_crop_counts_and_probabilities_equal_the_reference(golden):
    """The summed-area counts give the reference's distribution back bit for bit through the reference's own expression, and
    data.crop_probabilities (no scipy) within 1e-12 relative on the non-zero entries with the same zero pattern.  The bound:
    x, z, z^2 / 2, exp, the two divisions, the product by 10 and the division by the sum are fewer than ten float64 roundings
    (1.1e-16 each); the ones before exp are amplified by at most z^2 / 2 <= 32 (|z| <= 8 inside [0.1, 0.9]); the sum of
    non-negative terms is as accurate as its terms: about 1e-14 in all, 1e-12 with two orders to spare."""
    import data
    mixed = 0
    for name in golden["names"]:
        binary = golden[name + "_bin"]
        H, W = binary.shape
        for crop in golden[name + "_crops"]:
            want = golden["%s_p%d" % (name, crop)]
            assert golden["%s_pairs%d" % (name, crop)].tolist() == [list(p) for p in ref.crop_pairs(H, W, crop)]
            counts = ref.crop_counts(binary, crop)
            assert counts.shape == (len(range(0, H - crop, 10)), len(range(0, W - crop, 10)))
            assert np.array_equal(ref.crop_probabilities(counts, crop), want)
            got = data.crop_probabilities(counts, crop)
            assert got.shape == want.shape and got.dtype == np.float64
            assert np.array_equal(got == 0, want == 0)
            nz = want != 0
            assert (np.abs(got[nz] - want[nz]) <= 1e-12 * want[nz]).all()
            mixed += bool(nz.any() and (~nz).any())
            both = data.crop_probabilities(np.stack([counts, np.zeros_like(counts)]), crop)
            assert np.array_equal(both[0], got) and np.array_equal(both[1], np.full(counts.size, 1.0 / counts.size))
    assert mixed >= 1                                        # some image has windows inside and outside [0.1, 0.9]
    assert np.array_equal(golden["zeros_p36"], [0.5, 0.5])  # the uniform fallback


def test_draw_crop_follows_the_reference_generator(golden):
    import data
    binary = golden["discs_bin"]
    crop = int(golden["discs_crops"][0])
    pairs = [tuple(p) for p in golden["discs_pairs%d" % crop].tolist()]
    p = golden["discs_p%d" % crop]
    for s in golden["draw_seeds"]:
        rng = np.random.RandomState(int(s))
        x, y = data.draw_crop(rng, pairs, p, binary.shape, crop)
        rot = rng.choice(np.arange(0, 360, 30))
        assert [x, y, rot] == golden["draw%d" % s].tolist()
        st = rng.get_state()
        assert np.array_equal(st[1], golden["draw%d_keys" % s]) and [st[2], st[3]] == golden["draw%d_pos" % s].tolist()
    # clamping: a jitter below 0 or past dim - crop is pulled back
    for s in range(20):
        x, y = data.draw_crop(np.random.RandomState(s), [(0, 0), (60, 80)], np.array([0.5, 0.5]), (96, 120), 36)
        assert 0 <= x <= 60 and 0 <= y <= 84
