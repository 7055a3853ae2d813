"""Nearest-cell growth, the foreground pair table and the Rand / information scores on the device (functions.grow_cells ->
unet_grow_labels, functions.pair_table -> unet_partition_pairs, functions.rand_scores) against the numpy restatement
tests/rand_ref.py (pinned to the all-pairs definition and to hand-worked answers by tests/test_rand_cpu.py).  The growth, the
table, the integers and the Rand scores are exact; the information scores are float64 sums by math.fsum on both sides and agree to
1e-12 relative on images with H_pred, H_gt > 0.1 (checked on the CPU).  Every pointer handed to the raw entry points is a poisoned
guarded.Arena buffer."""
import numpy as np
import pytest
import torch

import guarded
import instances_ref
import rand_ref as ref
from gpu_support import dev

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 2), (2, 1), (1, 40), (17, 5), (33, 31), (64, 64), (63, 65), (37, 300), (300, 37), (129, 97), (257, 255)]


def raw_grow(dev, ids, max_dist2):
    """unet_grow_labels on guarded buffers: the grown map as numpy."""
    import _hip
    a = guarded.Arena(dev)
    B, H, W = ids.shape
    lab = a.inp(torch.from_numpy(ids), "labels")
    out = a.out((B, H, W), torch.int32, "out")
    scratch = a.scratch(_hip.lib().unet_grow_labels_scratch_bytes(B, H, W), "scratch")
    _hip.run("unet_grow_labels", dev, a.ptr(lab), B, H, W, -1 if max_dist2 is None else max_dist2, a.ptr(out), a.ptr(scratch))
    a.check()                                                # an id may be 0xffffffff's neighbour but never it: ids < 2^24
    a.assert_written(out)
    return out.cpu().numpy()


def raw_pairs(dev, gt, pred, ng_max, np_max, slots):
    """unet_partition_pairs on guarded buffers: (b, g, p, n) sorted, and status, as numpy int64."""
    import _hip
    a = guarded.Arena(dev)
    B, H, W = gt.shape
    g, p = a.inp(torch.from_numpy(gt), "gt"), a.inp(torch.from_numpy(pred), "pred")
    keys, counts = a.out((slots,), torch.int64, "pair_keys"), a.out((slots,), torch.int32, "pair_counts")
    n_pairs, status = a.out((1,), torch.int64, "n_pairs"), a.out((B, 2), torch.int64, "status")
    scratch = a.scratch(_hip.lib().unet_partition_pairs_scratch_bytes(B, slots), "scratch")
    _hip.run("unet_partition_pairs", dev, a.ptr(g), a.ptr(p), B, H, W, ng_max, np_max, slots, a.ptr(keys), a.ptr(counts), a.ptr(n_pairs),
             a.ptr(status), a.ptr(scratch))
    a.verify(n_pairs, status)
    n = int(n_pairs.item())
    assert 0 <= n <= slots
    k, c = keys.cpu().numpy(), counts.cpu().numpy()
    assert (k[n:] == -1).all() and (c[n:] == -1).all()       # past n_pairs the lists are untouched (still poison)
    assert len(np.unique(k[:n])) == n                        # no pair twice
    o = np.argsort(k[:n])
    k, c = k[:n][o], c[:n][o].astype(np.int64)
    return (k >> 48, (k >> 24) & ref.ID_MAX, k & ref.ID_MAX, c), status.cpu().numpy()


def same_table(got, want):
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), [(len(a), len(b)) for a, b in zip(got, want)]


def check_grow(dev, name, ids, distances=ref.DISTANCES, int64=False):
    import functions
    want = ref.grow_batch(ids, [ref.dist2(d) for d in distances])
    t = torch.from_numpy(ids).to(dev)
    for d in distances:
        m = ref.dist2(d)
        assert np.array_equal(raw_grow(dev, ids, m), want[m]), (name, d)
        got = functions.grow_cells(t.long() if int64 else t, d)
        assert got.dtype == torch.int32 and got.shape == t.shape and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want[m]), (name, d)
    return want


@pytest.mark.parametrize("H,W", SIZES)
def test_growth_equals_the_restatement(dev, H, W):
    """Bit for bit: every kind of id map at this size (B 1-4), unlimited and at every limit, through the raw entry point and
    through functions.grow_cells (int32 and int64 ids in turn)."""
    grew, sizes = 0, set()
    for k, (name, ids) in enumerate(ref.id_cases(H, W, 0)):
        want = check_grow(dev, name, ids, int64=k % 2 == 1)
        grew += int((want[None] != ids).sum())
        sizes.add(len(ids))
        assert np.array_equal(want[0], ids), name           # max_distance = 0 is the identity
    assert grew > 0 or H * W <= 2
    assert max(sizes) >= 3 and min(sizes) <= 2, sizes


def test_growth_of_a_516_image(dev):
    """The largest image of the suite (three workgroups per row, the last one partial): discs with a speckle of single-pixel
    cells between them, and a sparse second image whose cells are hundreds of pixels apart."""
    a = instances_ref.mask_batch("discs", 1, 516, 516)[0].astype(np.int64)
    rs = np.random.RandomState(516)
    ids = np.zeros((2, 516, 516), np.int32)
    ids[0] = np.where(a > 0, 3 * instances_ref.label(a)[0] + 5, (rs.rand(516, 516) < 0.002) * rs.randint(1, 1 << 24, (516, 516)))
    ids[1] = (rs.rand(516, 516) < 0.0001) * rs.randint(1, 4, (516, 516))
    check_grow(dev, "516", ids, distances=(None, 4, 7.3))


def test_growth_of_a_wide_row(dev):
    """W > 1024 + 256: several LDS rounds per workgroup, unlimited (every round holds candidates) and with a limit whose window
    starts and ends inside rounds; one row costs the restatement W^2 only."""
    rs = np.random.RandomState(5)
    ids = ((rs.rand(2, 3, 2700) < 0.01) * rs.randint(1, 6, (2, 3, 2700))).astype(np.int32)
    ids[1, :, 300:2500] = 0                                   # nearest cells more than two rounds away
    check_grow(dev, "wide", ids, distances=(None, 4, 600))


def test_every_tie_order(dev):
    """The centre and the mid-edges of a square are equally far from two or four labelled pixels (within a column, between
    columns, both): all 24 orders of the ids, so the first in raster order is the smallest in some images and not in others."""
    for H, W in ((9, 12), (24, 70)):
        t = ref.tie_maps(H, W)
        for k in range(0, 24, 4):
            want = check_grow(dev, "ties", t[k:k + 4], distances=(None, 1, 1.5, 2))
            assert (want[None][:, 1, 1] == 2).all() and (want[1][:, 1, 1] == 0).all() and (want[2][:, 1, 1] == 2).all()


def test_the_limit_is_inclusive(dev):
    """A labelled pixel at exactly d^2 = floor(max_distance^2) is in reach, one at d^2 + 1 is not."""
    m = np.zeros((1, 21, 23), np.int32)
    m[0, 10, 11] = 6
    yy, xx = np.mgrid[0:21, 0:23]
    d2 = (yy - 10) ** 2 + (xx - 11) ** 2
    for d in ref.DISTANCES[1:]:
        got = raw_grow(dev, m, ref.dist2(d))
        assert np.array_equal(got[0], np.where(d2 <= ref.dist2(d), 6, 0)), d
    g = raw_grow(dev, m, 53)[0]
    assert g[12, 18] == 6 and g[13, 18] == 0                 # 4 + 49 = 53, 9 + 49 = 58


def test_grow_cells_shapes_and_errors(dev):
    import _hip
    import functions
    ids = ref.id_cases(33, 31, 0)[0][1]
    one = functions.grow_cells(torch.from_numpy(ids[0]).to(dev), 4)
    assert one.shape == (33, 31) and np.array_equal(one.cpu().numpy(), ref.grow(ids[0], 16))
    assert torch.equal(functions.grow_cells(torch.from_numpy(ids).to(dev), float("inf")), functions.grow_cells(torch.from_numpy(ids).to(dev)))
    z = torch.zeros(2, 9, 7, dtype=torch.int32, device=dev)
    assert not functions.grow_cells(z).any() and (functions.grow_cells(z + 3, 2) == 3).all()
    neg = z.clone(); neg[1, 2, 3] = -1
    with pytest.raises(ValueError, match="negative"):
        functions.grow_cells(neg)
    big = z.long(); big[0, 0, 0] = 1 << 24
    with pytest.raises(ValueError, match="2\\^24"):
        functions.grow_cells(big)
    with pytest.raises(ValueError):
        functions.grow_cells(z, -1)
    with pytest.raises(ValueError):
        functions.grow_cells(z.float())
    o = torch.zeros(64, dtype=torch.int32, device=dev)
    assert _hip.lib().unet_grow_labels(_hip.ptr(o), 1, 1, 70000, -1, _hip.ptr(o), _hip.ptr(o), None) == -2
    assert b"W is at most" in _hip.lib().unet_last_error()
    assert _hip.lib().unet_grow_labels(_hip.ptr(o), 0, 8, 8, -1, _hip.ptr(o), _hip.ptr(o), None) == -2


# ---- the pair table -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def seeded():
    return ref.seeded_pairs()


def test_pair_table_equals_the_restatement(dev, seeded):
    """(b, g, p, n) after sorting, through the raw entry point (exact maxima, then maxima larger than any id) and through
    functions.pair_table; a table of two slots is doubled until every pair fits and ends the same."""
    import functions
    for name, pred, gt in seeded:
        want = ref.pairs(pred, gt)
        assert (want[2] == 0).any() and len(want[0]) > 8, name
        slots = 1 << (2 * len(want[0])).bit_length()
        for slack in (0, 17):
            got, status = raw_pairs(dev, gt, pred, int(gt.max()) + slack, int(pred.max()) + 2 * slack, slots)
            assert status.tolist() == [[0, 0]] * len(gt), name
            same_table(got, want)
        p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        got = functions.pair_table(p, g)
        assert all(a.dtype == np.int64 for a in got)
        same_table(got, want)
        same_table(functions.pair_table(p.long(), g, _table_slots=2), want)
    same_table(functions.pair_table(p[1], g[1]), ref.pairs(pred[1:], gt[1:]))


def test_pair_table_speckle_and_an_empty_image(dev):
    """Thousands of pairs between hundreds of ids, B = 3 with one all-background ground truth (no entry for it); then pred ids
    on gt background are changed at will, and a whole pred image set to 0: only the p = 0 column is left of it."""
    import functions
    pred, gt = ref.speckle_pairs()
    want = ref.pairs(pred, gt)
    got, status = raw_pairs(dev, gt, pred, int(gt.max()), int(pred.max()), 1 << 15)
    assert status.tolist() == [[0, 0]] * 3 and not (got[0] == 1).any()
    same_table(got, want)
    other = np.where(gt == 0, (pred * 7 + 3) % 390, pred).astype(np.int32)
    same_table(raw_pairs(dev, gt, other, int(gt.max()), int(pred.max()), 1 << 15)[0], want)
    other[2] = 0
    got = functions.pair_table(torch.from_numpy(other).to(dev), torch.from_numpy(gt).to(dev))
    same_table(got, ref.pairs(other, gt))
    assert (got[2][got[0] == 2] == 0).all() and np.array_equal(got[3][got[0] == 2], np.bincount(gt[2].ravel())[np.unique(gt[2])][1:])


def test_pair_table_overflow_and_ids_out_of_range(dev, seeded):
    """Fewer slots than pairs: status[:, 1] > 0, every entry that is listed is a true pair with no more than its pixels, nothing
    outside the outputs touched.  Ids out of range are counted in status[:, 0], whatever the gt value, and are in no entry."""
    import _hip
    import functions
    name, pred, gt = seeded[3]                               # cells 256
    want = ref.pairs(pred, gt)
    truth = {(b, g, p): n for b, g, p, n in zip(*(w.tolist() for w in want))}
    assert len(truth) > 64
    got, status = raw_pairs(dev, gt, pred, int(gt.max()), int(pred.max()), 64)
    assert status[:, 0].tolist() == [0, 0] and status[:, 1].sum() > 0 and len(got[0]) == 64
    assert all(n <= truth[(b, g, p)] for b, g, p, n in zip(*(w.tolist() for w in got)))
    assert got[3].sum() + status[:, 1].sum() == (gt >= 1).sum()
    bad_gt, bad_pred = gt.copy(), pred.copy()
    ng_max, np_max = int(gt.max()) - 5, int(pred.max()) - 3
    bad_gt[0, 0, :7] = -1
    bad_pred[1, 1, :5] = -(2 ** 31)
    bad = (bad_gt < 0) | (bad_gt > ng_max) | (bad_pred < 0) | (bad_pred > np_max)
    assert (bad & (bad_gt == 0)).any() and (bad & (bad_gt > 0)).any()
    got, status = raw_pairs(dev, bad_gt, bad_pred, ng_max, np_max, 4096)
    assert status.tolist() == [[int(b.sum()), 0] for b in bad]
    same_table(got, ref.pairs(np.where(bad, 0, bad_pred), np.where(bad, 0, bad_gt)))
    p, g = torch.from_numpy(bad_pred).to(dev), torch.from_numpy(bad_gt).to(dev)
    with pytest.raises(ValueError, match="12 pixels hold negative ids"):      # the count is the kernel's: status[:, 0]
        functions.pair_table(p, g)
    with pytest.raises(ValueError, match="12 pixels hold negative ids"):
        functions.rand_scores(p, g)
    with pytest.raises(ValueError, match="negative"):
        functions.rand_scores(p, g, grow=2)
    t = torch.zeros(64, dtype=torch.int32, device=dev)
    args = [_hip.ptr(t)] * 2 + [1, 8, 8, 3, 3, 48] + [_hip.ptr(t)] * 5 + [None]
    assert _hip.lib().unet_partition_pairs(*args) == -2 and b"power of two" in _hip.lib().unet_last_error()


# ---- the scores ---------------------------------------------------------------------------------------------------------------

def test_rand_scores_equal_the_restatement(dev, seeded):
    import functions
    for name, pred, gt in seeded:
        p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        for alpha in (0.5, 0.3):
            ref.check_scores(functions.rand_scores(p, g, alpha=alpha), ref.scores(pred, gt, alpha))
    ref.check_scores(functions.rand_scores(p[0], g[0].long()), ref.scores(pred[:1], gt[:1]))
    pred, gt = ref.speckle_pairs()
    got = functions.rand_scores(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev))
    ref.check_scores(got, ref.scores(pred, gt))
    assert all(np.isnan(getattr(got, k)[1]) for k in ref.SCORES) and got.N[1] == 0      # N = 0: every score nan, the means skip it
    assert got.rand_error_mean == got.rand_error[[0, 2]].mean()
    z = torch.zeros(2, 9, 7, dtype=torch.int32, device=dev)
    r = functions.rand_scores(z + 4, z + 2)                  # one segment on either side: H = 0, 0 / 0 is nan; the Rand scores are 1
    assert (r.rand_error == 0).all() and np.isnan(r.v_info).all() and np.isnan(r.v_info_mean) and (r.voi_split == 0).all()
    assert r.N.tolist() == [63, 63] and r.S_pair.tolist() == [63 * 63] * 2 and r.c.tolist() == [0, 0]
    r = functions.rand_scores(z, z + 2)                      # all singletons
    assert r.c.tolist() == [63, 63] and r.S_pair.tolist() == [63, 63] and (r.rand_split == 1 / 63).all() and (r.rand_merge == 1).all()


def test_rand_scores_after_growth(dev, seeded):
    import functions
    name, pred, gt = seeded[0]
    p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    plain = functions.rand_scores(p, g)
    for grow, d in ((True, None), (4, 4), (1.5, 1.5)):
        got = functions.rand_scores(p, g, grow=grow)
        explicit = functions.rand_scores(functions.grow_cells(p, d), g)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, explicit))
        ref.check_scores(got, ref.scores(ref.grow_batch(pred, [ref.dist2(d)])[ref.dist2(d)], gt))
        assert (got.c < plain.c).all()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(functions.rand_scores(p, g, grow=False), plain))
    assert (functions.rand_scores(p, g, grow=True).c == 0).all()


@pytest.mark.parametrize("seed,n,H,W", ref.E2E)
def test_growth_hands_the_carved_rim_back(dev, seed, n, H, W):
    """gt -> binary_target -> label_cells -> grow_cells -> seg_measure / rand_scores, all on the device: on these images (chosen
    and shown to have the property by test_rand_cpu.test_growth_hands_the_carved_rim_back, which also says when it does not
    hold) growth by the carve's reach does not lower SEG, and unlimited growth does not raise the Rand error."""
    import data
    import functions
    gt_np = instances_ref.cells_case(seed, n, H, W)[0]
    gt = torch.from_numpy(gt_np).to(dev)
    pred = functions.label_cells(data.binary_target(gt) > 0)[0]
    assert np.array_equal(pred.cpu().numpy(), ref.carved_prediction(gt_np[None])[0])
    s0, s1 = functions.seg_measure(pred, gt).seg, functions.seg_measure(functions.grow_cells(pred, 4), gt).seg
    e0, e1 = functions.rand_scores(pred, gt).rand_error[0], functions.rand_scores(pred, gt, grow=True).rand_error[0]
    print("%d x %d, seed %d: SEG %.4f -> %.4f, Rand error %.4f -> %.4f" % (H, W, seed, s0, s1, e0, e1))
    assert s1 >= s0 and e1 <= e0
