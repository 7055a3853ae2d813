"""Cell instances and the SEG measure on the device (functions.label_cells -> unet_label_components, functions.seg_measure ->
unet_instance_overlap, tester.segment(return_instances=True)) against the numpy/scipy restatement tests/instances_ref.py
(pinned to hand-worked answers by tests/test_instances_cpu.py).  Everything here is exact: integers, and float64 values
formed from equal integers by one formula.  Every pointer handed to the raw entry points is a poisoned guarded.Arena buffer."""
import numpy as np
import pytest
import torch

import guarded
import instances_ref as ref
import multiclass_ref
from gpu_support import dev

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 2), (2, 1), (1, 40), (17, 5), (33, 31), (64, 64), (37, 300), (300, 37), (129, 97), (516, 516), (520, 696)]
KINDS = ["discs", "speckle0.3", "speckle0.5", "speckle0.6", "speckle0.8", "zeros", "ones", "serpentine", "comb"]
CASES = ((1, 9, 128, 128), (2, 37, 256, 256), (3, 99, 388, 388))          # seed, cells, H, W of instances_ref.cells_case


def raw_label(dev, mask):
    """unet_label_components on guarded buffers: (labels, n_objects) as numpy."""
    import _hip
    a = guarded.Arena(dev)
    B, H, W = mask.shape
    m = a.inp(torch.from_numpy(mask), "mask")
    labels = a.out((B, H, W), torch.int32, "labels")
    n = a.out((B,), torch.int32, "n_objects")
    scratch = a.scratch(_hip.lib().unet_label_components_scratch_bytes(B, H, W), "scratch")
    _hip.run("unet_label_components", dev, a.ptr(m), 0 if mask.dtype == np.int64 else 1, B, H, W, a.ptr(labels), a.ptr(n), a.ptr(scratch))
    a.verify(labels, n)
    return labels.cpu().numpy(), n.cpu().numpy()


def raw_overlap(dev, gt, pred, ng_max, np_max, slots):
    """unet_instance_overlap on guarded buffers: area_gt, area_pred, match, inter, status as numpy int64."""
    import _hip
    a = guarded.Arena(dev)
    B, H, W = gt.shape
    g, p = a.inp(torch.from_numpy(gt), "gt"), a.inp(torch.from_numpy(pred), "pred")
    outs = [a.out((B, n), torch.int32, name) for name, n in (("area_gt", ng_max + 1), ("area_pred", np_max + 1), ("match", ng_max + 1),
                                                             ("inter", ng_max + 1))]
    status = a.out((B, 2), torch.int64, "status")
    scratch = a.scratch(_hip.lib().unet_instance_overlap_scratch_bytes(B, ng_max, np_max, slots), "scratch")
    _hip.run("unet_instance_overlap", dev, a.ptr(g), a.ptr(p), B, H, W, ng_max, np_max, slots, *(a.ptr(o) for o in outs), a.ptr(status),
             a.ptr(scratch))
    a.verify(*outs, status)
    return [o.cpu().numpy().astype(np.int64) for o in outs] + [status.cpu().numpy()]


def ref_overlap(gt, pred, ng_max, np_max):
    per = [ref.overlaps(g, p, ng_max, np_max) for g, p in zip(gt, pred)]
    return [np.stack([r[k] for r in per]) for k in range(4)] + [[r[4] for r in per], [r[5] for r in per]]


@pytest.mark.parametrize("H,W", SIZES)
def test_labels_equal_scipy(dev, H, W):
    """Bit for bit, counts included: every kind of mask at this size, B 1-4, int64 and float32, through the raw entry point and
    through functions.label_cells."""
    import functions
    for k, kind in enumerate(KINDS):
        mask = ref.mask_batch(kind, 31 * H + W + k, H, W).astype(np.float32 if k % 2 else np.int64)
        if k % 2:
            mask *= 0.25                                  # foreground is value != 0, not value == 1
        want = [ref.label(m) for m in mask]
        labels, n = raw_label(dev, mask)
        assert n.tolist() == [w[1] for w in want], kind
        assert np.array_equal(labels, np.stack([w[0] for w in want])), kind
        lab2, n2 = functions.label_cells(torch.from_numpy(mask).to(dev))
        assert lab2.dtype == torch.int32 and n2.dtype == torch.int32 and lab2.shape == mask.shape
        assert np.array_equal(lab2.cpu().numpy(), labels) and np.array_equal(n2.cpu().numpy(), n), kind
    if H * W >= 64 * 64:
        assert max(ref.label(m)[1] for m in ref.mask_batch("speckle0.3", 31 * H + W + 1, H, W)) > H * W // 20


def test_label_cells_shapes_and_dtypes(dev):
    import functions
    m = ref.mask_batch("discs", 5, 70, 90)[0]
    want, n = ref.label(m)
    for t in (torch.from_numpy(m), torch.from_numpy(m).bool(), torch.from_numpy(m).int(), torch.from_numpy(m).double()):
        lab, cnt = functions.label_cells(t.to(dev))
        assert lab.shape == (70, 90) and cnt.tolist() == [n] and np.array_equal(lab.cpu().numpy(), want)
    with pytest.raises(ValueError):
        functions.label_cells(torch.zeros(1, 1, 4, 4, device=dev))
    import _hip
    z = torch.zeros(1, 4, 4, dtype=torch.int64, device=dev)
    o = torch.zeros(16, dtype=torch.int32, device=dev)
    assert _hip.lib().unet_label_components(_hip.ptr(z), 2, 1, 4, 4, _hip.ptr(o), _hip.ptr(o), _hip.ptr(o), None) == -2
    assert b"dtype" in _hip.lib().unet_last_error()


@pytest.mark.parametrize("seed,n,H,W", CASES)
def test_overlap_integers_equal_the_restatement(dev, seed, n, H, W):
    """Areas, match and inter, exactly; B = 2 (a second image from another seed), consecutive ids with exact maxima, then ids
    three apart below maxima larger than any id present."""
    for stride, slack in ((1, 0), (3, 17)):
        pairs = [ref.cells_case(s, n, H, W, stride=stride) for s in (seed, seed + 10)]
        gt, pred = (np.stack([p[k] for p in pairs]) for k in (0, 1))
        ng_max, np_max = int(gt.max()) + slack, int(pred.max()) + 2 * slack
        area_gt, area_pred, match, inter, bad, npairs = ref_overlap(gt, pred, ng_max, np_max)
        got = raw_overlap(dev, gt, pred, ng_max, np_max, 4096)
        assert got[4].tolist() == [[0, 0], [0, 0]]
        for name, g, w in zip(("area_gt", "area_pred", "match", "inter"), got, (area_gt, area_pred, match, inter)):
            assert np.array_equal(g, w), name
        present = area_gt[:, 1:] > 0
        matched = (match[:, 1:] > 0).sum()
        assert matched >= 1                                  # not vacuous: both branches of the rule are taken
        if n > 9:
            assert matched < present.sum()


def test_overlap_ids_out_of_range_are_counted_in_status_only(dev):
    gt, pred = (a[None].copy() for a in ref.cells_case(2, 37, 256, 256))
    ng_max, np_max = int(gt.max()) - 5, int(pred.max()) - 3         # the highest ids fall out of range
    gt[0, 0, :7] = -1
    pred[0, 1, :5] = -(2 ** 31)
    area_gt, area_pred, match, inter, bad, _ = ref_overlap(gt, pred, ng_max, np_max)
    assert bad[0] > 12
    got = raw_overlap(dev, gt, pred, ng_max, np_max, 1024)
    assert got[4].tolist() == [[bad[0], 0]]
    for g, w in zip(got, (area_gt, area_pred, match, inter)):
        assert np.array_equal(g, w)
    assert got[0].sum() == gt.size - bad[0] == got[1].sum()


def test_overlap_table_overflow_is_reported(dev):
    """Fewer slots than distinct pairs: status[:, 1] > 0, areas still exact, nothing outside the outputs touched (the arena's
    guards); with room for every pair the same call is exact."""
    gt, pred = (a[None] for a in ref.cells_case(3, 99, 388, 388))
    ng_max, np_max = int(gt.max()), int(pred.max())
    area_gt, area_pred, match, inter, _, npairs = ref_overlap(gt, pred, ng_max, np_max)
    assert npairs[0] > 64
    got = raw_overlap(dev, gt, pred, ng_max, np_max, 64)
    assert got[4][0, 0] == 0 and got[4][0, 1] > 0
    assert np.array_equal(got[0], area_gt) and np.array_equal(got[1], area_pred)
    slots = 1 << int(npairs[0]).bit_length()
    got = raw_overlap(dev, gt, pred, ng_max, np_max, slots)
    assert got[4].tolist() == [[0, 0]] and np.array_equal(got[2], match) and np.array_equal(got[3], inter)
    import _hip
    t = torch.zeros(64, dtype=torch.int32, device=dev)
    args = [_hip.ptr(t)] * 2 + [1, 8, 8, 3, 3, 48] + [_hip.ptr(t)] * 6 + [None]
    assert _hip.lib().unet_instance_overlap(*args) == -2 and b"power of two" in _hip.lib().unet_last_error()


def check_seg(got, want):
    assert got.seg == want["seg"] or (np.isnan(got.seg) and np.isnan(want["seg"]))
    assert np.array_equal(got.per_image, want["per_image"], equal_nan=True)
    assert len(got.jaccard) == len(want["jaccard"]) and all(np.array_equal(a, b) for a, b in zip(got.jaccard, want["jaccard"]))
    assert (got.jaccard_sum, got.n_gt, got.n_matched, got.n_pred) == tuple(want[k] for k in ("jaccard_sum", "n_gt", "n_matched", "n_pred"))
    assert isinstance(got.n_gt, int) and isinstance(got.jaccard_sum, float) and got.per_image.dtype == np.float64


@pytest.mark.parametrize("seed,n,H,W", CASES)
def test_seg_measure_equals_the_restatement(dev, seed, n, H, W):
    import functions
    pairs = [ref.cells_case(s, n, H, W, stride=1 + seed % 2) for s in (seed, seed + 10, seed + 20)]
    gt, pred = (np.stack([p[k] for p in pairs]) for k in (0, 1))
    want = ref.seg(gt, pred)
    assert 0 < want["seg"] < 1
    got = functions.seg_measure(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev))
    check_seg(got, want)
    check_seg(functions.seg_measure(torch.from_numpy(pred).long().to(dev), torch.from_numpy(gt).to(dev)), want)
    one = functions.seg_measure(torch.from_numpy(pred[0]).to(dev), torch.from_numpy(gt[0]).to(dev))
    check_seg(one, ref.seg(gt[:1], pred[:1]))
    # a tiny first table: the overflow protocol doubles it until every pair fits, and the result is the same
    check_seg(functions.seg_measure(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), _table_slots=2), want)


def test_seg_measure_edges_and_errors(dev):
    import functions
    z = torch.zeros(2, 9, 7, dtype=torch.int32, device=dev)
    r = functions.seg_measure(z + 1, z)
    assert np.isnan(r.seg) and r.n_gt == 0 and r.n_pred == 2 and np.isnan(r.per_image).all() and [len(j) for j in r.jaccard] == [0, 0]
    r = functions.seg_measure(z, z + 4)
    assert r.seg == 0.0 and r.n_gt == 2 and r.n_matched == 0 and r.n_pred == 0
    r = functions.seg_measure(z + 2, z + 4)
    assert r.seg == 1.0 and r.n_matched == 2
    neg = z.clone(); neg[1, 2, 3] = -1
    with pytest.raises(ValueError, match="negative"):
        functions.seg_measure(z, neg)
    with pytest.raises(ValueError):
        functions.seg_measure(z, z[:1])
    with pytest.raises(ValueError):
        functions.seg_measure(z.float(), z)


def test_labels_feed_seg_measure_and_side_stream_is_identical(dev):
    """label_cells -> seg_measure end to end on device tensors, on the default stream and on another one."""
    import functions
    gt, pred = (np.stack(x) for x in zip(*(ref.cells_case(s, 60, 300, 420) for s in (4, 5))))
    g, fg = torch.from_numpy(gt).to(dev), torch.from_numpy(pred != 0).to(dev)
    lab0, n0 = functions.label_cells(fg)
    seg0 = functions.seg_measure(lab0, g)
    check_seg(seg0, ref.seg(gt, np.stack([ref.label(p)[0] for p in pred != 0])))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        lab1, n1 = functions.label_cells(fg)
        seg1 = functions.seg_measure(lab1, g)
    s.synchronize()
    assert torch.equal(lab0, lab1) and torch.equal(n0, n1)
    assert seg1.seg == seg0.seg and all(np.array_equal(a, b) for a, b in zip(seg0.jaccard, seg1.jaccard))
    big = torch.from_numpy(ref.mask_batch("speckle0.6", 3, 516, 516)).to(dev)
    first = functions.label_cells(big)
    for _ in range(10):                                      # a racy union-find or scan would change labels or counts
        again = functions.label_cells(big)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


@pytest.mark.parametrize("K", [2, 3])
def test_segment_return_instances(dev, K):
    """The keyword adds the labels and changes nothing else: mask and probabilities bit-identical, labels = label_cells(mask) =
    scipy's labels of the mask; single images follow the mask's shape rule."""
    import functions
    import network
    import tester
    net = network.Unet(n_classes=K)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in multiclass_ref.head_params(K, seed=1).items()})
    net = net.to(dev)
    x = torch.from_numpy((np.random.RandomState(K).rand(2, 130, 201) * 255).astype(np.float32)).to(dev)
    m0 = tester.segment(net, x, tile_size=220, max_batch=3)
    m1, inst = tester.segment(net, x, tile_size=220, max_batch=3, return_instances=True)
    assert torch.equal(m0, m1) and inst.dtype == torch.int32 and inst.shape == m0.shape and inst.is_cuda
    want = np.stack([ref.label(m)[0] for m in m0.cpu().numpy()])
    print("K=%d: foreground fraction %.3f, components per image %s" % (K, (want > 0).mean(), [int(w.max()) for w in want]))
    assert np.array_equal(inst.cpu().numpy(), want) and torch.equal(inst, functions.label_cells(m0)[0])
    mp0, p0 = tester.segment(net, x, tile_size=220, max_batch=3, return_probs=True)
    out = tester.segment(net, x, tile_size=220, max_batch=3, return_probs=True, return_instances=True)
    assert len(out) == 3 and torch.equal(out[0], m0) and torch.equal(mp0, m0) and torch.equal(out[1], p0) and torch.equal(out[2], inst)
    s1 = tester.segment(net, x[1], tile_size=220, return_probs=True, return_instances=True)
    assert s1[0].shape == (130, 201) and s1[2].shape == (130, 201) and torch.equal(s1[2], inst[1]) and torch.equal(s1[0], m0[1])
    assert s1[1].shape == ((130, 201) if K == 2 else (3, 130, 201))
