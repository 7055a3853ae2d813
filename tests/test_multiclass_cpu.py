"""K-class nets without a GPU: Unet(n_classes=K) shapes, keys and seeded draws, the argument checks that run before any device
work, the metrics from confusion counts, and the numpy restatements of tests/multiclass_ref.py against torch in fp64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multiclass_ref as ref


@pytest.mark.parametrize("K", [2, 3, 8, 16])
def test_unet_n_classes_shapes_and_keys(K):
    import network
    m, m2 = network.Unet(n_classes=K), network.Unet()
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert list(sd) == list(sd2) and len(sd) == 46
    for k in sd:
        want = (K, 64, 1, 1) if k == "finalconv.weight" else (K,) if k == "finalconv.bias" else tuple(sd2[k].shape)
        assert tuple(sd[k].shape) == want, k
    assert m.n_classes == K
    h = network.Unet(base_ch=32, n_classes=K)
    assert tuple(h.finalconv.weight.shape) == (K, 32, 1, 1)


def test_n_classes_2_draws_the_same_parameters_as_unet():
    import network
    torch.manual_seed(1234)
    a = network.Unet()
    torch.manual_seed(1234)
    b = network.Unet(n_classes=2)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka


@pytest.mark.parametrize("K", [0, 1, 17, 2.0, "3", True, None])
def test_invalid_n_classes_raise(K):
    import network
    with pytest.raises(ValueError):
        network.Unet(n_classes=K)


@pytest.mark.parametrize("K,loss,weights,ok", [
    (2, "bce", "class_balance", True), (2, "bce", "border", True), (2, "softmax_ce", "class_balance", True),
    (2, "softmax_ce", "border", True), (2, "softmax_ce", "none", True), (3, "softmax_ce", "none", True),
    (3, "bce", "none", False), (3, "bce", "class_balance", False), (3, "softmax_ce", "class_balance", False),
    (8, "softmax_ce", "border", False), (2, "ce", "class_balance", False), (2, "bce", "uniform", False)])
def test_loss_option_checks(K, loss, weights, ok):
    import trainer
    if ok:
        trainer.check_loss_options(K, loss, weights)
    else:
        with pytest.raises(ValueError):
            trainer.check_loss_options(K, loss, weights)


def test_training_rejects_bad_combinations_before_device_work(tmp_path):
    """No loader item is touched and no directory is made: the check comes first."""
    import network
    import trainer

    class Boom:
        def __iter__(self):
            raise AssertionError("loader touched")

        def __len__(self):
            return 1

    net = network.Unet(n_classes=3)
    for kw in (dict(), dict(loss="softmax_ce"), dict(loss="bce", loss_weights="none"), dict(loss="nll", loss_weights="none")):
        with pytest.raises(ValueError):
            trainer.training(net, Boom(), Boom(), 1, 1, "cpu", str(tmp_path / "f"), "X", **kw)
    assert not (tmp_path / "f").exists()


def test_testing_rejects_k_class_nets(tmp_path):
    import network
    import tester
    with pytest.raises(ValueError):
        tester.testing(network.Unet(n_classes=4), [], 1, "cpu", str(tmp_path))


def test_metrics_from_confusion():
    from functions import metrics_from_confusion, metrics_from_counts
    rs = np.random.RandomState(3)
    for _ in range(20):
        pred = rs.randint(0, 2, (17, 23))
        lab = rs.randint(0, 2, (17, 23))
        conf, _ = ref.confusion(pred[None], lab[None], 2)
        inter, union, diff = int((pred & lab).sum()), int((pred | lab).sum()), int(np.abs(pred - lab).sum())
        a, b = metrics_from_confusion(conf[0]), metrics_from_counts(inter, union, diff, pred.size)
        assert a.shape == b.shape == (2, 1) and np.array_equal(a, b)
    conf = np.array([[5, 1, 0], [2, 3, 0], [0, 0, 0]])        # class 2 absent: union 0, left out of the mean
    m = metrics_from_confusion(conf)
    assert m[0, 0] == 3 / 6 and m[1, 0] == 3 / 11
    conf = np.array([[4, 0, 0], [0, 0, 0], [0, 0, 0]])
    assert np.isnan(metrics_from_confusion(conf)[0, 0]) and metrics_from_confusion(conf)[1, 0] == 0.0
    conf = np.array([[1, 1, 0], [0, 2, 1], [1, 0, 3]])
    ious = [2 / (3 + 3 - 2), 3 / (4 + 4 - 3)]
    assert metrics_from_confusion(conf)[0, 0] == np.mean(ious)


@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("weighted", [False, True])
def test_numpy_softmax_ce_matches_torch_fp64(K, weighted):
    rs = np.random.RandomState(K)
    B, H, W = 2, 9, 13
    l = rs.randn(B, K, H, W) * 3
    lab = rs.randint(0, K, (B, H, W))
    lab[0, 0, :3] = [-1, K, K + 5]                                   # invalid labels: no loss, no gradient
    w = rs.uniform(0.2, 3, (B, H, W)) if weighted else None
    loss, d, mask, bad = ref.softmax_ce(l, lab, w, grad_scale=0.5)
    lt = torch.tensor(l, requires_grad=True)
    ok = torch.tensor((lab >= 0) & (lab < K))
    ce = F.cross_entropy(lt, torch.tensor(np.where(lab >= 0, lab, 0) % K), reduction="none")
    wt = torch.ones(B, H, W, dtype=torch.float64) if w is None else torch.tensor(w)
    tl = (ce * wt * ok).sum() / (B * H * W)
    (tl * 0.5).backward()
    assert bad == 3
    assert abs(loss - tl.item()) <= 1e-13 * abs(tl.item())
    assert np.abs(d - lt.grad.numpy()).max() <= 1e-15
    assert np.array_equal(mask, torch.argmax(torch.tensor(l), dim=1).numpy())


def test_numpy_confusion_matches_torch_bincount():
    rs = np.random.RandomState(5)
    for K in (2, 3, 7, 16):
        pred = rs.randint(0, K, (3, 11, 11))
        lab = rs.randint(-1, K + 1, (3, 11, 11))
        conf, bad = ref.confusion(pred, lab, K)
        for b in range(3):
            ok = (lab[b] >= 0) & (lab[b] < K)
            tb = torch.bincount(torch.tensor(lab[b][ok] * K + pred[b][ok]), minlength=K * K).reshape(K, K)
            assert np.array_equal(conf[b], tb.numpy()) and bad[b] == (~ok).sum()


def test_numpy_stitch_k_matches_torch():
    """K-class stitch of one-tile-per-image grids equals torch's argmax / softmax of the cropped logits; two classes reduce
    to segment_ref.stitch."""
    import segment_ref
    rs = np.random.RandomState(9)
    S, So = 220, 36
    for K in (2, 3, 5):
        lg = rs.randn(4, K, So, So).astype(np.float32)
        lg[:, 1, 0, :4] = lg[:, 0, 0, :4]                           # ties -> class 0
        mask, prob = ref.stitch_k(lg, 1, 60, 70, S)                 # 2 x 2 tiles
        full = np.zeros((K, 2 * So, 2 * So), np.float32)
        for t in range(4):
            i, j = divmod(t, 2)
            full[:, i * So:(i + 1) * So, j * So:(j + 1) * So] = lg[t]
        oy, ox = (2 * So - 60) // 2, (2 * So - 70) // 2
        crop = torch.tensor(full[:, oy:oy + 60, ox:ox + 70], dtype=torch.float64)
        assert np.array_equal(mask[0], torch.argmax(crop, dim=0).numpy())
        assert np.abs(prob[0] - torch.softmax(crop, dim=0).numpy()).max() <= 1e-15
        if K == 2:
            m2, p2 = segment_ref.stitch(lg, 1, 60, 70, S)
            assert np.array_equal(mask, m2) and np.abs(prob[:, 1] - p2).max() <= 1e-15


# ---- the inputs of tests/test_multiclass_ops_gpu.py are well-posed ----------------------------------------------------------

@pytest.mark.parametrize("K", [5, 9, 16])
def test_numpy_softmax_ce_matches_torch_fp64_on_extreme_logits(K):
    """multiclass_ref.softmax_ce on the 'extreme' family (logits up to +-1e4, invalid labels planted) against
    F.cross_entropy(reduction='none') in fp64 with the weight applied by hand and the gradient from autograd."""
    B, H, W = 3, 1, 683
    l, lab, w = ref.ce_cases(B, K, H, W, "extreme")
    lab, nbad = ref.plant_invalid(lab, K)
    assert np.abs(l).max() == 1e4
    loss, d, mask, bad = ref.softmax_ce(l, lab, w, grad_scale=0.25)
    ok = (lab >= 0) & (lab < K)
    lt = torch.tensor(l.astype(np.float64), requires_grad=True)
    ce = F.cross_entropy(lt, torch.tensor(np.where(ok, lab, 0)), reduction="none")
    tl = (ce * torch.tensor(w.astype(np.float64)) * torch.tensor(ok)).sum() / (B * H * W)
    (tl * 0.25).backward()
    assert bad == nbad == 5
    assert abs(loss - tl.item()) <= 1e-13 * abs(tl.item())
    assert np.abs(d - lt.grad.numpy()).max() <= 1e-15
    assert np.array_equal(mask, torch.argmax(torch.tensor(l), dim=1).numpy())
    assert (d.transpose(0, 2, 3, 1)[~ok] == 0).all()


def test_ce_shape_and_class_lists():
    assert [b * h * w for b, h, w in ref.CE_SHAPES] == [1, 2047, 2048, 2049, 2100, 255, 525312]
    assert 300 * 1 * 7 == 2100 and 1 * 7 < 256                        # a thread's next pixel lies 256 / 7 = 36 images on
    assert -(-525312 // 2048) == 257                                   # partials: one more than the finisher's 256 threads
    assert (3, 1, 683) in ref.CE_SMALL_SHAPES and 683 < 2048 < 3 * 683  # one block over three images
    small = [c for c in ref.CE_CASES if c[0] != ref.CE_LARGE_SHAPE]
    assert [c for c in ref.CE_CASES if c[0] == ref.CE_LARGE_SHAPE] == [(ref.CE_LARGE_SHAPE, 3)]
    assert len(set(small)) == len(small)
    for K in ref.ALL_K:
        assert sum(1 for s, k in small if k == K) >= 3, K
    for s in ref.CE_SMALL_SHAPES:
        assert sum(1 for t, k in small if t == s) >= 3, s
    assert set(k for _, k in small) == set(ref.ALL_K) == {2, 3, 4, 5, 8, 9, 16}


@pytest.mark.parametrize("family", ref.CE_FAMILIES)
@pytest.mark.parametrize("shape,K", ref.CE_CASES)
def test_ce_cases_are_well_posed(shape, K, family):
    """Ties where the shape has room, saturated pixels where claimed, invalid labels as planted, a loss of ordinary size,
    a positive finite bound; the reference's dlogits are exactly 0 at saturated pixels to within 1e-45 x w / n."""
    B, H, W = shape
    npix = B * H * W
    x, lab, w = ref.ce_cases(B, K, H, W, family)
    assert x.dtype == np.float32 and x.shape == (B, K, H, W) and lab.dtype == np.int64 and w.dtype == np.float32
    assert np.isfinite(x).all() and lab.min() >= 0 and lab.max() < K and w.min() >= 0.1 and w.max() <= 4.0
    f = x.transpose(1, 0, 2, 3).reshape(K, -1)
    t_all, t_last, t_one = ref.tie_pixels(npix)
    if npix >= 3:
        assert len({t_all, t_last, t_one}) == 3
        assert (f[:, t_all] == f[0, t_all]).all()
        assert f[K - 1, t_last] == f[:, t_last].max() and f[1, t_one] == f[:, t_one].max()
        if K > 2:                                                      # a lower class shares the maximum: the first one wins
            assert f[:, t_last].argmax() < K - 1 or (f[:K - 1, t_last] < f[K - 1, t_last]).all()
    else:
        assert (t_all, t_last, t_one) == (None, None, None)
    if family == "extreme":
        assert npix < 255 or all((x == v).any() for v in ref.SPECIAL if v != 0) and (np.signbit(x) & (x == 0)).any()
    bad, nbad = ref.plant_invalid(lab, K)
    assert nbad == (5 if npix >= 16 else 0)
    wrong = (bad < 0) | (bad >= K)
    assert wrong.sum() == nbad and (nbad == 0 or sorted(bad[wrong].tolist()) == sorted([-1, K, 1000, -7, 2 ** 40]))
    assert not (set(np.flatnonzero(wrong.reshape(-1)).tolist()) & {t_all, t_last, t_one})
    sat = ref.saturated_pixels(x, bad)
    if family == "extreme" and npix >= 2047:
        assert sat.sum() >= 5
    assert not (sat & wrong).any()
    for gs, wt in ((1.0, None), (0.25, w)):
        loss, d, _, n = ref.softmax_ce(x, bad, wt, gs)
        assert n == nbad and np.isfinite(loss) and loss > 1e-2
        bound = ref.softmax_ce_grad_bound(x, wt, K, gs)
        assert bound.shape == (B, 1, H, W) and np.isfinite(bound).all() and (bound > 0).all()
        assert (bound >= (0.1 if wt is not None else 1.0) / npix * gs * (K + 12) * ref.EPS32).all()
        assert np.abs(d.transpose(0, 2, 3, 1)[sat]).max(initial=0.0) <= 2.0 ** -126


def test_head_bounds_helper_shapes():
    x, w, b, dl = torch.randn(2, 3, 5, 32), torch.randn(5, 32, 1, 1), torch.randn(5), torch.randn(2, 5, 3, 5)
    r = ref.head_reference_and_bounds(x, w, b, dl, 1, True)
    assert r["y"].shape == r["yb"].shape == (30, 5) and r["dz"].shape == r["dzb"].shape == (30, 32)
    assert r["dw"].shape == r["dwb"].shape == (5, 32) and r["db"].shape == r["dbb"].shape == (5,)
    assert all(v.dtype == torch.float64 for v in r.values()) and all((r[k] > 0).all() for k in ("yb", "dzb", "dwb", "dbb"))
    y = torch.einsum("bhwc,kc->bhwk", x.double(), w.double().reshape(5, 32)) + b.double()
    assert torch.allclose(r["y"], y.reshape(30, 5), rtol=1e-13, atol=1e-13)
