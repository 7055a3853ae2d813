"""The border weight map on the device (functions.weighted_map -> unet_weighted_map) against the reference's golden and
the numpy/scipy restatement tests/weighted_map_ref.py (pinned to that golden by tests/test_weighted_map_cpu.py), and the
trainer's loss_weights='border' option."""
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import weighted_map_ref as ref
from gpu_support import dev
from weighted_map_ref import check_against_restatement, golden_cases

pytestmark = pytest.mark.gpu


def test_weighted_map_matches_reference_golden(dev, golden_dir):
    import functions
    for name, lab, w_ref in golden_cases(golden_dir):
        w, n = functions.weighted_map(torch.from_numpy(lab).to(dev), return_objects=True)
        assert w.dtype == torch.float32 and w.shape == w_ref.shape and w.is_cuda
        w = w.cpu().numpy()
        assert np.all(np.abs(w - w_ref) <= 1e-5 * np.maximum(1.0, np.abs(w_ref))), name
        assert np.all(w[lab != 0] == 1.0), name
        assert [ndimage.label(l, ref.CROSS)[1] for l in lab] == n.cpu().tolist(), name


def random_labels(seed):
    """A seeded label batch: B 1-4, H != W included, 1 x 2 up to 516^2, discs (blobs) or speckle, int64 or float32."""
    rs = np.random.RandomState(1000 + seed)
    B = int(rs.randint(1, 5))
    sizes = [(1, 2), (2, 1), (3, 3), (1, 40), (17, 5), (64, 64), (37, 300), (300, 37), (129, 97), (256, 256), (516, 516),
             (200, 516), (516, 90)]
    H, W = sizes[seed % len(sizes)]
    speckle = seed % 3 == 1 and H * W <= 160 * 160
    lab = np.zeros((B, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        if speckle:
            lab[b] = rs.rand(H, W) < rs.uniform(0.2, 0.5)
        else:
            for _ in range(rs.randint(1, 25)):
                cy, cx, r = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(0.5, max(1.0, min(H, W) / 6))
                lab[b] |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        if lab[b].all():
            lab[b].flat[rs.randint(H * W)] = 0
        if not lab[b].any():
            lab[b].flat[rs.randint(H * W)] = 1
    return lab.astype(np.float32 if seed % 4 == 3 else np.int64)


@pytest.mark.parametrize("seed", range(30))
def test_weighted_map_random_shapes_vs_restatement(dev, seed):
    import functions
    lab = random_labels(seed)
    w, n = functions.weighted_map(torch.from_numpy(lab).to(dev), return_objects=True)
    check_against_restatement(lab, w.cpu().numpy(), n.cpu().numpy())


def test_weighted_map_errors(dev):
    import functions
    for lab in (torch.zeros(2, 8, 8, dtype=torch.int64), torch.ones(1, 5, 3)):
        with pytest.raises(IndexError):
            functions.weighted_map(lab.to(dev))
    mixed = torch.zeros(2, 8, 8, dtype=torch.int64)
    mixed[0, 3, 3] = 1                                     # image 1 has one class only
    with pytest.raises(IndexError):
        functions.weighted_map(mixed.to(dev))
    with pytest.raises(IndexError):
        functions.weighted_map(torch.ones(1, 1, 1, dtype=torch.int64, device=dev))
    with pytest.raises(NotImplementedError, match="device"):
        functions.weighted_map(torch.from_numpy(random_labels(4)))


def test_weighted_map_side_stream_and_repeats_bit_identical(dev):
    import functions
    rs = np.random.RandomState(5)
    lab = torch.from_numpy((rs.rand(2, 512, 512) < 0.35).astype(np.int64)).to(dev)
    w0, n0 = functions.weighted_map(lab, return_objects=True)
    assert n0.cpu().tolist() == [ndimage.label(l, ref.CROSS)[1] for l in lab.cpu().numpy()]
    assert min(n0.cpu().tolist()) > 10000
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        w1, n1 = functions.weighted_map(lab, return_objects=True)
    s.synchronize()
    assert torch.equal(w0, w1) and torch.equal(n0, n1)
    for _ in range(20):                                    # a racy union-find would change labels, counts or weights
        w, n = functions.weighted_map(lab, return_objects=True)
        assert torch.equal(w, w0) and torch.equal(n, n0)


def test_weighted_map_parameters(dev):
    """w0 and sig2 are arguments: w0 scales the border term, a wider sig2 reaches farther."""
    import functions
    lab = torch.from_numpy(random_labels(9)[:1]).to(dev)
    w = functions.weighted_map(lab).cpu().numpy()
    fg = lab.cpu().numpy() != 0
    w10 = functions.weighted_map(lab, w0=10).cpu().numpy()
    n1 = np.float32(fg.sum()); wcb = np.float32(np.trunc(n1 / np.float32(fg.size - fg.sum())))
    assert np.allclose(w10[~fg] - wcb, (w[~fg] - wcb) / 2, rtol=1e-5, atol=1e-6)
    wide = functions.weighted_map(lab, sig2=100).cpu().numpy()
    assert np.all(wide[~fg] >= w[~fg]) and (wide[~fg] > w[~fg]).any()


def test_trainer_border_loss_weights(dev, tmp_path):
    """training(..., loss_weights='border'): one epoch on a B = 2 batch from data.augment; loss.out is the fp64
    BCEWithLogitsLoss(weight=restated border map) of the initial-weight logits (Q4 broadcast, / len(loader) * batch)."""
    import data
    import network
    from oracle import aux_ref
    from trainer import training
    n = 196
    pairs = [aux_ref.cells(s, n) for s in (11, 12)]
    img = torch.from_numpy(np.stack([p[0] for p in pairs]).astype(np.float32)).to(dev)
    tgt = torch.from_numpy(np.stack([p[1] for p in pairs]).astype(np.float32)).to(dev)
    inp, gt = data.augment(img, tgt, [(0, 0), (0, 0)], n, [30.0, 0.0], 200.0, 10.0, random_state=np.random.RandomState(3))
    assert gt.shape == (2, 1, n, n) and gt.dtype == torch.int64
    batch = [(inp.contiguous(), gt.contiguous())]

    torch.manual_seed(0)
    net = network.Unet().to(dev)
    with torch.no_grad():
        logits = net(inp).detach().cpu().double()
    pad = (logits.shape[-1] - n) // 2
    logits = logits[:, :, pad:pad + n, pad:pad + n]
    lab = gt[:, 0].cpu().numpy()
    w_ref, _ = ref.weighted_map_batch(lab)
    y = torch.from_numpy(lab).double()
    target = torch.stack([1 - y, y], dim=1)
    expect = torch.nn.functional.binary_cross_entropy_with_logits(logits, target, weight=torch.from_numpy(w_ref).double()).item() / 2

    out_b = os.path.join(str(tmp_path), "border")
    training(net, batch, batch, 0, 2, dev, out_b, "DIC-C2DH-HeLa", loss_weights="border")
    got = float(np.loadtxt(os.path.join(out_b, "progress", "loss.out")))
    assert abs(got - expect) <= 1e-5 * abs(expect)

    torch.manual_seed(0)
    net = network.Unet().to(dev)
    out_d = os.path.join(str(tmp_path), "default")
    training(net, batch, batch, 0, 2, dev, out_d, "DIC-C2DH-HeLa")
    assert float(np.loadtxt(os.path.join(out_d, "progress", "loss.out"))) != got
    with pytest.raises(ValueError):
        training(net, batch, batch, 0, 2, dev, out_d, "DIC-C2DH-HeLa", loss_weights="unknown")
