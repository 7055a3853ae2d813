"""The Python surface of the soft Dice / CE + Dice step on the device: optim.dice_step (loss, parts, backward, argument checks)
against tests/dice_ref.py, trainer.training(loss='dice' | 'ce_dice') against a hand-written loop, and plain gradient descent."""
import copy

import numpy as np
import pytest
import torch

import dice_ref as dref
import multiclass_ref as ref
from gpu_support import dev
from test_multiclass_gpu import knet, tiny_loader

pytestmark = pytest.mark.gpu


def cropped(x, dev, pad=3):
    """x [B,K,H,W] as the centre crop of a larger NaN tensor on the device (a leaf that requires grad), and the crop."""
    B, K, H, W = x.shape
    big = torch.full((B, K, H + 2 * pad, W + 2 * pad), float("nan"))
    big[:, :, pad:pad + H, pad:pad + W] = torch.from_numpy(x)
    big = big.to(dev).requires_grad_(True)
    return big, big[:, :, pad:pad + H, pad:pad + W]


@pytest.mark.parametrize("K,batch,include_background,cw,dw", [(2, False, True, 0.0, 1.0), (3, True, False, 1.0, 1.0), (9, False, False, 0.5, 2.0),
                                                              (16, True, True, 1.0, 1.0)])
def test_dice_step_matches_reference_on_a_cropped_view(dev, K, batch, include_background, cw, dw):
    """Loss, parts, coefficients and the .backward() gradient (x an upstream factor of 3) within dice_ref.bounds; the gradient
    outside the crop is exactly 0; the mask is the first maximum."""
    import optim
    B, H, W = 3, 37, 61
    x, labels, w, _ = dref.cases(B, K, H, W, "tame")
    labels = np.where((labels < 0) | (labels >= K), 0, labels)          # validate=True: valid labels only
    wt = w if cw else None
    o = dref.Options(cw, dw, dref.SMOOTH_SMALL, batch, include_background, 0.25)
    res = dref.dice_loss(x, labels, wt, *o)
    bnd = dref.bounds(x, labels, wt, dref.prepare(x, labels), res, o)
    big, view = cropped(x, dev)
    loss, mask, parts = optim.dice_step(view, torch.from_numpy(labels)[:, None].to(dev), None if wt is None else torch.from_numpy(wt).to(dev),
                                        ce_weight=cw, dice_weight=dw, smooth=1e-3, batch=batch, include_background=include_background,
                                        grad_scale=0.25, return_parts=True)
    assert isinstance(parts, optim.DiceParts) and parts.per_class.shape == ((1, K) if batch else (B, K))
    (loss * 3.0).backward()
    g = big.grad.cpu().numpy()
    inner = g[:, :, 3:-3, 3:-3]
    ratios = dref.error_ratios((loss.item(), parts.ce.item(), parts.dice.item(), parts.per_class.cpu().numpy(), inner / 3.0), res, bnd)
    print("dice_step K=%d: err / bound %s" % (K, ["%.3g" % r for r in ratios]))
    assert max(ratios[:4]) <= 1.0
    assert float((np.abs(inner - 3.0 * res.dlogits) / (3.0 * bnd.dlogits + 2 * ref.EPS32 * np.abs(3.0 * res.dlogits))).max()) <= 1.0
    outer = g.copy()
    outer[:, :, 3:-3, 3:-3] = 0
    assert (outer == 0).all()
    assert np.array_equal(mask.cpu().numpy(), res.mask)
    two = optim.dice_step(view.detach(), torch.from_numpy(labels).to(dev), ce_weight=cw, dice_weight=dw, smooth=1e-3, batch=batch,
                          include_background=include_background, want_mask=False, weight=None if wt is None else torch.from_numpy(wt).to(dev))
    assert len(two) == 2 and two[1] is None and torch.equal(two[0], loss.detach())


def test_dice_step_value_errors(dev):
    import optim
    x = torch.zeros(2, 3, 4, 5, device=dev)
    y = torch.zeros(2, 4, 5, dtype=torch.int64, device=dev)
    w = torch.ones(2, 4, 5, device=dev)
    for kw in (dict(smooth=0.0), dict(smooth=-1.0), dict(ce_weight=-1.0), dict(dice_weight=-1.0), dict(ce_weight=0.0, dice_weight=0.0),
               dict(weight=w), dict(weight=w, ce_weight=0.0, dice_weight=2.0)):
        with pytest.raises(ValueError):
            optim.dice_step(x, y, **kw)
    with pytest.raises(ValueError):
        optim.dice_step(x[:, :1], y)
    y[1, 2, 3] = 3
    with pytest.raises(ValueError, match="1 label"):
        optim.dice_step(x, y)
    loss, _ = optim.dice_step(x, y, validate=False)
    assert torch.isfinite(loss)
    optim.dice_step(x, y.clamp(max=2), weight=w, ce_weight=1.0)


def hand_loop(net, train, val, B, dev, epochs, **kw):
    """The trainer's epochs written out over the public ops: forward, centre crop, dice_step, backward, optim.SGD."""
    import optim
    opt = optim.SGD(net.parameters(), lr=0.0001, momentum=0.99)
    losses, vlosses = [], []

    def step_loss(images, labels):
        preds = net(images.to(dev))
        n = labels.shape[-1]
        pad = (preds.shape[-1] - n) // 2
        return optim.dice_step(preds[:, :, pad:pad + n, pad:pad + n], labels.to(dev), want_mask=False, **kw)[0]

    for _ in range(epochs):
        tot = 0
        for images, labels in train:
            opt.zero_grad()
            loss = step_loss(images, labels)
            loss.backward()
            opt.step()
            tot += loss.detach()
        vt = 0
        with torch.no_grad():
            for images, labels in val:
                vt += step_loss(images, labels)
        losses.append((tot / (len(train) * B)).item())
        vlosses.append((vt / (len(val) * B)).item())
    return np.array(losses, np.float64), np.array(vlosses, np.float64)


@pytest.mark.parametrize("K,loss,options,kw", [
    (3, "ce_dice", None, dict(ce_weight=1.0, dice_weight=1.0)),
    (2, "dice", dict(smooth=1e-3, batch=True, include_background=False), dict(ce_weight=0.0, dice_weight=1.0, smooth=1e-3, batch=True,
                                                                              include_background=False))])
def test_training_dice_matches_hand_loop(dev, tmp_path, K, loss, options, kw):
    """training(loss='ce_dice', loss_weights='none') of a K = 3 net, and loss='dice' with dice_options of a K = 2 net, for 2
    epochs: the loss series equal, bit for bit, the hand-written loop; the six progress files are written."""
    import trainer
    S, B = 220, 2
    train, val = tiny_loader(1, 2, B, S, K), tiny_loader(2, 1, B, S, K)
    net = knet(K, dev)
    ref_net = copy.deepcopy(net)
    trainer.training(net, train, val, 1, B, dev, str(tmp_path), "synthetic", loss=loss, loss_weights="none", dice_options=options)
    losses, vlosses = hand_loop(ref_net, train, val, B, dev, 2, **kw)
    got = np.loadtxt(str(tmp_path / "progress" / "loss.out"))
    got_v = np.loadtxt(str(tmp_path / "progress" / "loss_val.out"))
    assert np.array_equal(got, losses) and np.array_equal(got_v, vlosses)
    assert np.isfinite(got).all() and (got > 0).all()
    for f in ("train_eval_iou.out", "train_eval_pe.out", "val_eval_iou.out", "val_eval_pe.out"):
        assert np.loadtxt(str(tmp_path / "progress" / f)).shape == (2,)


def test_gradient_descent_lowers_the_dice_loss(dev):
    """30 plain gradient steps of dice_step on free logits [2,3,16,16], at the step size at which the fp64 reference falls at
    every step (tests/test_dice_cpu.py): the device's Dice loss falls at every step too, and ends within 1e-4 of the reference's."""
    import optim
    x0, lab = dref.descent_start()
    x = torch.from_numpy(x0).to(dev).requires_grad_(True)
    y = torch.from_numpy(lab).to(dev)
    x64 = x0.astype(np.float64)
    losses = []
    for _ in range(dref.DESCENT_STEPS):
        loss, _ = optim.dice_step(x, y, want_mask=False)
        loss.backward()
        losses.append(loss.item())
        with torch.no_grad():
            x -= dref.DESCENT_LR * x.grad
            x.grad = None
        x64 = x64 - dref.DESCENT_LR * dref.dice_loss(x64, lab).dlogits
    last = optim.dice_step(x.detach(), y, want_mask=False)[0].item()
    losses.append(last)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert abs(last - dref.dice_loss(x64, lab).dice) <= 1e-4
