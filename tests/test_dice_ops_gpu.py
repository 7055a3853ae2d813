"""Per-op tests of dice.hip (unet_dice_step) through the C ABI against the fp64 reference and the derived bounds of
tests/dice_ref.py, at the shapes where the kernels change path: pixel counts per image either side of a block's 2048-pixel
quantum, images smaller than a wave, more partials per term than a finisher group has lanes, more terms than the finisher has
groups, every class padding, logits at which expf underflows.  Every pointer handed to the library comes from a guarded.Arena
(tests/guarded.py): scratch is exact to the byte, mem.verify(outputs...) after every call = every element written, every guard
intact; an output passed as NULL has a poisoned buffer beside it that must stay poison.  Inputs, shape and option lists and
bounds are dice_ref's, proved well-posed without a device by tests/test_dice_cpu.py."""
import numpy as np
import pytest
import torch

import dice_ref as dref
import guarded as gd
import multiclass_ref as ref
from gpu_support import hip, put, still_poison, strided
from test_multiclass_ops_gpu import ce_weight_forms

pytestmark = pytest.mark.gpu


class DiceCall:
    """One unet_dice_step call on Arena buffers; outputs not asked for are still allocated (and must stay poison)."""

    def __init__(self, hip, x, labels, warr, ws, o, want_dx=True, want_mask=True, want_dice=True, want_invalid=True, stream=None):
        L = hip.lib()
        B, K, H, W = x.shape
        T = 1 if o.batch else B
        self.mem = mem = gd.Arena()
        view, (xsB, xsC, xsH) = strided(mem, x)
        lab = put(mem, labels, "labels")
        wd = None if warr is None else put(mem, warr, "weight")
        self.loss = mem.out((3,), torch.float32, "losses")
        self.coeffs = mem.out((T, K), torch.float32, "dice")
        self.dx = mem.out((B, K, H, W), torch.float32, "dlogits")
        self.mask = mem.out((B, H, W), torch.int64, "mask")
        self.invalid = mem.out((1,), torch.int64, "invalid")
        nbytes = L.unet_dice_scratch_bytes(B, K, H, W)
        assert nbytes == dref.scratch_bytes(B, K, H, W)
        sc = mem.scratch(nbytes, "dice scratch")
        torch.cuda.synchronize()                                     # the buffers are ready whichever stream runs the call
        st = hip.stream() if stream is None else stream
        hip.check(L.unet_dice_step(view, xsB, xsC, xsH, K, mem.ptr(lab), mem.ptr(wd), ws[0], ws[1], ws[2], B, H, W, o.ce_weight,
                                   o.dice_weight, o.smooth, dref.flags_of(o), mem.ptr(self.loss), mem.ptr(self.coeffs) if want_dice else None,
                                   mem.ptr(self.dx) if want_dx else None, o.grad_scale, mem.ptr(self.mask) if want_mask else None,
                                   mem.ptr(self.invalid) if want_invalid else None, mem.ptr(sc), st), "unet_dice_step")
        torch.cuda.synchronize()
        mem.verify(self.loss, self.coeffs if want_dice else None, self.dx if want_dx else None, self.mask if want_mask else None,
                   self.invalid if want_invalid else None)
        assert want_dx or still_poison(self.dx)
        assert want_mask or still_poison(self.mask)
        assert want_dice or still_poison(self.coeffs)
        assert want_invalid or still_poison(self.invalid)

    def same(self, other, dx=True, mask=True, dice=True, invalid=True):
        return (torch.equal(self.loss, other.loss) and (not dx or torch.equal(self.dx, other.dx)) and (not mask or torch.equal(self.mask, other.mask))
                and (not dice or torch.equal(self.coeffs, other.coeffs)) and (not invalid or torch.equal(self.invalid, other.invalid)))


def reference(x, labels, wref, s, o, ce_cache):
    """(fp64 Result, Bounds) for options o; the CE term per weight is computed once per case."""
    key = id(wref)
    if key not in ce_cache:
        ce_cache[key] = ref.softmax_ce(x, labels, wref, 1.0)
    l_ce, d_ce, mask, bad = ce_cache[key]
    res = dref.Result(*dref.finish(s, (l_ce, d_ce), o), mask, bad)
    return res, dref.bounds(x, labels, wref, s, res, o)


def check(c, res, bnd, what):
    """The outputs of one call within the bounds; returns the error / bound ratios (total, ce, dice, coeffs, dlogits)."""
    loss, g = c.loss.cpu().numpy(), c.dx.cpu().numpy()
    assert np.isfinite(loss).all() and np.isfinite(g).all() and np.isfinite(c.coeffs.cpu().numpy()).all(), what
    ratios = dref.error_ratios((loss[0], loss[1], loss[2], c.coeffs.cpu().numpy(), g), res, bnd)
    return ratios


@pytest.mark.parametrize("family", dref.FAMILIES)
@pytest.mark.parametrize("shape,K", dref.CASES, ids=["%dx%dx%d-K%d" % (s + (K,)) for s, K in dref.CASES])
def test_dice_step_edge_shapes(hip, shape, K, family):
    """For the 48 option sets of dice_ref.OPTIONS (ce / dice weights (0, 1), (1, 1), (0.5, 2); both flags; smooth 1 and 1e-3;
    grad_scale 1 and 0.25; a dense weight map whenever the CE term counts): the three losses and dice_out within dice_ref.bounds,
    dlogits element-wise within its bound and exactly 0 on every plane of a pixel with an invalid label, everything finite,
    the mask bit-equal to the first maximum, the invalid count exact."""
    B, H, W = shape
    x, labels, w, nbad = dref.cases(B, K, H, W, family)
    s = dref.prepare(x, labels)
    mask_ref = ref.argmax_first(x)
    bad = ~s.ok
    worst = np.zeros(5)
    cache = {}
    for o in dref.OPTIONS:
        warr, ws, wref = (w, (H * W, W, 1), w) if o.ce_weight else (None, (0, 0, 0), None)
        res, bnd = reference(x, labels, wref, s, o, cache)
        c = DiceCall(hip, x, labels, warr, ws, o)
        ratios = check(c, res, bnd, o)
        worst = np.maximum(worst, ratios)
        assert max(ratios) <= 1.0, (o, ratios)
        assert np.all(c.dx.cpu().numpy().transpose(0, 2, 3, 1)[bad] == 0.0), o
        assert np.array_equal(c.mask.cpu().numpy(), mask_ref), o
        assert c.invalid.item() == nbad == res.invalid, o
    print("dice %s K=%d %s: worst err / bound total %.3g, ce %.3g, dice %.3g, coefficients %.3g, dlogits %.3g" % ((shape, K, family) + tuple(worst)))


@pytest.mark.parametrize("family", dref.FAMILIES)
@pytest.mark.parametrize("shape,K", [((3, 1, 2049), 5), ((300, 1, 7), 16), ((5, 3, 17), 9), ((1, 23, 89), 2)])
def test_dice_step_ce_alone_is_the_ce_step(hip, shape, K, family):
    """ce_weight 1, dice_weight 0: the CE part (and the total) within 1e-6 relative of multiclass_ref.softmax_ce, dlogits within
    softmax_ce_grad_bound, for the weight map and without one, both grad scales."""
    B, H, W = shape
    x, labels, w, nbad = dref.cases(B, K, H, W, family)
    for wt, gs in ((w, 1.0), (None, 0.25)):
        o = dref.Options(1.0, 0.0, 1.0, False, True, gs)
        loss_ref, d_ref, _, _ = ref.softmax_ce(x, labels, wt, gs)
        c = DiceCall(hip, x, labels, wt, (H * W, W, 1) if wt is not None else (0, 0, 0), o)
        loss, g = c.loss.cpu().numpy(), c.dx.cpu().numpy()
        assert np.isfinite(loss).all() and np.isfinite(g).all()
        el = abs(loss[1] - loss_ref) / abs(loss_ref)
        eg = float((np.abs(g - d_ref) / ref.softmax_ce_grad_bound(x, wt, K, gs)).max())
        print("dice (1, 0) %s K=%d %s: CE rel err %.3g, dlogits err / CE bound %.3g" % (shape, K, family, el, eg))
        assert el <= 1e-6 and abs(loss[0] - loss_ref) <= 1e-6 * abs(loss_ref) and eg <= 1.0
        assert c.invalid.item() == nbad


@pytest.mark.parametrize("shape,K,flags", [((3, 1, 2049), 5, (False, True)), ((300, 1, 7), 16, (True, False)), ((5, 3, 17), 9, (True, True))])
def test_dice_step_optional_outputs_repeats_and_streams(hip, shape, K, flags):
    """dlogits, mask, dice_out and invalid passed as NULL, one at a time: what is asked for is bit-identical to the full call,
    what is NULL stays poison (checked in DiceCall).  Two repeats and a call on a side stream are bit-identical too."""
    B, H, W = shape
    x, labels, w, nbad = dref.cases(B, K, H, W, "extreme")
    o = dref.Options(0.5, 2.0, dref.SMOOTH_SMALL, flags[0], flags[1], 0.25)
    ws = (H * W, W, 1)
    full = DiceCall(hip, x, labels, w, ws, o)
    assert full.invalid.item() == nbad
    for name in ("dx", "mask", "dice", "invalid"):
        c = DiceCall(hip, x, labels, w, ws, o, **{"want_" + name: False})
        assert c.same(full, **{name: False}), name
    for _ in range(2):
        assert DiceCall(hip, x, labels, w, ws, o).same(full)
    side = torch.cuda.Stream()
    assert DiceCall(hip, x, labels, w, ws, o, stream=side.cuda_stream).same(full)


def test_dice_step_weight_forms(hip):
    """The six weight forms of test_multiclass_ops_gpu.ce_weight_forms on one case (the CE term's weight), within the bounds."""
    B, K, H, W = 3, 5, 1, 2049
    x, labels, w, nbad = dref.cases(B, K, H, W, "tame")
    s = dref.prepare(x, labels)
    o = dref.Options(1.0, 1.0, 1.0, False, False, 0.25)
    for name, warr, ws, wref in ce_weight_forms(w):
        res, bnd = reference(x, labels, wref, s, o, {})
        c = DiceCall(hip, x, labels, warr, ws, o)
        ratios = check(c, res, bnd, name)
        print("dice weight form %s: err / bound %s" % (name, ["%.3g" % r for r in ratios]))
        assert max(ratios) <= 1.0, (name, ratios)


def test_dice_step_rejects_bad_arguments(hip):
    """smooth <= 0 or NaN, a negative weight, both weights 0, K outside 2..16 and unknown flags are refused; nothing is written."""
    L = hip.lib()
    B, K, H, W = 2, 3, 4, 5
    x, labels, w, _ = dref.cases(B, K, H, W, "tame")
    good = dict(K=K, cw=1.0, dw=1.0, smooth=1.0, flags=0)
    for bad in (dict(smooth=0.0), dict(smooth=-1.0), dict(smooth=float("nan")), dict(cw=-1.0), dict(dw=-0.5), dict(cw=0.0, dw=0.0),
                dict(K=1), dict(K=17), dict(flags=4)):
        a = dict(good, **bad)
        mem = gd.Arena()
        view, (xsB, xsC, xsH) = strided(mem, x)
        lab = put(mem, labels, "labels")
        outs = [mem.out((3,), torch.float32), mem.out((B, K), torch.float32), mem.out((B, K, H, W), torch.float32),
                mem.out((B, H, W), torch.int64), mem.out((1,), torch.int64)]
        sc = mem.scratch(L.unet_dice_scratch_bytes(B, K, H, W))
        rc = L.unet_dice_step(view, xsB, xsC, xsH, a["K"], mem.ptr(lab), None, 0, 0, 0, B, H, W, a["cw"], a["dw"], a["smooth"], a["flags"],
                              mem.ptr(outs[0]), mem.ptr(outs[1]), mem.ptr(outs[2]), 1.0, mem.ptr(outs[3]), mem.ptr(outs[4]), mem.ptr(sc),
                              hip.stream())
        assert rc != 0 and L.unet_last_error(), bad
        torch.cuda.synchronize()
        assert all(still_poison(t) for t in outs) and still_poison(sc), bad
        mem.verify()
