"""Step-side HIP kernels behind torch-shaped interfaces.

  bce_with_logits  — nn.BCEWithLogitsLoss(weight=w)(preds, ll) + backward   (trainer.py:63-77)
  argmax2          — preds.argmax(dim=1) for the 2-class head               (trainer.py:82, tester.py:30)
  SGD              — optim.SGD(lr, momentum).step()                          (trainer.py:30,78)
  Adam, AdamW      — torch.optim.Adam / AdamW (no amsgrad / maximize) by one multi-tensor HIP kernel (no counterpart in the reference)
  clip_grad_norm_  — nn.utils.clip_grad_norm_ on the device, without a host sync
  softmax_ce_step  — the paper's eq. 1 for K classes; dice_step — soft Dice, alone or added to it (no counterpart in the reference)
"""
import collections
import ctypes as C
import math

import torch

import _hip


class _LossFn(torch.autograd.Function):
    """The autograd shell of the loss ops: the forward's device pass has written dlogits already, so backward is dl * g for the
    logits (input 0) and None for every other input.  A forward saves dl unless the logits need no gradient (dl is then None)."""

    @staticmethod
    def backward(ctx, g, *_unused):
        (dl,) = ctx.saved_tensors
        return (dl * g,) + (None,) * (len(ctx.needs_input_grad) - 1)       # one entry per input of forward


def _step_inputs(ctx, logits, labels, want_mask, loss_shape=()):
    """What the label-driven steps share: logits [B,K,H,W] with unit last stride, labels as contiguous int64 [B,H,W] on their
    device, that device, and the outputs: loss (fp32, loss_shape), dl [B,K,H,W] (None unless the logits need a gradient) and
    mask int64 [B,H,W] (None unless wanted)."""
    B, K, H, W = logits.shape
    # (read before any copy: forward runs with grad mode off, so a contiguous() copy never requires grad)
    need_grad = ctx.needs_input_grad[0]
    if logits.stride(3) != 1:
        logits = logits.contiguous()
    dev = logits.device
    labels = labels.to(dev).reshape(B, H, W)
    if labels.dtype != torch.int64:
        labels = labels.long()
    loss = torch.empty(loss_shape, dtype=torch.float32, device=dev)
    dl = torch.empty(B, K, H, W, dtype=torch.float32, device=dev) if need_grad else None
    mask = torch.empty(B, H, W, dtype=torch.int64, device=dev) if want_mask else None
    return logits, labels.contiguous(), dev, loss, dl, mask


def _no_mask(dev):
    """What a forward returns in the mask's place when none was asked for (autograd wants a tensor)."""
    return torch.empty(0, dtype=torch.int64, device=dev)


def _broadcast_strides(weight, target, mismatch):
    """The element strides with which `weight`, right-aligned, broadcasts against the shape `target`: 0 on every axis along
    which it does not vary.  An axis that is neither 1 nor the target's raises mismatch(axis, size)."""
    pad = len(target) - weight.dim()
    shape = (1,) * pad + tuple(weight.shape)
    st = (0,) * pad + tuple(weight.stride())
    for d, n in enumerate(target):
        if shape[d] not in (n, 1):
            raise mismatch(d, shape[d])
    return [st[d] if shape[d] > 1 else 0 for d in range(len(target))]


def _weight_strides(weight, logits):
    """torch broadcasting of `weight` against [B,2,H,W] as four element strides (0 on broadcast axes); like the reference
    (trainer.py:72-75), a [B,H,W] map is right-aligned: its first axis meets the CLASS axis (quirk Q4), other sizes raise.
    No weight: (None, zeros)."""
    if weight is None:
        return None, (0, 0, 0, 0)
    weight = weight.to(logits.device, torch.float32).contiguous()
    return weight, _broadcast_strides(weight, logits.shape, lambda d, size: RuntimeError(
        "The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension %d" % (logits.shape[d], size, d)))


class _BCEFn(_LossFn):
    @staticmethod
    def forward(ctx, logits, target, weight, ws, grad_scale):
        B, two, H, W = logits.shape
        assert two == 2
        logits = logits.contiguous()
        target = target.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        dl = torch.empty_like(logits)
        sc = _hip.scratch("unet_bce", logits.device, logits.numel())
        _hip.run("unet_bce_logits", logits.device, _hip.ptr(logits), _hip.ptr(target), _hip.ptr(weight), ws[0], ws[1], ws[2], ws[3],
                 B, H, W, _hip.ptr(loss), _hip.ptr(dl), float(grad_scale), _hip.ptr(sc))
        ctx.save_for_backward(dl)
        return loss


class _BCEStepFn(_LossFn):
    """unet_bce_step: loss (+ its gradient) and the argmax mask from logits and integer labels in one device pass."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ws, grad_scale, want_mask):
        B, two, H, W = logits.shape
        assert two == 2
        logits, labels, dev, loss, dl, mask = _step_inputs(ctx, logits, labels, want_mask)
        sc = _hip.scratch("unet_bce_step", dev, B * H * W)
        _hip.run("unet_bce_step", dev, _hip.ptr(logits), logits.stride(0), logits.stride(1), logits.stride(2), _hip.ptr(labels),
                 _hip.ptr(weight), ws[0], ws[1], ws[2], ws[3], B, H, W, _hip.ptr(loss), _hip.ptr(dl), float(grad_scale), _hip.ptr(mask), _hip.ptr(sc))
        if dl is not None:
            ctx.save_for_backward(dl)
        if mask is None:
            return loss, _no_mask(dev)
        ctx.mark_non_differentiable(mask)
        return loss, mask


def bce_argmax_step(preds, labels, weight=None, grad_scale=1.0, want_mask=True):
    """Both halves of the step either side of the network in one kernel (trainer.py:60-82):
         loss = BCEWithLogitsLoss(weight)(preds, [1 - y, y])      mask = preds.argmax(dim=1)
    preds [B,2,H,W] (any view with unit last stride, e.g. the trainer's centre crop), labels int64 [B,1,H,W] or [B,H,W].
    Returns (loss, mask | None); loss.backward() feeds the gradient the same pass produced."""
    weight, wstrides = _weight_strides(weight, preds)
    loss, mask = _BCEStepFn.apply(preds, labels, weight, wstrides, grad_scale, want_mask)
    return loss, (mask if want_mask else None)


def bce_with_logits(logits, target, weight=None, grad_scale=1.0):
    """mean(weight * bce(logits, target)).  `weight` follows torch broadcasting against
    [B,2,H,W]: like the reference (trainer.py:72-75), a [B,H,W] map is right-aligned, i.e. its
    first axis meets the CLASS axis and must be 1 or 2 (quirk Q4) — other sizes raise."""
    weight, wstrides = _weight_strides(weight, logits)
    return _BCEFn.apply(logits, target, weight, wstrides, grad_scale)


def onehot2(labels, like):
    """ll[:,0] = 1 - y, ll[:,1] = y on the device (trainer.py:63-66)."""
    labels = labels.to(like.device).contiguous()
    B, _, H, W = like.shape
    out = torch.empty(B, 2, H, W, dtype=torch.float32, device=like.device)
    _hip.run("unet_onehot2", like.device, _hip.ptr(labels), _hip.ptr(out), B, H, W)
    return out


def argmax2(preds):
    """preds [B,2,H,W] (any view with unit last stride) -> int64 [B,H,W]; ties -> class 0."""
    B, two, H, W = preds.shape
    assert two == 2 and preds.stride(3) == 1
    out = torch.empty(B, H, W, dtype=torch.int64, device=preds.device)
    _hip.run("unet_argmax2", preds.device, _hip.ptr(preds), preds.stride(0), preds.stride(1), preds.stride(2), _hip.ptr(out), B, H, W)
    return out


class SGD(torch.optim.Optimizer):
    """optim.SGD(params, lr, momentum) with the update done by one multi-tensor HIP kernel per
    <=46 tensors.  No dampening / nesterov / weight decay (the reference uses none).  param_groups
    and state keep torch's shape so lr schedulers (ReduceLROnPlateau, trainer.py:31) work."""

    def __init__(self, params, lr=1e-4, momentum=0.99):
        super().__init__(params, dict(lr=lr, momentum=momentum))

    @torch.no_grad()
    def step(self, closure=None):
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            first = [p for p in ps if "momentum_buffer" not in self.state[p]]
            rest = [p for p in ps if "momentum_buffer" in self.state[p]]
            for batch, is_first in ((first, 1), (rest, 0)):
                for i in range(0, len(batch), _hip.N_PARAMS):
                    chunk = batch[i:i + _hip.N_PARAMS]
                    if is_first:
                        for p in chunk:
                            self.state[p]["momentum_buffer"] = torch.empty_like(p)
                    bufs = [self.state[p]["momentum_buffer"] for p in chunk]
                    grads = [p.grad.contiguous() for p in chunk]
                    numel = (C.c_size_t * len(chunk))(*[p.numel() for p in chunk])
                    _hip.run("unet_sgd_momentum", chunk[0].device, _hip.ptr_table(chunk), _hip.ptr_table(grads), _hip.ptr_table(bufs),
                             numel, len(chunk), float(group["lr"]), float(group["momentum"]), is_first)


def check_adam_options(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """Raises ValueError for hyper-parameters unet_adam_step does not take: lr < 0, a beta outside [0, 1), eps <= 0,
    weight_decay < 0 (non-finite values included).  No device is touched."""
    try:
        b1, b2 = betas
    except (TypeError, ValueError):
        raise ValueError("Adam: betas must be a pair (beta1, beta2), got %r" % (betas,))
    if not (float(lr) >= 0.0 and math.isfinite(float(lr))):
        raise ValueError("Adam: lr must be >= 0, got %r" % (lr,))
    for i, b in enumerate((b1, b2)):
        if not 0.0 <= float(b) < 1.0:
            raise ValueError("Adam: beta%d must lie in [0, 1), got %r" % (i + 1, b))
    if not (float(eps) > 0.0 and math.isfinite(float(eps))):
        raise ValueError("Adam: eps must be positive, got %r" % (eps,))
    if not (float(weight_decay) >= 0.0 and math.isfinite(float(weight_decay))):
        raise ValueError("Adam: weight_decay must be >= 0, got %r" % (weight_decay,))


def _numel_table(tensors):
    return (C.c_size_t * len(tensors))(*[t.numel() for t in tensors])


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) without amsgrad / maximize, the update done by one multi-tensor HIP
    kernel per <= 46 tensors (unet_adam_step; the statement order is in include/unet_hip.h).  decoupled=False adds weight_decay * p
    to the gradient (L2), decoupled=True shrinks p by lr * weight_decay before the update (AdamW).  param_groups and state keep
    torch's shape (state: step, a Python int, exp_avg, exp_avg_sq), so lr schedulers and checkpoint.py work unchanged.
    step(grad_scale=c), c a 1-element fp32 device tensor such as clip_grad_norm_(..., scale=False)'s coefficient, multiplies
    every gradient by c inside the same pass; the stored gradients are left as they are.  Parameters without a gradient are
    skipped; host tensors raise (there is no CPU fallback)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False):
        check_adam_options(lr, betas, eps, weight_decay)
        super().__init__(params, dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps, weight_decay=weight_decay,
                                      decoupled=bool(decoupled)))

    @torch.no_grad()
    def step(self, closure=None, *, grad_scale=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if grad_scale is not None and (grad_scale.numel() != 1 or grad_scale.dtype != torch.float32):
            raise ValueError("Adam.step: grad_scale must be a 1-element float32 device tensor, got %s %s"
                             % (tuple(grad_scale.shape), grad_scale.dtype))
        for group in self.param_groups:
            by_step = {}                                       # tensors that have taken the same number of updates share a launch
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "step" not in st:
                    _hip.ptr(p)                                 # a host tensor raises before any state is made
                    st["step"] = 0
                    st["exp_avg"] = torch.empty_like(p)         # written, never read, by the first update
                    st["exp_avg_sq"] = torch.empty_like(p)
                by_step.setdefault(int(st["step"]), []).append(p)
            b1, b2 = group["betas"]
            for done, ps in by_step.items():
                for i in range(0, len(ps), _hip.N_PARAMS):
                    chunk = ps[i:i + _hip.N_PARAMS]
                    grads = [p.grad.contiguous() for p in chunk]
                    _hip.run("unet_adam_step", chunk[0].device, _hip.ptr_table(chunk), _hip.ptr_table(grads),
                             _hip.ptr_table([self.state[p]["exp_avg"] for p in chunk]),
                             _hip.ptr_table([self.state[p]["exp_avg_sq"] for p in chunk]), _numel_table(chunk), len(chunk),
                             float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                             int(bool(group["decoupled"])), done + 1, _hip.ptr(grad_scale))
                    for p in chunk:
                        self.state[p]["step"] = done + 1
        return loss


class AdamW(Adam):
    """Adam with decoupled weight decay (Loshchilov & Hutter 2019): Adam(decoupled=True), weight_decay 1e-2 by default."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=True)


def clip_grad_norm_(parameters, max_norm, *, scale=True):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) (2-norm) on the device, without a host sync: one sum-of-squares
    launch per <= 46 gradients (fp64 partials in a fixed order, unet_grad_sumsq), one finishing workgroup, and with scale=True
    one launch per <= 46 gradients that multiplies them in place by the coefficient.  scale=False leaves the gradients alone:
    hand `coef` to Adam.step(grad_scale=coef), which saves that read-and-write pass.
    Returns (total_norm, coef), 0-dim fp32 device tensors (views of one [2] buffer): coef = min(1, max_norm / (total_norm + 1e-6)).
    Non-finite gradients are not treated specially: a NaN norm gives a NaN coefficient.  Parameters without a gradient are
    skipped; gradients must be contiguous fp32 device tensors."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError("clip_grad_norm_: max_norm must be positive, got %r" % max_norm)
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        raise ValueError("clip_grad_norm_: no parameter has a gradient")
    for g in grads:
        if g.dtype != torch.float32 or not g.is_contiguous():
            raise ValueError("clip_grad_norm_: gradients must be contiguous float32 tensors, got %s with strides %s" % (g.dtype, g.stride()))
    dev = grads[0].device
    L = _hip.lib()
    calls = []
    for i in range(0, len(grads), _hip.N_PARAMS):
        chunk = grads[i:i + _hip.N_PARAMS]
        numel = _numel_table(chunk)
        calls.append((_hip.ptr_table(chunk), numel, len(chunk), L.unet_grad_sumsq_partials(numel, len(chunk))))
    n_partials = sum(c[3] for c in calls)
    partials = torch.empty(n_partials, dtype=torch.float64, device=dev)
    out2 = torch.empty(2, dtype=torch.float32, device=dev)
    offset = 0
    for table, numel, n, count in calls:
        _hip.run("unet_grad_sumsq", dev, table, numel, n, _hip.ptr(partials), offset)
        offset += count
    _hip.run("unet_grad_norm_finish", dev, _hip.ptr(partials), n_partials, max_norm, _hip.ptr(out2))
    if scale:
        coef = _hip.ptr(out2[1:])
        for table, numel, n, _ in calls:
            _hip.run("unet_grads_scale", dev, table, numel, n, coef)
    return out2[0], out2[1]


def _crop_to_labels(preds, labels):
    """The centre crop of the two back ends below: `preds` [B,K,So,So] (unit last stride) is cropped to the labels' size n (So
    without labels).  Returns labels as contiguous [B,n,n] on preds' device (or None), the empty mask int64 [B,n,n], n and the pad."""
    B, So = preds.shape[0], preds.shape[2]
    assert preds.stride(3) == 1
    n = So
    if labels is not None:
        labels = labels.to(preds.device).reshape(B, labels.shape[-2], labels.shape[-1]).contiguous()
        n = labels.shape[-1]
    return labels, torch.empty(B, n, n, dtype=torch.int64, device=preds.device), n, int((So - n) / 2)


def crop_argmax_metrics(preds, labels=None):
    """Fused back end of the test/validation step (tester.py:29-42): centre-crop `preds` [B,2,So,So] to the
    label size, argmax over the two classes, and (with int64 labels [B,1,n,n] or [B,n,n]) count
    sum(pred&label), sum(pred|label), sum|pred-label| per image.  Returns (mask int64 [B,n,n], stats int64 [B,3] | None)."""
    B, two = preds.shape[:2]
    assert two == 2
    labels, mask, n, pad = _crop_to_labels(preds, labels)
    stats = torch.empty(B, 3, dtype=torch.int64, device=preds.device) if labels is not None else None
    _hip.run("unet_eval_masks", preds.device, _hip.ptr(preds), preds.stride(0), preds.stride(1), preds.stride(2), pad, _hip.ptr(labels),
             _hip.ptr(mask), B, n, _hip.ptr(stats))
    return mask, stats


# ---- K classes (Unet(n_classes=K)): the paper's loss, eq. 1 ------------------------------------------------------------------

def _pixel_weight_strides(weight, preds):
    """A per-pixel weight [B,H,W] / [H,W] / [1,H,W] (or anything that broadcasts to [B,H,W]) as three element strides
    (batch, row, column; 0 on broadcast axes).  Unlike the BCE path's right-alignment against [B,2,H,W] (quirk Q4), the map
    is aligned with the PIXELS: weight[b, y, x] multiplies pixel (b, y, x) of every class.  No weight: (None, zeros)."""
    if weight is None:
        return None, (0, 0, 0)
    B, _, H, W = preds.shape
    weight = weight.to(preds.device, torch.float32)
    if weight.dim() == 4 and weight.shape[1] == 1:
        weight = weight[:, 0]
    error = ValueError("softmax_ce_step: weight must broadcast to [B,H,W] = %s, got %s" % ((B, H, W), tuple(weight.shape)))
    if weight.dim() > 3:
        raise error
    return weight, _broadcast_strides(weight, (B, H, W), lambda d, size: error)


def _raise_invalid(name, invalid, K):
    """validate=True of the K-class steps: reads the kernel's count of labels outside [0, K) back (8 bytes, one host sync)."""
    n = int(invalid.item())
    if n:
        raise ValueError("%s: %d label(s) outside [0, %d)" % (name, n, K))


class _SoftmaxCEFn(_LossFn):
    """unet_softmax_ce_step: loss (+ its gradient), the argmax mask and the invalid-label count in one device pass."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ws, grad_scale, want_mask):
        B, K, H, W = logits.shape
        logits, labels, dev, loss, dl, mask = _step_inputs(ctx, logits, labels, want_mask)
        invalid = torch.empty((), dtype=torch.int64, device=dev)
        sc = _hip.scratch("unet_softmax_ce", dev, B * H * W)
        _hip.run("unet_softmax_ce_step", dev, _hip.ptr(logits), logits.stride(0), logits.stride(1), logits.stride(2), K,
                 _hip.ptr(labels), _hip.ptr(weight), ws[0], ws[1], ws[2], B, H, W, _hip.ptr(loss), _hip.ptr(dl), float(grad_scale),
                 _hip.ptr(mask), _hip.ptr(invalid), _hip.ptr(sc))
        if dl is not None:
            ctx.save_for_backward(dl)
        ctx.mark_non_differentiable(invalid)
        if mask is None:
            return loss, _no_mask(dev), invalid
        ctx.mark_non_differentiable(mask)
        return loss, mask, invalid


def softmax_ce_step(preds, labels, weight=None, grad_scale=1.0, want_mask=True, validate=True):
    """The paper's loss (Ronneberger et al. 2015, eq. 1), a pixel-wise soft-max over the K classes with a weighted
    cross-entropy, and the argmax mask, in one kernel (unet_softmax_ce_step):
         loss = mean over the B*H*W pixels of w * (logsumexp(preds) - preds[label])      mask = preds.argmax(dim=1)
    preds [B,K,H,W], K >= 2 (any view with unit last stride, e.g. the trainer's centre crop), labels integer [B,1,H,W] or
    [B,H,W] in [0, K).  weight: None, or a PER-PIXEL map that broadcasts to [B,H,W] (e.g. [B,H,W], or [H,W] for every
    sample) - NOT bce_argmax_step's right-alignment against the class axis (quirk Q4).  Labels outside [0, K) are never used
    as an index and add no loss and no gradient; the kernel counts them, and validate=True reads that count back (8 bytes,
    one host sync) and raises ValueError when it is not 0.  Returns (loss, mask | None); loss.backward() feeds the gradient
    the same pass produced (x grad_scale), as bce_argmax_step does."""
    if preds.dim() != 4 or preds.shape[1] < 2:
        raise ValueError("softmax_ce_step: expected preds [B,K,H,W] with K >= 2, got %s" % (tuple(preds.shape),))
    weight, wstrides = _pixel_weight_strides(weight, preds)
    loss, mask, invalid = _SoftmaxCEFn.apply(preds, labels, weight, wstrides, grad_scale, want_mask)
    if validate:
        _raise_invalid("softmax_ce_step", invalid, preds.shape[1])
    return loss, (mask if want_mask else None)


DICE_BATCH = 1                  # UNET_DICE_BATCH
DICE_SKIP_BACKGROUND = 2        # UNET_DICE_SKIP_BACKGROUND


class DiceParts(collections.namedtuple("DiceParts", "ce dice per_class")):
    """The parts of dice_step's loss: ce and dice are 0-d fp32 tensors (L_ce and L_dice, unweighted), per_class the soft Dice
    coefficients, fp32 [B,K] ([1,K] with batch=True), of every class whether it is counted in the mean or not."""


class _DiceFn(_LossFn):
    """unet_dice_step: the loss and its parts, the gradient, the argmax mask and the invalid-label count in one call."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ws, ce_weight, dice_weight, smooth, flags, grad_scale, want_mask):
        B, K, H, W = logits.shape
        logits, labels, dev, losses, dl, mask = _step_inputs(ctx, logits, labels, want_mask, loss_shape=(3,))
        coeffs = torch.empty(1 if flags & DICE_BATCH else B, K, dtype=torch.float32, device=dev)
        invalid = torch.empty((), dtype=torch.int64, device=dev)
        sc = _hip.scratch("unet_dice", dev, B, K, H, W)
        _hip.run("unet_dice_step", dev, _hip.ptr(logits), logits.stride(0), logits.stride(1), logits.stride(2), K, _hip.ptr(labels),
                 _hip.ptr(weight), ws[0], ws[1], ws[2], B, H, W, float(ce_weight), float(dice_weight), float(smooth), int(flags),
                 _hip.ptr(losses), _hip.ptr(coeffs), _hip.ptr(dl), float(grad_scale), _hip.ptr(mask), _hip.ptr(invalid), _hip.ptr(sc))
        if dl is not None:
            ctx.save_for_backward(dl)
        if mask is None:
            mask = _no_mask(dev)
        loss, ce, dice = losses[0], losses[1], losses[2]
        ctx.mark_non_differentiable(ce, dice, coeffs, mask, invalid)
        return loss, ce, dice, coeffs, mask, invalid


def dice_step(preds, labels, weight=None, *, ce_weight=0.0, dice_weight=1.0, smooth=1.0, batch=False, include_background=True,
              grad_scale=1.0, want_mask=True, validate=True, return_parts=False):
    """The soft Dice loss (Milletari et al. 2016) over the K-class soft-max, alone or added to the weighted cross-entropy of
    softmax_ce_step (nnU-Net's CE + Dice), with its gradient and the argmax mask, in one library call (unet_dice_step).  With
    p = softmax(preds) over the classes and v = the pixels whose label lies in [0, K):
         I[b,k] = sum_v p_k [y = k]     P[b,k] = sum_v p_k     Y[b,k] = sum_v [y = k]
         dice[b,k] = (2 I + smooth) / (P + Y + smooth)         L_dice = 1 - mean of dice over the (b,k) counted
         loss = ce_weight * L_ce + dice_weight * L_dice        L_ce = softmax_ce_step's loss, `weight` included
    batch=True sums I, P and Y over the batch before the ratio (nnU-Net's batch dice: one term per class);
    include_background=False leaves class 0 out of the mean.  smooth must be positive: it keeps 0 / 0 out of a class that is
    absent and unpredicted.  preds, labels, weight (a PER-PIXEL map; it multiplies the CE term only), grad_scale, want_mask and
    validate are softmax_ce_step's; labels outside [0, K) add nothing to any sum and no gradient.
    Returns (loss, mask | None), and with return_parts=True a third value DiceParts(ce, dice, per_class); loss.backward()
    feeds the gradient the same call produced (x grad_scale).  The result is bit-identical on every run and stream.
    Raises ValueError for smooth <= 0, a negative weight, both weights 0, and a weight map with ce_weight == 0 (it would be
    silently unused)."""
    if preds.dim() != 4 or preds.shape[1] < 2:
        raise ValueError("dice_step: expected preds [B,K,H,W] with K >= 2, got %s" % (tuple(preds.shape),))
    ce_weight, dice_weight, smooth = float(ce_weight), float(dice_weight), float(smooth)
    if not (smooth > 0.0 and math.isfinite(smooth)):
        raise ValueError("dice_step: smooth must be positive and finite, got %r" % smooth)
    if not (ce_weight >= 0.0 and dice_weight >= 0.0 and math.isfinite(ce_weight + dice_weight)):
        raise ValueError("dice_step: ce_weight and dice_weight must be >= 0, got %r and %r" % (ce_weight, dice_weight))
    if ce_weight == 0.0 and dice_weight == 0.0:
        raise ValueError("dice_step: ce_weight and dice_weight are both 0")
    if weight is not None and ce_weight == 0.0:
        raise ValueError("dice_step: a weight map multiplies the cross-entropy term only; with ce_weight = 0 it would be unused")
    weight, wstrides = _pixel_weight_strides(weight, preds)
    flags = (DICE_BATCH if batch else 0) | (0 if include_background else DICE_SKIP_BACKGROUND)
    loss, ce, dice, coeffs, mask, invalid = _DiceFn.apply(preds, labels, weight, wstrides, ce_weight, dice_weight, smooth, flags,
                                                          grad_scale, want_mask)
    if validate:
        _raise_invalid("dice_step", invalid, preds.shape[1])
    out = (loss, mask if want_mask else None)
    return out + (DiceParts(ce, dice, coeffs),) if return_parts else out


def argmaxk(preds):
    """preds [B,K,H,W] (any view with unit last stride), 2 <= K <= 16 -> int64 [B,H,W]; ties -> the lowest class (torch.argmax)."""
    B, K, H, W = preds.shape
    assert preds.stride(3) == 1
    out = torch.empty(B, H, W, dtype=torch.int64, device=preds.device)
    _hip.run("unet_argmaxk", preds.device, _hip.ptr(preds), preds.stride(0), preds.stride(1), preds.stride(2), K, _hip.ptr(out), B, H, W)
    return out


def crop_argmax_confusion(preds, labels=None, return_invalid=False):
    """The K-class counterpart of crop_argmax_metrics (same centre crop): argmax over the K classes and, with int64 labels
    [B,1,n,n] or [B,n,n], the per-image confusion counts conf[b, i, j] = pixels labelled i predicted j (unet_eval_confusion).
    Labels outside [0, K) fall in no bin; return_invalid=True also returns their per-image count.
    Returns (mask int64 [B,n,n], conf int64 [B,K,K] | None) (+ invalid int64 [B] | None)."""
    B, K = preds.shape[:2]
    labels, mask, n, pad = _crop_to_labels(preds, labels)
    conf = torch.empty(B, K, K, dtype=torch.int64, device=preds.device) if labels is not None else None
    invalid = torch.empty(B, dtype=torch.int64, device=preds.device) if labels is not None else None
    _hip.run("unet_eval_confusion", preds.device, _hip.ptr(preds), preds.stride(0), preds.stride(1), preds.stride(2), pad, K,
             _hip.ptr(labels), _hip.ptr(mask), B, n, _hip.ptr(conf), _hip.ptr(invalid))
    return (mask, conf, invalid) if return_invalid else (mask, conf)
