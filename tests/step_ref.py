"""fp64 references of the step-side kernels of loss.hip (bce_logits, bce_step, onehot2, argmax2) and direct.hip (sgd_momentum), shared by
tests/test_ops_gpu.py and tests/test_step_ops_gpu.py.  Imported like the other *_ref.py files."""
import ctypes as C

import numpy as np
import torch


def bce(x, z, w=None, grad_scale=1.0):
    """x, z [B,2,H,W], w broadcastable to x or None, all used as fp64.
    loss = mean(w * (max(x, 0) - x z + log1p(exp(-|x|)))) over all 2 B H W terms; grad = w (sigmoid(x) - z) / n * grad_scale."""
    x = np.asarray(x, np.float64); z = np.asarray(z, np.float64)
    w = np.ones_like(x) if w is None else np.broadcast_to(np.asarray(w, np.float64), x.shape)
    ex = np.exp(-np.abs(x))
    loss = float((w * (np.maximum(x, 0) - x * z + np.log1p(ex))).sum() / x.size)
    sg = np.where(x >= 0, 1 / (1 + ex), ex / (1 + ex))
    return loss, w * (sg - z) / x.size * float(grad_scale)


def onehot2(labels):
    """labels [B,H,W] -> [B,2,H,W]: plane 0 = 1 - y, plane 1 = y."""
    y = np.asarray(labels, np.float64)
    return np.stack([1 - y, y], axis=1)


def argmax2(x):
    """x [B,2,H,W] -> int64 [B,H,W]; the first maximum wins (class 0 on ties, +0.0 == -0.0 included)."""
    return np.argmax(np.asarray(x), axis=1).astype(np.int64)


# SGD momentum against the pinned C oracle in fp64 (oracle_c.sgd_momentum: buf = first ? g : mu*buf + g; p -= lr*buf).  The C ABI
# takes lr and mu as fp32, so the oracle is given those same fp32 values: what remains is the kernel's fp32 arithmetic, fused or
# not.  Per step (elementwise; step 1 is exact: buf = g):
#   buf: mu*buf and + g round once each, <= 2^-24 (mu|buf| + |mu buf + g|) <= 2^-23 (mu|buf| + |g|), plus mu x the error carried in;
#   p:   lr*buf and p - lr*buf round once each, <= 2^-24 lr|buf| + 2^-24 |p|, plus lr x the buffer's error
# (tb, tp below; the lr*buf term is counted as 2^-22 lr|buf|, with room to spare).
def sgd_vs_oracle(hip, ps, nsteps=2, lr=1e-4, mu=0.99, bufs=None, make_grad=None, ptrs=None, after_call=None):
    """ps: the parameter tensors on the device, updated in place.  bufs: the momentum buffers (default: zeros; their contents
    before the first step must not matter).  make_grad(p) -> gradient tensor (default torch.randn_like).  ptrs(tensors) -> the
    void*[] handed to the library (default hip.ptr_table).  after_call(step, gs, bufs) runs after every library call.
    Returns (gs of the last step, bufs)."""
    from oracle import oracle_c
    L = hip.lib()
    ptrs = ptrs or hip.ptr_table
    make_grad = make_grad or torch.randn_like
    lr, mu = float(np.float32(lr)), float(np.float32(mu))       # what the kernel computes with
    p64 = [p.double().cpu().numpy().copy() for p in ps]
    b64 = [np.zeros_like(q) for q in p64]
    if bufs is None:
        bufs = [torch.zeros_like(p) for p in ps]
    numel = (C.c_size_t * len(ps))(*[p.numel() for p in ps])
    tol_p = [np.zeros_like(q) for q in p64]; tol_b = [np.zeros_like(q) for q in p64]
    gs = None
    for step in range(nsteps):
        gs = [make_grad(p) for p in ps]
        for q, b_, g_, tp, tb in zip(p64, b64, gs, tol_p, tol_b):
            prev = np.abs(b_).copy()
            g64 = g_.double().cpu().numpy()
            oracle_c.sgd_momentum(q, g64, b_, lr, mu, int(step == 0))
            tb[:] = 0.0 if step == 0 else 2.0 ** -23 * (mu * prev + np.abs(g64)) + mu * tb
            tp += 2.0 ** -24 * np.abs(q) + 2.0 ** -22 * lr * np.abs(b_) + lr * tb
        hip.check(L.unet_sgd_momentum(ptrs(ps), ptrs(gs), ptrs(bufs), numel, len(ps), lr, mu, int(step == 0), hip.stream()))
        if after_call is not None:
            after_call(step, gs, bufs)
    for p, q, bd, b_, tp, tb in zip(ps, p64, bufs, b64, tol_p, tol_b):
        assert np.all(np.abs(p.double().cpu().numpy() - q) <= tp)
        assert np.all(np.abs(bd.double().cpu().numpy() - b_) <= tb)
    return gs, bufs
