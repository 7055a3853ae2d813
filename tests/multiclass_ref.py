"""Plain numpy restatements of the K-class end of the net (Unet(n_classes=K)): the paper's softmax cross-entropy (eq. 1) and
its gradient, the K-way argmax, the per-image confusion counts and the K-class overlap-tile stitch.
tests/test_multiclass_cpu.py pins them to torch (F.cross_entropy, torch.argmax, torch.bincount) in fp64."""
import numpy as np

import segment_ref

EPS32 = 2.0 ** -24          # unit roundoff of fp32


def head_params(K, base=64, seed=0, head_seed=11):
    """The 46 state-dict tensors of a K-class net: oracle.prng.make_params(seed) with finalconv widened to K rows; rows 0 and 1
    are the binary net's, the others N(0, std of the binary rows), the extra biases U(-0.1, 0.1)."""
    from oracle import prng
    p = prng.make_params(seed, base=base)
    w2, b2 = p["finalconv.weight"], p["finalconv.bias"]
    rs = np.random.RandomState(head_seed)
    w = np.concatenate([w2, (rs.randn(K - 2, base, 1, 1) * w2.std()).astype(np.float32)])
    b = np.concatenate([b2, rs.uniform(-0.1, 0.1, K - 2).astype(np.float32)])
    p["finalconv.weight"], p["finalconv.bias"] = w, b
    return p


def argmax_first(logits):
    """[B,K,H,W] -> [B,H,W] int64, ties -> the lowest class index (what torch.argmax and numpy.argmax return)."""
    return np.argmax(np.asarray(logits), axis=1).astype(np.int64)


def softmax(logits):
    """fp64 softmax over axis 1, max-subtracted."""
    l = np.asarray(logits, np.float64)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def softmax_ce(logits, labels, weight=None, grad_scale=1.0):
    """eq. 1 in fp64: logits [B,K,H,W], int labels [B,H,W] (labels outside [0, K) add nothing and count as invalid), per-pixel
    weight broadcasting to [B,H,W] or None.  Returns (loss = sum over valid pixels of w * (logsumexp - l_label) / (B*H*W),
    dlogits [B,K,H,W] = w * (softmax - onehot) / (B*H*W) * grad_scale (0 at invalid pixels), mask, invalid count)."""
    l = np.asarray(logits, np.float64)
    B, K, H, W = l.shape
    lab = np.asarray(labels).reshape(B, H, W)
    ok = (lab >= 0) & (lab < K)
    w = np.ones((B, H, W)) if weight is None else np.broadcast_to(np.asarray(weight, np.float64), (B, H, W))
    m = l.max(axis=1)
    lse = m + np.log(np.exp(l - m[:, None]).sum(axis=1))
    safe = np.where(ok, lab, 0)
    ll = np.take_along_axis(l, safe[:, None], axis=1)[:, 0]
    n = B * H * W
    loss = float(np.where(ok, w * (lse - ll), 0.0).sum() / n)
    onehot = (np.arange(K)[None, :, None, None] == safe[:, None]).astype(np.float64)
    d = (w * ok)[:, None] * (softmax(l) - onehot) / n * grad_scale
    return loss, d, argmax_first(logits), int((~ok).sum())


def confusion(mask, labels, K):
    """Per-image K x K counts conf[b, i, j] = pixels labelled i predicted j (labels outside [0, K) in no bin), and the
    per-image invalid counts."""
    mask = np.asarray(mask).reshape(mask.shape[0], -1)
    lab = np.asarray(labels).reshape(mask.shape[0], -1)
    conf = np.zeros((mask.shape[0], K, K), np.int64)
    bad = np.zeros(mask.shape[0], np.int64)
    for b in range(mask.shape[0]):
        ok = (lab[b] >= 0) & (lab[b] < K)
        conf[b] = np.bincount(lab[b][ok] * K + mask[b][ok], minlength=K * K).reshape(K, K)
        bad[b] = int((~ok).sum())
    return conf, bad


def stitch_k(logits, B, H, W, S):
    """logits [B*ny*nx, K, So, So] -> (mask int64 [B,H,W], ties -> the lowest class; prob float64 [B,K,H,W] = softmax)."""
    logits = np.asarray(logits)
    K = logits.shape[1]
    mask = segment_ref.stitch_plane(argmax_first(logits), B, H, W, S)
    sm = softmax(logits)
    prob = np.stack([segment_ref.stitch_plane(sm[:, k], B, H, W, S) for k in range(K)], axis=1)
    return mask, prob


def softmax_bound(logits, K):
    """Bound on |p32 - p64| of the kernels' fp32 softmax p = exp(l - m) / sum exp(l - m): l - m is rounded once (relative
    EPS32, absolute <= R EPS32 with R = max |l - m|, so exp gains a relative R EPS32), expf adds <= 2 ulp, the K-term sum
    K EPS32 relative, the division 1 ulp: |p32 - p| <= (2 R + K + 8) EPS32 * p <= (2 R + K + 8) EPS32."""
    l = np.asarray(logits, np.float64)
    R = float((l.max(axis=1, keepdims=True) - l).max())
    return (2 * R + K + 8) * EPS32
