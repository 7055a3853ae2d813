"""Plain numpy restatements of the K-class end of the net (Unet(n_classes=K)): the paper's softmax cross-entropy (eq. 1) and
its gradient, the K-way argmax, the per-image confusion counts and the K-class overlap-tile stitch.
tests/test_multiclass_cpu.py pins them to torch (F.cross_entropy, torch.argmax, torch.bincount) in fp64.
Also the seeded inputs, the shape lists and the error bounds that tests/test_multiclass_ops_gpu.py holds the K-class
kernels of loss.hip and multiclass.hip to; tests/test_multiclass_cpu.py proves those inputs well-posed without a device."""
import math


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


# ---- inputs, shapes and bounds of the per-op tests (tests/test_multiclass_ops_gpu.py) ---------------------------------------
# logits at which expf(l - m) underflows, the gradient saturates and m - l_label reaches 2e4 (test_step_ops_gpu.py's list)
SPECIAL = np.float32([0.0, -0.0, 1e-8, -1e-8, 17, -17, 88, -88, 104, -104, 1e4, -1e4])
SATURATION = 104.0          # e^-104 < 2^-150: expf(l - m) is 0 in fp32, and below 1e-45 in fp64, once l <= m - 104

ALL_K = (2, 3, 4, 5, 8, 9, 16)      # KP = 4 (2, 3, 4), KP = 8 padded and full (5, 8), KP = 16 padded and full (9, 16)
# pixel counts 1, 2047, 2048, 2049 (either side of the 2048 pixels of a block), 2100 with H W = 7 < 256 (a thread's next
# pixel lies 36 images on), 255 (one partly filled block); then 257 blocks: the finisher's second trip over the partials
CE_SMALL_SHAPES = [(1, 1, 1), (1, 23, 89), (2, 16, 64), (3, 1, 683), (300, 1, 7), (5, 3, 17)]
CE_LARGE_SHAPE = (2, 513, 512)
CE_SHAPES = CE_SMALL_SHAPES + [CE_LARGE_SHAPE]
# every K at three small shapes, every small shape at three or four K; K = 3 alone at the large one
CE_CASES = [(s, K) for i, s in enumerate(CE_SMALL_SHAPES) for j, K in enumerate(ALL_K) if (i + j) % 2 == 0] + [(CE_LARGE_SHAPE, 3)]
CE_FAMILIES = ("tame", "extreme")
INVALID_LABELS = (-1, None, 1000, -7, 2 ** 40)      # None stands for K, the first label past the range


def tie_pixels(npix):
    """Flat pixel indices (over B H W) of the planted ties: (every class tied, maximum = last class, maximum = class 1);
    None where the shape has no room."""
    if npix < 3:
        return (None, None, None)
    return (0, npix - 1, npix // 2)


def ce_cases(B, K, H, W, family):
    """(logits float32 [B,K,H,W], labels int64 [B,H,W] in [0, K), weight float32 [B,H,W] in [0.1, 4]).
    'tame': randn x 2.  'extreme': the same with 30 % of the elements drawn from SPECIAL.  Ties are planted last, so they
    survive: every class tied at the first pixel, the maximum tied with the last class at the last pixel, the maximum tied
    with class 1 at the middle one."""
    assert family in CE_FAMILIES
    rs = np.random.RandomState((B * 7919 + H * 104729 + W * 31 + K * 1009 + CE_FAMILIES.index(family)) % (2 ** 31))
    x = (rs.randn(B, K, H, W) * 2).astype(np.float32)
    if family == "extreme":
        pick = rs.rand(B, K, H, W) < 0.3
        x[pick] = rs.choice(SPECIAL, int(pick.sum()))
    labels = rs.randint(0, K, (B, H, W)).astype(np.int64)
    weight = rs.uniform(0.1, 4.0, (B, H, W)).astype(np.float32)
    f = np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(K, -1)             # [K, npix]
    t_all, t_last, t_one = tie_pixels(B * H * W)
    if t_all is not None:
        f[:, t_all] = f[0, t_all]
        f[K - 1, t_last] = f[:, t_last].max()
        f[1, t_one] = f[:, t_one].max()
    x = np.ascontiguousarray(f.reshape(K, B, H, W).transpose(1, 0, 2, 3))
    return x, labels, weight


def plant_invalid(labels, K):
    """A copy of labels with INVALID_LABELS at flat pixels 3..7 (clear of the planted ties) where the shape has 16 pixels or
    more, and how many were planted."""
    lab = labels.copy()
    if lab.size < 16:
        return lab, 0
    bad = [K if v is None else v for v in INVALID_LABELS]
    lab.reshape(-1)[3:3 + len(bad)] = bad
    return lab, len(bad)


def saturated_pixels(logits, labels):
    """[B,H,W] bool: the label is the maximum and every other logit is <= m - 104.  There the kernel's every other
    expf(l - m) is 0, the sum is exactly 1 and p - onehot is exactly 0 on every class plane."""
    l = np.asarray(logits, np.float64)
    B, K, H, W = l.shape
    lab = np.asarray(labels).reshape(B, H, W)
    ok = (lab >= 0) & (lab < K)
    safe = np.where(ok, lab, 0)
    ll = np.take_along_axis(l, safe[:, None], axis=1)[:, 0]
    others = np.where(np.arange(K)[None, :, None, None] == safe[:, None], -np.inf, l).max(axis=1)
    return ok & (others <= ll - SATURATION)


def softmax_ce_grad_bound(logits, weight, K, grad_scale):
    """Per-element bound [B,K,H,W] (broadcast over K) on |dlogits32 - dlogits64| of unet_softmax_ce_step:
    (w / n) |grad_scale| (2 R_px + K + 12) EPS32 + 2^-126, R_px = min(max_k (m - l_k), 104) per pixel: softmax_bound's
    (2 R + K + 8) EPS32 on p, plus the roundings of w / n x grad_scale and of p - onehot.  Beyond l - m = -104 fp32 and fp64
    both give 0 to within 1e-45, hence the cap; 2^-126 covers a result that is flushed to zero as a subnormal."""
    l = np.asarray(logits, np.float64)
    B, _, H, W = l.shape
    n = B * H * W
    R = np.minimum((l.max(axis=1, keepdims=True) - l).max(axis=1, keepdims=True), SATURATION)
    w = np.ones((B, 1, H, W)) if weight is None else np.broadcast_to(np.asarray(weight, np.float64), (B, H, W))[:, None]
    return w / n * abs(grad_scale) * (2 * R + K + 12) * EPS32 + 2.0 ** -126


def head_reference_and_bounds(x, w, b, dl, nb, bf16):
    """fp64 results and per-element bounds of unet_head1xk_fwd / _bwd.  x [B,H,W,C], w [K,C,1,1], b [K], dl [B,K,H,W]: torch
    fp32 tensors holding the values the kernels read (exact bf16 values for bf16 activations); nb = the backward's blocks
    (scratch bytes / (K C + K) floats); bf16: dz is stored as bf16.  Returns pixel-major fp64 tensors: y, yb [n,K]; dz, dzb
    [n,C]; dw, dwb [K,C]; db, dbb [K].  EPS = 2^-24:
      forward  y = sum_c x_c w_c + b: 4-term dot products per lane, then a log2(C/4)-deep pairwise tree, then + b:
               |y - y64| <= (log2(C) + 3) EPS (sum_c |x_c w_c| + |b|);
      dz       = (sum_k dl_k w_k) [x > 0], an fma chain of K terms: <= (K + 1) EPS sum_k |dl_k w_k|, plus, for bf16 dz, the
               final rounding to 8 significant bits, half an ulp: <= 2^-8 |dz|;
      dw, db   per lane a serial fma chain over its pixels (head1x1: n / (blocks x pixels per pass); K > 2: 512-pixel chunks per
               block x passes per chunk), then a shuffle tree over the wave (<= 3), the 4 waves (3), and the cross-block
               reduce (nb / 64 + 6): <= (chain + nb/64 + 12) EPS sum_m |dl_k x_c|."""
    B, H, W, C_ = x.shape
    K = w.shape[0]
    n = B * H * W
    x64 = x.double().reshape(n, C_)
    w64 = w.double().reshape(K, C_)
    dl64 = dl.double().permute(0, 2, 3, 1).reshape(n, K)
    y64 = x64 @ w64.T + b.double()
    yb = (math.log2(C_) + 3) * EPS32 * ((x64.abs() @ w64.abs().T) + b.double().abs())
    dz64 = (dl64 @ w64) * (x64 > 0)
    dzb = (K + 1) * EPS32 * (dl64.abs() @ w64.abs())
    if bf16:
        dzb = dzb + 2.0 ** -8 * dz64.abs()
    ppp = 256 // (C_ // 4)                                   # pixels per pass of a block
    chain = max(-(-n // (nb * ppp)), -(-(-(-n // 512)) // nb) * (512 // ppp)) + nb / 64 + 12
    dw64 = dl64.T @ x64
    dwb = chain * EPS32 * (dl64.abs().T @ x64.abs())
    db64 = dl64.sum(0)
    dbb = chain * EPS32 * dl64.abs().sum(0)
    return dict(y=y64, yb=yb, dz=dz64, dzb=dzb, dw=dw64, dwb=dwb, db=db64, dbb=dbb)
