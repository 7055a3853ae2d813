"""fp64 numpy restatement of unet_dice_step (dice.hip; optim.dice_step): the soft Dice loss over the K-class soft-max, alone
or added to the weighted cross-entropy of multiclass_ref.softmax_ce, with its gradient; tests/test_dice_cpu.py pins it to
torch.autograd in fp64.  Also the seeded inputs, the shape and option lists and the DERIVED error bounds that
tests/test_dice_ops_gpu.py holds the kernels to, and an fp32 emulation of the kernels' arithmetic with which
tests/test_dice_cpu.py proves, without a device, that the bounds are positive, finite and not violated by that arithmetic.

The kernels' quanta (dice.hip's named constants, restated): a workgroup of the sums and gradient kernels covers
PX_PER_BLOCK = 2048 pixels of ONE image, a thread PX_PER_THREAD = 8 of them, which it sums in fp32 before widening to double;
the finisher is one workgroup of FIN_GROUPS = 16 groups of FIN_GROUP = 16 lanes, a group per (image, class) term - per class
with batch=True - whose lanes stride that term's per-block partials.

The shape list is test_multiclass_ops_gpu's, adjusted to these constants: the quantum is per image, so 2048 pixels per image
is (2, 32, 64) and one pixel past it (3, 1, 2049); a group has 16 lanes, not the CE finisher's 256 threads, so its second
trip over the partials starts at 17 blocks per image: (1, 33, 1024) = 33 792 pixels = 16.5 blocks stands where the issue's
(1, 514, 1024) stood for a 256-thread finisher.  With batch=True a group strides the B x blocks partials of its class:
(300, 1, 7) is 300 of them, 19 trips.  16 groups: more than 16 terms (every shape with B K > 16) is the groups' second round."""
import collections
import itertools

import numpy as np

import multiclass_ref as ref

EPS32 = ref.EPS32
PX_PER_BLOCK = 2048
THREADS = 256
PX_PER_THREAD = PX_PER_BLOCK // THREADS
FIN_GROUP = 16
FIN_GROUPS = 16
BATCH, SKIP_BACKGROUND = 1, 2           # UNET_DICE_BATCH, UNET_DICE_SKIP_BACKGROUND

# c1 of beta_px = (2 min(R_px, 104) + K + C1) EPS32, the relative error of one fp32 soft-max value AS IT ENTERS A SUM:
# multiclass_ref.softmax_bound's 8 (l - m rounded once, expf <= 2 ulp, the K-term sum, and for the division one correctly
# rounded reciprocal + one multiply = 2 EPS32, which its 8 already has room for: 4 + 2 <= 8), plus PX_PER_THREAD = 8 for the up
# to 7 fp32 additions of a thread's pixels (each <= EPS32 relative to a sum of positive terms) with one to spare.
C1 = 8 + PX_PER_THREAD
# c2 of the gradient: the roundings of p_j ((C_j - A_j [y = j]) - S), S = fma chain of K products C_k p_k and one more for
# - A_y p_y: K + 1 in S; the subtraction C_j - A_j, the subtraction of S, the product with p_j: 3; the table's two entries
# are rounded to fp32 once each: 2.  Every intermediate is <= 2 max|g| in size except A_y and C_j - A_j (<= 2 |g_y| <= 2 max|g|,
# since |g_y| >= a_y / 2), which the factor 2 max|g| of the bound already carries; the K of (K + C2) pays for the chain, C2 = 12
# for the 1 + 3 + 2 = 6 others counted twice.
C2 = 12
TINY = 2.0 ** -126                      # a subnormal result may be flushed: absolute slack per pixel / per element

Options = collections.namedtuple("Options", "ce_weight dice_weight smooth batch include_background grad_scale")
Result = collections.namedtuple("Result", "total ce dice coeffs dlogits mask invalid")
Bounds = collections.namedtuple("Bounds", "total ce dice coeffs dlogits")
Sums = collections.namedtuple("Sums", "p ok onehot I P Y")      # p [B,K,H,W]; ok [B,H,W]; onehot [B,K,H,W]; I, P, Y [B,K]

WEIGHTS = ((0.0, 1.0), (1.0, 1.0), (0.5, 2.0))
# smooth crosses the C ABI as a float: the reference is given the value the kernel receives, 1e-3 rounded to fp32 (4.7e-8 off;
# with the double 1e-3 a coefficient N / D with N << D moves by 0.8 EPS32 of itself, as much as its own final rounding).  The
# weights and grad scales of the lists are exact in fp32.
SMOOTH_SMALL = float(np.float32(1e-3))
OPTIONS = [Options(cw, dw, s, b, bg, gs) for (cw, dw), b, bg, s, gs in
           itertools.product(WEIGHTS, (False, True), (True, False), (1.0, SMOOTH_SMALL), (1.0, 0.25))]

SMALL_SHAPES = [(1, 1, 1), (1, 23, 89), (2, 32, 64), (3, 1, 2049), (300, 1, 7), (5, 3, 17)]
LARGE_SHAPE = (1, 33, 1024)
SHAPES = SMALL_SHAPES + [LARGE_SHAPE]
# every K at three small shapes, every small shape at three or four K; K = 3 alone at the large one
CASES = [(s, K) for i, s in enumerate(SMALL_SHAPES) for j, K in enumerate(ref.ALL_K) if (i + j) % 2 == 0] + [(LARGE_SHAPE, 3)]
FAMILIES = ref.CE_FAMILIES


def flags_of(o):
    return (BATCH if o.batch else 0) | (0 if o.include_background else SKIP_BACKGROUND)


def blocks_per_image(H, W):
    return -(-(H * W) // PX_PER_BLOCK)


def scratch_bytes(B, K, H, W):
    """unet_dice_scratch_bytes: per block a double and a 64-bit count, per block and class two doubles and a 32-bit count; the
    coefficient table, two floats per (image, class); 0 for an empty shape."""
    if min(B, K, H, W) <= 0:
        return 0
    return B * blocks_per_image(H, W) * (16 + 20 * K) + 8 * B * K


def cases(B, K, H, W, family):
    """multiclass_ref.ce_cases, with class K - 1 taken out of image 0's labels (relabelled 0: absent from at least one image, so
    `smooth` matters there; a one-pixel image lacks K - 1 classes as it is and keeps its label, and with it a cross-entropy of
    ordinary size), then multiclass_ref.plant_invalid.  Returns (logits, labels, weight, invalid labels planted)."""
    x, labels, w = ref.ce_cases(B, K, H, W, family)
    labels = labels.copy()
    if H * W > 1:
        labels[0][labels[0] == K - 1] = 0
    labels, nbad = ref.plant_invalid(labels, K)
    return x, labels, w, nbad


def _sum_bk(a):
    return a.reshape(a.shape[0], a.shape[1], -1).sum(axis=2)


def prepare(logits, labels):
    """The fp64 soft-max and the exact per-image sums."""
    l = np.asarray(logits, np.float64)
    B, K, H, W = l.shape
    lab = np.asarray(labels).reshape(B, H, W)
    ok = (lab >= 0) & (lab < K)
    onehot = ((np.arange(K)[None, :, None, None] == lab[:, None]) & ok[:, None]).astype(np.float64)
    p = ref.softmax(l)
    pv = p * ok[:, None]
    return Sums(p, ok, onehot, _sum_bk(pv * onehot), _sum_bk(pv), _sum_bk(onehot))


def prepare32(logits, labels):
    """The same with the kernels' fp32 arithmetic and summation order: p = expf(l - m) x (1 / sum), the sum serial over the
    classes; a thread's 8 pixels (256 apart inside a 2048-pixel block of one image) added in fp32, everything after in double."""
    f = np.float32
    l = np.asarray(logits, f)
    B, K, H, W = l.shape
    lab = np.asarray(labels).reshape(B, H, W)
    ok = (lab >= 0) & (lab < K)
    onehot = ((np.arange(K)[None, :, None, None] == lab[:, None]) & ok[:, None])
    ex = np.exp((l - l.max(axis=1, keepdims=True)).astype(f)).astype(f)
    se = np.zeros((B, 1, H, W), f)
    for k in range(K):
        se = (se + ex[:, k:k + 1]).astype(f)
    p = (ex * (f(1.0) / se).astype(f)).astype(f)
    nbx = blocks_per_image(H, W)

    def thread_sums(v):                                          # [B,K,H,W] fp32 -> [B,K] double
        pad = np.zeros((B, K, nbx * PX_PER_BLOCK), f)
        pad[:, :, :H * W] = v.reshape(B, K, -1)
        pad = pad.reshape(B, K, nbx, PX_PER_THREAD, THREADS)
        s = np.zeros((B, K, nbx, THREADS), f)
        for j in range(PX_PER_THREAD):
            s = (s + pad[:, :, :, j]).astype(f)
        return s.astype(np.float64).reshape(B, K, -1).sum(axis=2)

    pv = (p * ok[:, None]).astype(f)
    return Sums(p, ok, onehot.astype(np.float64), thread_sums((pv * onehot).astype(f)), thread_sums(pv), _sum_bk(onehot.astype(np.float64)))


def _terms(s, o):
    """(I, P, Y) [T,K] with T = 1 (batch) or B, the counted-class mask [K] and the number of terms."""
    I, P, Y = (s.I, s.P, s.Y) if not o.batch else tuple(a.sum(axis=0, keepdims=True) for a in (s.I, s.P, s.Y))
    K = I.shape[1]
    counted = np.arange(K) >= (0 if o.include_background else 1)
    return I, P, Y, counted, I.shape[0] * int(counted.sum())


def finish(s, ce, o, f32=False):
    """Losses, coefficients and dlogits from the sums `s` and ce = (L_ce, dL_ce / dlogits at grad_scale 1).  f32: the table and
    the gradient arithmetic in fp32, as the kernels do them (the emulation)."""
    I, P, Y, counted, n_terms = _terms(s, o)
    D = P + Y + o.smooth
    N = 2.0 * I + o.smooth
    coeffs = N / D
    l_dice = 1.0 - float((coeffs * counted).sum() / n_terms)
    l_ce, d_ce = ce
    total = o.ce_weight * l_ce + o.dice_weight * l_dice
    sc = o.grad_scale * o.dice_weight / n_terms
    A, C = sc * 2.0 / D * counted, sc * N / (D * D) * counted    # [T,K]
    ft = np.float32 if f32 else np.float64
    A, C = A.astype(ft)[:, :, None, None], C.astype(ft)[:, :, None, None]
    p, oh = s.p.astype(ft), s.onehot.astype(ft)
    S = np.zeros(p[:, :1].shape, ft)
    for k in range(p.shape[1]):
        S = (S + C[:, k:k + 1] * p[:, k:k + 1]).astype(ft)
    S = (S - (A * oh * p).sum(axis=1, keepdims=True).astype(ft)).astype(ft)
    g = (C - (A * oh).astype(ft)).astype(ft)
    d_dice = (p * (g - S).astype(ft)).astype(ft) * s.ok[:, None]
    if f32:
        d = ((o.ce_weight * o.grad_scale * d_ce).astype(ft) + d_dice).astype(ft)
    else:
        d = o.ce_weight * o.grad_scale * d_ce + d_dice
    return total, l_ce, l_dice, coeffs, np.asarray(d, np.float64)


def dice_loss(logits, labels, weight=None, ce_weight=0.0, dice_weight=1.0, smooth=1.0, batch=False, include_background=True,
              grad_scale=1.0):
    """fp64: logits [B,K,H,W], int labels [B,H,W] (labels outside [0, K) add nothing to any sum and no gradient, and count as
    invalid), per-pixel weight (the CE term's only) or None.  With v = the valid pixels and p = softmax(logits):
        I = sum_v p_k [y = k], P = sum_v p_k, Y = sum_v [y = k] per (image, class), over the batch too with batch=True
        dice = (2 I + s) / (P + Y + s); L_dice = 1 - mean over the counted terms (class 0 left out with include_background=False)
        total = ce_weight L_ce + dice_weight L_dice, L_ce = multiclass_ref.softmax_ce's loss
        dL_dice / dl_j = p_j (g_j - sum_k g_k p_k), g_k = -(2 [y = k] / D - (2 I + s) / D^2) / n_terms, D = P + Y + s
    Returns Result(total, ce, dice, coeffs [B,K] or [1,K], dlogits (x grad_scale), mask, invalid count)."""
    o = Options(ce_weight, dice_weight, smooth, batch, include_background, grad_scale)
    l_ce, d_ce, mask, bad = ref.softmax_ce(logits, labels, weight, 1.0)
    return Result(*finish(prepare(logits, labels), (l_ce, d_ce), o), mask, bad)


def bounds(logits, labels, weight, s, res, o):
    """Bounds on |kernel - fp64| for the outputs of unet_dice_step, from the arithmetic of dice.hip (s = prepare(logits, labels),
    res = the fp64 Result for the same options o).  EPS32 = 2^-24.
      p        every fp32 soft-max value that enters a sum is within beta_px p of the fp64 one, beta_px = (2 min(R_px, 104) +
               K + C1) EPS32 (C1 above; R_px = max_k (m - l_k), capped where fp32 and fp64 both give 0 to 1e-45), plus TINY for a
               flushed subnormal.
      sums     dI <= sum_v beta p [y = k], dP <= sum_v beta p (the sums after the thread's are in double, in a fixed order); Y is
               an integer count, exact.
      coeffs   dice = N / D, N = 2 I + s <= D = P + Y + s: |d dice| <= 2 dI / D + N dP / D^2 <= (2 dI + dP) / D, and one rounding
               of the double quotient to fp32: + EPS32 dice.
      dice     the Dice loss can be near 0, so it is bounded absolutely: the mean of the counted coefficient bounds + EPS32 (the
               loss is <= 1 and rounded to fp32 once).
      ce       1e-6 |L_ce|, what test_multiclass_ops_gpu holds the same arithmetic to in unet_softmax_ce_step.
      total    ce_weight x ce + dice_weight x dice + EPS32 |total| (formed in double, rounded once).
      dlogits  per element |grad_scale| dice_weight p_j 2 max_k|g_k| (2 beta_px + (K + C2) EPS32 + rho_b) + TINY:
               p_j (g_j - S) with |g_j - S| <= 2 max|g|; the error of p_j gives beta, that of S = sum_k g_k p_k another beta
               (sum_k |g_k| beta p_k <= max|g| beta), hence 2 beta; (K + C2) EPS32 are the roundings (C2 above); rho_b = max over
               the counted classes of (2 dI + 2 dP) / D is the error of the table: |d a| <= a dP / D and |d c| <= (2 dI + 2 N dP / D)
               / D^2 <= (2 dI + 2 dP) / D x a / 2, and a / 2 <= |g_y| <= max|g| for the pixel's own class (for another class k
               the term is rho_b a_k / 2 = rho_b / D_k, of the size of max|g| while the classes' D are of one order, as in every
               case here; dI and dP are worst-case linear sums, some 1e3 x what random roundings leave).
               On top, ce_weight x multiclass_ref.softmax_ce_grad_bound, and 2 EPS32 (|CE part| + |Dice part|) for the product with
               ce_weight and the final addition.
    Returns Bounds(total, ce, dice, coeffs [T,K], dlogits [B,K,H,W])."""
    l = np.asarray(logits, np.float64)
    B, K, H, W = l.shape
    R = np.minimum((l.max(axis=1, keepdims=True) - l).max(axis=1, keepdims=True), ref.SATURATION)
    beta = (2 * R + K + C1) * EPS32                               # [B,1,H,W]
    okk = s.ok[:, None]
    dI = _sum_bk(beta * s.p * s.onehot + TINY * s.onehot)
    dP = _sum_bk((beta * s.p + TINY) * okk)
    if o.batch:
        dI, dP = dI.sum(axis=0, keepdims=True), dP.sum(axis=0, keepdims=True)
    I, P, Y, counted, n_terms = _terms(s, o)
    D = P + Y + o.smooth
    coeffs_b = (2 * dI + dP) / D + EPS32 * res.coeffs
    dice_b = float((coeffs_b * counted).sum() / n_terms) + EPS32
    ce_b = 1e-6 * abs(res.ce)
    total_b = o.ce_weight * ce_b + o.dice_weight * dice_b + EPS32 * abs(res.total)
    rho = ((2 * dI + 2 * dP) / D * counted).max(axis=1)           # [T]
    a, c = 2.0 / D * counted, (2.0 * I + o.smooth) / (D * D) * counted
    g = np.abs(c[:, :, None, None] - a[:, :, None, None] * s.onehot) / n_terms      # [B,K,H,W] (T = 1 broadcasts)
    gmax = g.max(axis=1, keepdims=True)
    scale = abs(o.grad_scale) * o.dice_weight
    d_b = scale * s.p * 2 * gmax * (2 * beta + (K + C2) * EPS32 + rho[:, None, None, None]) + TINY
    _, d_ce, _, _ = ref.softmax_ce(logits, labels, weight, o.grad_scale)
    d_ce = o.ce_weight * d_ce
    if o.ce_weight:
        d_b = d_b + o.ce_weight * ref.softmax_ce_grad_bound(logits, weight, K, o.grad_scale)
    d_b = d_b + 2 * EPS32 * (np.abs(d_ce) + np.abs(res.dlogits - d_ce))
    return Bounds(total_b, ce_b, dice_b, coeffs_b, d_b)


# Plain gradient descent on free logits (tests/test_dice_gpu.py): the Dice loss's gradient is O(1 / pixels per image), so a step
# of 100 moves a logit by about 0.1 .. 0.4; tests/test_dice_cpu.py checks that the fp64 loss falls at every one of the steps.
DESCENT_STEPS = 30
DESCENT_LR = 100.0


def descent_start():
    """(logits float32 [2,3,16,16], labels int64 [2,16,16]) of the descent test."""
    rs = np.random.RandomState(77)
    return rs.randn(2, 3, 16, 16).astype(np.float32), rs.randint(0, 3, (2, 16, 16)).astype(np.int64)


def error_ratios(got, res, bnd):
    """Worst |got - fp64| / bound of (total, ce, dice, coeffs, dlogits); got = any 5 values in that order (dlogits may be None)."""
    out = []
    for name in ("total", "ce", "dice", "coeffs", "dlogits"):
        v = got[len(out)]
        if v is None:
            out.append(0.0)
            continue
        err = np.abs(np.asarray(v, np.float64) - np.asarray(getattr(res, name), np.float64))
        b = np.asarray(getattr(bnd, name), np.float64)
        out.append(float((err / np.where(b > 0, b, 1.0)).max()) if (b > 0).all() or not err.any() else np.inf)
    return out
