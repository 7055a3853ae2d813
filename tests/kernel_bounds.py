"""Element-level criteria for the reduced-precision arithmetic modes, shared by the GPU tests (kernel outputs) and by
tests/test_kernel_bounds_cpu.py (numpy / torch emulations, correct and deliberately broken).

Notation: z = the exact (fp64) value of an output element after bias, add, mask and ReLU; A = the same contraction of
absolute values (|x| * |w| + |b| + |add|), also in fp64; K = the number of products summed into the element;
u = 2^-24 (fp32 unit roundoff, round to nearest).

fp32 accumulation slack.  Every fp32 addition of the accumulation commits an error of at most u |s| with |s| <= A for
every partial sum s, whatever the order; modelled as independent zero-mean errors bounded by u A, Hoeffding gives
    P(|sum of K of them| > lam sqrt(K) u A) <= 2 exp(-lam^2 / 2),
so lam = 8 fails with probability <= 2.6e-14 per element (the style of oracle/parity.py's bf16 model).  A matrix core
that rounds once per instruction instead (fewer, possibly directed, roundings of at most 2u |s| each) stays inside it
for K / 32 instructions as long as K / 16 < lam sqrt(K), i.e. for every K below 16384.

bf16x3 (math mode 1).  Each fp32 operand a is split into hi = RNE_bf16(a) and lo = RNE_bf16(a - hi); the product ab is
formed as hi_a hi_b + hi_a lo_b + lo_a hi_b (each exact in fp32) and lo_a lo_b is dropped.  With a in [2^e, 2^(e+1)):
    |a - hi|  <= 2^(e-8) <= 2^-8 |a|                 (half an ulp of 8 significant bits)
    |r_a| = |a - hi - lo| <= half an ulp of lo <= 2^(e-17) <= 2^-17 |a|   (a - hi < 2^(e-8): lo's ulp <= 2^(e-16))
    ab - (hi_a hi_b + hi_a lo_b + lo_a hi_b) = lo_a lo_b + r_a b + (hi_a + lo_a) r_b
    |...| <= (2^-8 (1 + 2^-8))^2 + 2^-17 + 2^-17 (1 + 2^-17)  per |ab|
          <= C_SPLIT = 2^-15 (1 + 2^-7)
so |y - z| <= (C_SPLIT + lam sqrt(3K) u) A  (3K fp32 products are summed).  That catches a dropped cross term
(errors of 2^-8 |ab|) but not a truncated lo, whose extra error (< 2^-16 |ab|, random sign on random data) hides
under C_SPLIT; split_probe() below builds operands on which it shows as a bias of the mean.

bf16 outputs (math mode 2).  An output stored in bf16 must be ONE round-to-nearest-even of the fp32 accumulator, which
is within eps = lam sqrt(K) u A of z.  Hence |y - z| <= ulp_bf16 / 2 + eps, and wherever z lies farther than eps from
every rounding midpoint of bf16, y must equal RNE_bf16(z) bit for bit (check_rne).
"""
import math

import numpy as np

U32 = 2.0 ** -24
LAM = 8.0
LAM_FAIL = 2.0 * math.exp(-LAM * LAM / 2.0)            # per-element failure probability of the accumulation bound
C_SPLIT = 2.0 ** -15 * (1.0 + 2.0 ** -7)


def acc_slack(A, K, lam=LAM):
    """lam sqrt(K) u A: the fp32 accumulation slack of a sum of K products (A = sum of their absolute values)."""
    return lam * math.sqrt(K) * U32 * np.asarray(A, dtype=np.float64)


# ---- bf16 rounding, exactly, from fp64 ---------------------------------------------------------------------------------
def rne_bf16(z):
    """Round fp64 values to bf16 (8 significant bits, round to nearest, ties to even) exactly - no detour through fp32
    (which would round twice)."""
    z = np.asarray(z, dtype=np.float64)
    m, e = np.frexp(z)                                  # z = m 2^e, 0.5 <= |m| < 1
    return np.ldexp(np.round(np.ldexp(m, 8)), e - 8)    # np.round: ties to even


def trunc_bf16(z):
    """Round toward zero to 8 significant bits (a broken converter, for the CPU tests)."""
    z = np.asarray(z, dtype=np.float64)
    m, e = np.frexp(z)
    return np.ldexp(np.trunc(np.ldexp(m, 8)), e - 8)


def ulp_bf16(v):
    """Spacing of bf16 numbers at |v| (the larger spacing at an exact power of two)."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(np.where(v > 0, v, 2.0 ** -126))
    return np.ldexp(1.0, e - 8)


def midpoint_distance(z):
    """Distance of z to the nearest point where RNE_bf16 changes its result (a midpoint between two bf16 numbers)."""
    z = np.asarray(z, dtype=np.float64)
    r = rne_bf16(z)
    up = np.abs(r) + ulp_bf16(r)                       # neighbours of r in magnitude
    ar = np.abs(r)
    _, e = np.frexp(np.where(ar > 0, ar, 2.0 ** -126))
    down = ar - np.where(ar == np.ldexp(0.5, e), ulp_bf16(r) / 2, ulp_bf16(r))     # a power of two: finer spacing below
    az = np.abs(z)
    return np.minimum(np.abs(az - (ar + up) / 2), np.abs(az - (ar + down) / 2))


def check_rne(y, z, eps, relu=False, min_decidable=0.25):
    """Every bf16 output y is one RNE rounding of a value within eps of z.  Returns statistics; raises AssertionError
    naming the first offending element otherwise.
      - |y - z| <= ulp_bf16(|z| + eps) / 2 + eps everywhere;
      - where the midpoint distance of z exceeds eps, y == RNE_bf16(z) exactly;
      - relu: where z < -eps (a negative pre-activation) y is exactly 0 (z is then the pre-activation value);
      - the decidable set holds at least min_decidable of the elements that are not ReLU'd zeros (about 90 % at K = 288,
        30 % at K = 4608 on random operands: eps grows as sqrt(K) A while |z| grows as sqrt(K) rms)."""
    z = np.asarray(z, dtype=np.float64)
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float64), z.shape).ravel()
    y = np.asarray(y, dtype=np.float64).ravel()
    z = z.ravel()
    zr = np.maximum(z, 0.0) if relu else z
    neg = (z < -eps) if relu else np.zeros(z.shape, bool)
    if relu:
        bad = np.flatnonzero(neg & (y != 0.0))
        assert bad.size == 0, "ReLU'd negative not exactly 0 at %d: y=%r z=%r" % (bad[0], y[bad[0]], z[bad[0]])
    bound = ulp_bf16(np.abs(zr) + eps) / 2 + eps
    err = np.abs(y - zr)
    ratio = err / bound
    worst = int(np.argmax(ratio))
    assert ratio[worst] <= 1.0, "bf16 output beyond one rounding at %d: y=%r z=%r bound=%r" % (worst, y[worst], zr[worst], bound[worst])
    live = ~neg & ~(relu & (np.abs(z) <= eps))
    dec = live & (midpoint_distance(zr) > eps)
    mism = np.flatnonzero(dec & (y != rne_bf16(zr)))
    assert mism.size == 0, "%d of %d decidable outputs are not RNE_bf16(z), first at %d: y=%r RNE(z)=%r z=%r eps=%r" % (
        mism.size, int(dec.sum()), mism[0], y[mism[0]], rne_bf16(zr)[mism[0]], zr[mism[0]], eps[mism[0]])
    frac = float(dec.sum()) / max(int(live.sum()), 1)
    assert frac >= min_decidable, "decidable set too small (%.3f of %d): the check would be vacuous" % (frac, int(live.sum()))
    return {"n": int(z.size), "decidable": int(dec.sum()), "frac": frac, "worst": float(ratio[worst]),
            "relu_zeros": int(neg.sum())}


# ---- bf16x3 ------------------------------------------------------------------------------------------------------------
def split3(a, lo_round=rne_bf16):
    """The bf16x3 split of fp32 values: hi = RNE(a), lo = lo_round(a - hi) (exact in fp64)."""
    a = np.asarray(a, dtype=np.float64)
    hi = rne_bf16(a)
    return hi, lo_round(a - hi)


def bf16x3_bound(A, K, lam=LAM):
    return (C_SPLIT + lam * math.sqrt(3 * K) * U32) * np.asarray(A, dtype=np.float64)


def check_bf16x3(y, z, A, K, lam=LAM):
    """|y - z| <= (C_SPLIT + lam sqrt(3K) u) A elementwise; returns the worst |y - z| / A and the worst ratio to the
    bound."""
    y = np.asarray(y, dtype=np.float64).ravel(); z = np.asarray(z, dtype=np.float64).ravel()
    A = np.asarray(A, dtype=np.float64).ravel()
    b = bf16x3_bound(A, K, lam)
    err = np.abs(y - z)
    r = err / np.where(b > 0, b, 1e-300)
    i = int(np.argmax(r))
    assert r[i] <= 1.0, "bf16x3 error beyond its bound at %d: y=%r z=%r A=%r (|y-z|/A = %.3g, bound %.3g)" % (
        i, y[i], z[i], A[i], err[i] / A[i], b[i] / A[i])
    rel = err / np.where(A > 0, A, 1e-300)
    return {"worst_rel": float(rel.max()), "bound_rel": C_SPLIT + lam * math.sqrt(3 * K) * U32, "worst_ratio": float(r[i])}


def split_probe(shape, seed=0):
    """Positive fp32 operands whose split is fully determined: a = hi + lo + 3/4 ulp(lo) with hi a bf16 number in [1, 2)
    and lo a bf16 number in [2^-9, 2^-8).  Then RNE(a) = hi (a - hi < 2^-8, half of hi's ulp), RNE(a - hi) = lo + ulp(lo)
    (3/4 of an ulp rounds up), and the dropped residual is -ulp(lo)/4 = -2^-18 for every element; a truncating lo would
    leave +3 2^-18 instead.  a needs 19 significant bits: exact in fp32."""
    g = np.random.default_rng(seed)
    hi = 1.0 + g.integers(0, 128, size=shape) * 2.0 ** -7
    lo = 2.0 ** -9 + g.integers(0, 128, size=shape) * 2.0 ** -16
    a = hi + lo + 0.75 * 2.0 ** -16
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    return a


def split_bias(y, z_split, A):
    """Mean of (y - z_split) / A over all elements, z_split = the exact sum of the three bf16 products the split
    prescribes.  fp32 accumulation by round to nearest is unbiased; a wrong split of the probe's operands (a truncated
    lo: +4 2^-18 per product of a bf16-exact positive weight, relative to a in [1, 2): at least 2^-17 of A) is not.
    SPLIT_BIAS_TOL = 2^-18 leaves room for a matrix core that rounds once per instruction toward zero: K / 32 such
    roundings of at most 2^-23 of A each stay below it up to K = 1024 (the probes use K <= 9 x 96)."""
    y = np.asarray(y, dtype=np.float64).ravel(); z = np.asarray(z_split, dtype=np.float64).ravel()
    A = np.asarray(A, dtype=np.float64).ravel()
    return float(np.mean((y - z) / A))


SPLIT_BIAS_TOL = 2.0 ** -18
