"""fp64 references of adam.hip (unet_adam_step, unet_grad_sumsq + unet_grad_norm_finish, unet_grads_scale) with their
element-wise bounds, shared by tests/test_adam_cpu.py, tests/test_adam_ops_gpu.py and tests/test_adam_gpu.py.  Imported like
the other *_ref.py files; needs neither the library nor a device.

The update, in the order include/unet_hip.h states it (sc = scalars(...), the fp32 values the host hands the kernel):
    1  g = g * c                         only with a grad scale c
    2  g = g + wd * p                    Adam (L2), wd != 0        |   p = p * decay      AdamW, wd != 0
    3  m = m + om1 * (g - m)
    4  v = beta2 * v + om2 * (g * g)
    5  d = sqrt(v) * rbc2 + eps
    6  p = p - step_size * (m / d)
update() is that in fp64.  Tracker carries it over several steps together with a running error bound: every fp32 operation of
the kernel is one entry of the list above, it is correctly rounded, so its result is off by at most U = 2^-24 of itself, a
product or quotient that lands among the subnormals by at most T = 2^-149 more (sums, differences and square roots of floats
do not underflow), plus what the errors already in its operands do to it.  The helpers _mul, _add, _sub, _sqrt, _div below
state exactly that for (value, error) pairs, so the errors carried in m, v and p go into the next step through the same rules.
Two allowances, both stated where they are made: the first moment may also be formed as beta1 * m + om1 * g (torch's other
form; beta1 + om1 is 1 only up to the rounding of om1), and the host's pow / sqrt may differ from Python's in the last place
of the double, which can move the fp32 rounding of step_size and rbc2 by one place (U relative)."""
import collections
import math

import numpy as np

U = 2.0 ** -24          # relative rounding error of one correctly rounded fp32 operation
T = 2.0 ** -149         # absolute error of a product or quotient that underflows (the smallest subnormal)
CHUNK = 4096            # ADAM_CHUNK of adam.hip: elements of one tensor behind one fp64 partial
FINISH_THREADS = 256    # the finishing workgroup

Scalars = collections.namedtuple("Scalars", "step_size rbc2 beta1 om1 beta2 om2 eps wd decay")


def f32(x):
    return float(np.float32(x))


def scalars(lr, betas, eps, wd, step, rounded=True):
    """What unet_adam_step computes with: the fp32 arguments, and om1, om2, decay, rbc2 and step_size formed in double from them
    and rounded to fp32 once each.  rounded=False keeps everything in double (the form torch.optim.Adam computes in float64)."""
    r = f32 if rounded else float
    lr, b1, b2, eps, wd = (r(x) for x in (lr, betas[0], betas[1], eps, wd))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return Scalars(r(lr / bc1), r(1.0 / math.sqrt(bc2)), b1, r(1.0 - b1), b2, r(1.0 - b2), eps, wd, r(1.0 - lr * wd))


def update(p, m, v, g, sc, decoupled, c=None):
    """One update in fp64 in the stated order; returns the new (p, m, v)."""
    p, m, v, g = (np.asarray(a, np.float64) for a in (p, m, v, g))
    if c is not None:
        g = g * c
    if sc.wd != 0.0:
        if decoupled:
            p = p * sc.decay
        else:
            g = g + sc.wd * p
    m = m + sc.om1 * (g - m)
    v = sc.beta2 * v + sc.om2 * (g * g)
    d = np.sqrt(v) * sc.rbc2 + sc.eps
    return p - sc.step_size * (m / d), m, v


# ---- (value, error) pairs: value in fp64, error >= |what the kernel holds - value| ----------------------------------------------
def _k(x, e=0.0):
    return (np.float64(x), np.float64(e))


def _mul(a, b):
    val = a[0] * b[0]
    prop = np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1]
    return val, prop + U * (np.abs(val) + prop) + T


def _add(a, b, sign=1.0):
    val = a[0] + sign * b[0]
    prop = a[1] + b[1]
    return val, prop + U * (np.abs(val) + prop)


def _sub(a, b):
    return _add(a, b, -1.0)


def _sqrt(a):
    val = np.sqrt(a[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        # |sqrt(x) - sqrt(y)| = |x - y| / (sqrt(x) + sqrt(y)) <= |x - y| / sqrt(y), and <= sqrt(|x - y|)
        prop = np.where(val > 0, np.minimum(a[1] / np.where(val > 0, val, 1.0), np.sqrt(a[1])), np.sqrt(a[1]))
    return val, prop + U * (val + prop)


def _div(a, b):
    val = a[0] / b[0]
    low = np.abs(b[0]) - b[1]                                  # the kernel's divisor is at least this far from 0
    assert np.all(low > 0)
    prop = (a[1] + np.abs(val) * b[1]) / low
    return val, prop + U * (np.abs(val) + prop) + T


class Tracker:
    """One tensor's p, m, v in fp64 from the stated order (the values are update()'s, bit for bit: tests/test_adam_cpu.py), with
    ep, em, ev >= the kernel's distance from them, element-wise."""

    def __init__(self, p):
        self.p = np.asarray(p, np.float64).copy()
        self.m = np.zeros_like(self.p); self.v = np.zeros_like(self.p)
        self.ep = np.zeros_like(self.p); self.em = np.zeros_like(self.p); self.ev = np.zeros_like(self.p)

    def step(self, g, sc, decoupled, c=None):
        """g: this step's gradient as the kernel reads it (exact fp32 values); c: the fp32 scale it multiplies by, or None."""
        P, M, V = (self.p, self.ep), (self.m, self.em), (self.v, self.ev)
        G = (np.asarray(g, np.float64), np.float64(0.0))
        if c is not None:
            G = _mul(G, _k(c))
        if sc.wd != 0.0:
            if decoupled:
                P = _mul(P, _k(sc.decay))
            else:
                G = _add(G, _mul(_k(sc.wd), P))
        lerp = _add(M, _mul(_k(sc.om1), _sub(G, M)))
        other = _add(_mul(_k(sc.beta1), M), _mul(_k(sc.om1), G))            # the allowance for torch's second form
        M = (lerp[0], np.maximum(lerp[1], other[1] + np.abs(other[0] - lerp[0])))
        V = _add(_mul(_k(sc.beta2), V), _mul(_k(sc.om2), _mul(G, G)))
        D = _add(_mul(_sqrt(V), _k(sc.rbc2, U * sc.rbc2)), _k(sc.eps))
        P = _sub(P, _mul(_k(sc.step_size, U * sc.step_size), _div(M, D)))
        (self.p, self.ep), (self.m, self.em), (self.v, self.ev) = P, M, V

    def misses(self, p, m, v):
        """How many elements of the kernel's p, m, v lie outside the bound (non-finite ones count)."""
        bad = 0
        for got, want, err in ((p, self.p, self.ep), (m, self.m, self.em), (v, self.v, self.ev)):
            got = np.asarray(got, np.float64)
            bad += int((~(np.abs(got - want) <= err)).sum())
        return bad

    def worst(self, p, m, v):
        """max over the elements of error / bound, for p, m, v (printed by the tests; 0 / 0 counts as 0)."""
        out = []
        for got, want, err in ((p, self.p, self.ep), (m, self.m, self.em), (v, self.v, self.ev)):
            e = np.abs(np.asarray(got, np.float64) - want)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(e == 0, 0.0, e / err)
            out.append(float(r.max()) if r.size else 0.0)
        return out


# ---- the kernel's arithmetic in numpy fp32, and ways to get it wrong (tests/test_adam_cpu.py) ----------------------------------------
VARIANTS = ("stated", "mul_add", "no_bias_correction", "eps_in_sqrt", "swapped_decay", "beta2_in_first_moment", "scale_ignored")


def emulate(p, m, v, g, lr, betas, eps, wd, step, decoupled, c=None, variant="stated"):
    """One update on fp32 arrays, each operation rounded to fp32 by numpy.  'stated' is the kernel's order, 'mul_add' forms
    m = beta1 * m + om1 * g; the others are the mistakes their names say."""
    F = np.float32
    sc = scalars(lr, betas, eps, wd, step)
    p, m, v, g = (np.asarray(a, F).copy() for a in (p, m, v, g))
    step_size, rbc2 = F(sc.step_size), F(sc.rbc2)
    if variant == "no_bias_correction":
        step_size, rbc2 = F(lr), F(1.0)
    if variant == "swapped_decay":
        decoupled = not decoupled
    with np.errstate(all="ignore"):
        if c is not None and variant != "scale_ignored":
            g = g * F(c)
        if sc.wd != 0.0:
            if decoupled:
                p = p * F(sc.decay)
            else:
                g = g + F(sc.wd) * p
        if variant == "mul_add":
            m = F(sc.beta1) * m + F(sc.om1) * g
        elif variant == "beta2_in_first_moment":
            m = m + F(sc.om2) * (g - m)
        else:
            m = m + F(sc.om1) * (g - m)
        v = F(sc.beta2) * v + F(sc.om2) * (g * g)
        if variant == "eps_in_sqrt":
            d = np.sqrt(v * (rbc2 * rbc2) + F(sc.eps))
        else:
            d = np.sqrt(v) * rbc2 + F(sc.eps)
        p = p - step_size * (m / d)
    assert p.dtype == F and m.dtype == F and v.dtype == F
    return p, m, v


# ---- the gradient norm and the clipping coefficient -------------------------------------------------------------------------------
def partial_count(sizes):
    """unet_grad_sumsq_partials: one fp64 partial per started chunk of CHUNK elements of every tensor."""
    return sum((int(n) + CHUNK - 1) // CHUNK for n in sizes)


def grad_norm(grads, max_norm):
    """(norm, coef) of torch.nn.utils.clip_grad_norm_ in fp64: the 2-norm over all tensors, min(1, max_norm / (norm + 1e-6))."""
    total = math.fsum(float(np.square(np.asarray(g, np.float64)).sum()) for g in grads)
    norm = math.sqrt(total)
    return norm, min(1.0, max_norm / (norm + 1e-6))


def norm_rel_bound(n_partials):
    """Relative bound of the kernel's fp32 norm against fp64.  Every square is exact in fp64 and every term is >= 0, so a sum
    is off by at most (the additions an element passes through) x 2^-53 of itself: CHUNK / 256 = 16 per lane, 6 butterfly
    steps over the wave and 3 over the block's four waves, then in the finish ceil(n_partials / 256) per thread and 8 tree
    steps.  The fp64 square root halves that and adds one rounding, the conversion to fp32 adds U.  (First order; the 1.01
    covers the products of these terms.)"""
    adds = CHUNK // FINISH_THREADS + 6 + 3 + (n_partials + FINISH_THREADS - 1) // FINISH_THREADS + 8
    return 1.01 * (U + (adds / 2.0 + 1.0) * 2.0 ** -53)


def coef_fp32(norm32, max_norm):
    """The coefficient the finish kernel forms from the fp32 norm it wrote, operation by operation in fp32."""
    F = np.float32
    with np.errstate(all="ignore"):
        c = F(max_norm) / (F(norm32) + F(1e-6))
    return F(1.0) if c > F(1.0) else c


# ---- test inputs --------------------------------------------------------------------------------------------------------------------
def make_params(sizes, seed=0):
    rs = np.random.RandomState(seed)
    return [rs.randn(n).astype(np.float32) for n in sizes]


def make_grads(sizes, seed, tiny=False):
    """Gradients over seven decades (1e-6 .. 10) with exact zeros planted; tiny=True adds magnitudes near 1e-25 and 1e-40,
    whose squares underflow in fp32 (to a subnormal or to 0)."""
    rs = np.random.RandomState(1000 + seed)
    out = []
    for n in sizes:
        g = (rs.randn(n) * 10.0 ** rs.uniform(-6, 1, n)).astype(np.float32)
        if n:
            g[rs.rand(n) < 0.05] = 0.0
            if tiny:
                pick = rs.rand(n) < 0.1
                g[pick] = (rs.choice([1e-25, -3e-23, 1e-40, 7e-21], int(pick.sum())) * rs.uniform(0.5, 2.0, int(pick.sum()))).astype(np.float32)
        out.append(g)
    return out
