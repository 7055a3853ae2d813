"""Per-op tests of adam.hip (unet_adam_step, unet_grad_sumsq, unet_grad_norm_finish, unet_grads_scale) through the C ABI against
the fp64 references and the derived bounds of tests/adam_ref.py: tensor sizes either side of ADAM_CHUNK (4096) with a zero-size
tensor in the middle, all pointers 16-byte aligned (the 16-byte kernel with 4-byte tails) and all 4 bytes off (the 4-byte kernel).
Every pointer handed to the library comes from a guarded.Arena (tests/guarded.py): every output element is written, every guard
stays intact, and the float in front of a misaligned tensor is never touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as aref
import guarded as gd
from gpu_support import hip, rejected, still_poison

pytestmark = pytest.mark.gpu

SIZES = [1, 4095, 4096, 0, 4097, 8192, 70001]              # either side of ADAM_CHUNK = 4096, a zero-size tensor in the middle
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
SENTINEL = 12345.0


def numel_table(sizes):
    return (C.c_size_t * max(len(sizes), 1))(*sizes)


class Tensors:
    """One guarded allocation per tensor; with off = 1 every tensor starts 4 bytes into its allocation, behind one float
    that is not its own (SENTINEL in inputs, poison in outputs)."""

    def __init__(self, mem, off):
        self.mem, self.off = mem, off

    def inp(self, arrays, label):
        base = [self.mem.inp(torch.from_numpy(np.concatenate([np.full(self.off, SENTINEL, np.float32), a])), "%s%d" % (label, i))
                for i, a in enumerate(arrays)]
        return base

    def out(self, sizes, label):
        return [self.mem.out((n + self.off,), torch.float32, "%s%d" % (label, i)) for i, n in enumerate(sizes)]

    def ptrs(self, bases):
        arr = (C.c_void_p * max(len(bases), 1))()
        for i, b in enumerate(bases):
            arr[i] = self.mem.address(b) + 4 * self.off
        return arr

    def values(self, bases):
        return [b[self.off:].cpu().numpy() for b in bases]

    def untouched_fronts(self, inputs=(), outputs=()):
        if self.off:
            assert all(float(b[0]) == SENTINEL for b in inputs)
            assert all(still_poison(b[:1]) for b in outputs)

    def written(self, outputs):
        """Every element of the outputs is written (no poison NaN left), every guard of the arena intact."""
        if self.off:
            assert not any(bool(torch.isnan(b[1:]).any()) for b in outputs)
            self.mem.check()
        else:
            self.mem.verify(*outputs)


class AdamCase:
    """Parameters, moments (poison before the first step: it must not read them) and per-step gradients of `sizes`, the
    fp64 Trackers beside them, and the library call."""

    def __init__(self, hip, sizes, off=0, seed=0, grads=None):
        self.hip, self.L, self.sizes = hip, hip.lib(), list(sizes)
        self.mem = gd.Arena()
        self.t = Tensors(self.mem, off)
        self.p0 = aref.make_params(sizes, seed)
        self.p = self.t.inp(self.p0, "p")
        self.m = self.t.out(sizes, "exp_avg")
        self.v = self.t.out(sizes, "exp_avg_sq")
        self.trackers = [aref.Tracker(p) for p in self.p0]
        self.make_grads = grads or (lambda step: aref.make_grads(sizes, 10 * seed + step, tiny=True))
        self.numel = numel_table(self.sizes)

    def call(self, g, step, wd, decoupled, scale_ptr=None, n=None, eps=EPS):
        return self.L.unet_adam_step(self.t.ptrs(self.p), self.t.ptrs(g), self.t.ptrs(self.m), self.t.ptrs(self.v), self.numel,
                                     len(self.sizes) if n is None else n, LR, BETAS[0], BETAS[1], eps, wd, int(decoupled), step,
                                     scale_ptr, self.hip.stream())

    def step(self, step, wd, decoupled, c=None):
        """One library call at `step` with fresh gradients (x c through grad_scale_dev), checked against the Trackers."""
        gs = self.make_grads(step)
        g = self.t.inp(gs, "g")
        scale = None if c is None else self.mem.inp(torch.tensor([c], dtype=torch.float32), "grad scale")
        self.hip.check(self.call(g, step, wd, decoupled, self.mem.ptr(scale)), "unet_adam_step")
        torch.cuda.synchronize()
        self.t.written(self.m + self.v)
        self.t.untouched_fronts(self.p + g, self.m + self.v)
        assert all(np.array_equal(a, b) for a, b in zip(self.t.values(g), gs))          # the gradients are read only
        sc = aref.scalars(LR, BETAS, EPS, wd, step)
        c32 = None if c is None else aref.f32(c)
        worst = [0.0, 0.0, 0.0]
        for tr, gi, p, m, v in zip(self.trackers, gs, *(self.t.values(x) for x in (self.p, self.m, self.v))):
            tr.step(gi, sc, decoupled, c32)
            assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all()
            assert tr.misses(p, m, v) == 0, (step, p.size, tr.worst(p, m, v))
            worst = [max(a, b) for a, b in zip(worst, tr.worst(p, m, v))]
        return worst


@pytest.mark.parametrize("c", [None, 0.37], ids=["unscaled", "grad_scale"])
@pytest.mark.parametrize("decoupled,wd", [(0, 0.0), (0, 0.1), (1, 0.0), (1, 0.1)], ids=["adam", "adam-l2", "adamw-wd0", "adamw"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-bytes-off"])
def test_adam_step_sizes_and_alignment(hip, off, decoupled, wd, c):
    """Three steps, then one call at step = 100000 (both corrections round to 1), element-wise inside the bound for p, exp_avg
    and exp_avg_sq.  The first step runs on poisoned (NaN) moments and gives finite results: they were not read.  The gradients
    hold exact zeros and values whose squares underflow in fp32."""
    case = AdamCase(hip, SIZES, off)
    for step in (1, 2, 3, 100000):
        worst = case.step(step, wd, decoupled, c)
        print("adam step %d: max err / bound  p %.3g  m %.3g  v %.3g" % (step, *worst))
    assert aref.scalars(LR, BETAS, EPS, wd, 100000).rbc2 == 1.0


def test_adam_step_table_limits(hip):
    """46 tensors are accepted.  47 tensors, step = 0 and eps = 0 return the argument error, unet_last_error names the argument,
    and nothing is written."""
    sizes = [(37 * i) % 300 + 1 for i in range(46)]; sizes[20] = 4097; sizes[45] = 4096
    case = AdamCase(hip, sizes)
    case.step(1, 0.1, 0)
    case.step(2, 0.1, 0)
    case = AdamCase(hip, sizes + [5])
    g = case.t.inp(case.make_grads(1), "g")
    for kw, word in ((dict(n=47), b"n=47"), (dict(n=0), b"n=0"), (dict(n=46, step=0), b"step=0"), (dict(n=46, eps=0.0), b"eps=0")):
        rc = case.call(g, kw.pop("step", 1), 0.0, 0, **kw)
        assert rc == -2 and word in hip.lib().unet_last_error(), hip.lib().unet_last_error()
        rejected(hip, rc, case.mem, *(case.m + case.v))
        assert all(np.array_equal(a, b) for a, b in zip(case.t.values(case.p), case.p0))


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-bytes-off"])
def test_adam_step_edge_values(hip, off):
    """Gradients exactly 0 (wd = 0): p keeps its bits, exp_avg and exp_avg_sq are exactly 0, step after step.  Gradients whose
    squares all underflow in fp32 (|g| <= 1e-23): inside the bound, whose 2^-149 per product covers it."""
    sizes = [4097, 5000]
    zero = AdamCase(hip, sizes, off, grads=lambda step: [np.zeros(n, np.float32) for n in sizes])
    for step in (1, 2):
        zero.step(step, 0.0, 0)
        assert all(np.array_equal(a, b) for a, b in zip(zero.t.values(zero.p), zero.p0))
        assert all(not a.any() for a in zero.t.values(zero.m) + zero.t.values(zero.v))

    def tiny(step):
        rs = np.random.RandomState(step)
        return [(rs.choice([1e-23, -1e-25, 3e-30, 1e-40, -1e-44], n) * rs.uniform(0.5, 1.0, n)).astype(np.float32) for n in sizes]
    under = AdamCase(hip, sizes, off, grads=tiny)
    for step in (1, 2, 3):
        under.step(step, 0.0, 0)
    assert all((v < 2.0 ** -126).all() for v in under.t.values(under.v))          # subnormal or 0, as the bound's term assumes


def test_adam_step_is_deterministic_across_streams(hip):
    """The same two steps on two non-default streams: p, exp_avg, exp_avg_sq bit-equal."""
    res = []
    for _ in range(2):
        with torch.cuda.stream(torch.cuda.Stream()):
            case = AdamCase(hip, SIZES)
            case.step(1, 0.1, 1, 0.37)
            case.step(2, 0.1, 1, 0.37)
            res.append([b.clone() for b in case.p + case.m + case.v])
        torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*res))


@pytest.mark.parametrize("decoupled", [0, 1], ids=["adam-l2", "adamw"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-bytes-off"])
def test_fused_grad_scale_equals_separate_scale(hip, off, decoupled):
    """unet_grads_scale followed by unet_adam_step(NULL) is bit-equal to unet_adam_step(grad_scale_dev) on copies of the
    same state, for two steps."""
    L = hip.lib()
    a, b = AdamCase(hip, SIZES, off), AdamCase(hip, SIZES, off)
    scale = a.mem.inp(torch.tensor([0.37], dtype=torch.float32), "grad scale")
    for step in (1, 2):
        gs = aref.make_grads(SIZES, step, tiny=True)
        ga, gb = a.t.inp(gs, "g"), b.t.inp(gs, "g")
        hip.check(L.unet_grads_scale(a.t.ptrs(ga), a.numel, len(SIZES), a.mem.ptr(scale), hip.stream()), "unet_grads_scale")
        hip.check(a.call(ga, step, 0.1, decoupled), "unet_adam_step")
        hip.check(b.call(gb, step, 0.1, decoupled, a.mem.ptr(scale)), "unet_adam_step")
        torch.cuda.synchronize()
        a.t.written(a.m + a.v); b.t.written(b.m + b.v)
        for x, y in zip(a.p + a.m + a.v, b.p + b.m + b.v):
            assert torch.equal(x[off:], y[off:])
        a.t.untouched_fronts(a.p + ga, a.m + a.v)
        assert all(np.array_equal(s, g * np.float32(0.37)) for s, g in zip(a.t.values(ga), gs))      # one fp32 multiply


# ---- the norm, the coefficient and the in-place scale -----------------------------------------------------------------------
def wide_grads(sizes, seed):
    """magnitudes from 1e-12 to 1e6"""
    rs = np.random.RandomState(seed)
    return [(rs.randn(n) * 10.0 ** rs.uniform(-12, 6, n)).astype(np.float32) for n in sizes]


def norm_case(hip, sizes, gs, max_norm, off, split=None):
    """sumsq (in the calls `split` lists as slices; default one) + finish + in-place scale, all checked.  Returns (norm, coef)."""
    L = hip.lib()
    mem = gd.Arena()
    t = Tensors(mem, off)
    g = t.inp(gs, "g")
    count = aref.partial_count(sizes)
    partials = mem.scratch(8 * count, "partials")                           # exact to the byte
    out2 = mem.out((2,), torch.float32, "norm and coefficient")
    offset = 0
    for sl in split or [slice(0, len(sizes))]:
        n = len(sizes[sl])
        numel = numel_table(sizes[sl])
        assert L.unet_grad_sumsq_partials(numel, n) == aref.partial_count(sizes[sl])
        hip.check(L.unet_grad_sumsq(t.ptrs(g[sl]), numel, n, mem.ptr(partials), offset, hip.stream()), "unet_grad_sumsq")
        offset += aref.partial_count(sizes[sl])
    assert offset == count
    hip.check(L.unet_grad_norm_finish(mem.ptr(partials), count, max_norm, mem.ptr(out2), hip.stream()), "unet_grad_norm_finish")
    torch.cuda.synchronize()
    mem.verify(out2)
    assert not bool(torch.isnan(partials.view(torch.float64)).any())       # every partial written
    t.untouched_fronts(g)
    assert all(np.array_equal(a, b) for a, b in zip(t.values(g), gs))
    norm32, coef32 = (np.float32(x) for x in out2.cpu().numpy())
    norm64, _ = aref.grad_norm(gs, max_norm)
    assert abs(float(norm32) - norm64) <= aref.norm_rel_bound(count) * norm64, (float(norm32), norm64)
    assert coef32 == aref.coef_fp32(norm32, max_norm), (coef32, norm32)
    coef_ptr = C.c_void_p(mem.address(out2) + 4)
    for sl in split or [slice(0, len(sizes))]:
        hip.check(L.unet_grads_scale(t.ptrs(g[sl]), numel_table(sizes[sl]), len(sizes[sl]), coef_ptr, hip.stream()), "unet_grads_scale")
    torch.cuda.synchronize()
    mem.check()
    t.untouched_fronts(g)
    assert all(np.array_equal(a, b * coef32) for a, b in zip(t.values(g), gs))
    return float(norm32), float(coef32)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-bytes-off"])
def test_grad_norm_sizes_and_alignment(hip, off):
    """The fp32 norm within the derived relative bound of fp64, the coefficient exactly min(1, max_norm / (norm + 1e-6)) formed
    in fp32 from the returned norm, for a max_norm that clips and one that does not; the scaled gradients are g * coef exactly."""
    gs = wide_grads(SIZES, 3)
    norm, coef = norm_case(hip, SIZES, gs, 1.0, off)
    assert norm > 1e5 and coef < 1e-5
    norm, coef = norm_case(hip, SIZES, gs, 1e9, off)
    assert coef == 1.0
    norm, coef = norm_case(hip, SIZES, [np.zeros(n, np.float32) for n in SIZES], 0.5, off)
    assert norm == 0.0 and coef == 1.0


def test_grad_norm_over_47_tensors_in_two_calls(hip):
    """More tensors than one table holds: two unet_grad_sumsq calls at increasing partial offsets, one finish."""
    sizes = [(53 * i) % 700 + 1 for i in range(47)]; sizes[10] = 4097; sizes[46] = 9000
    gs = wide_grads(sizes, 4)
    norm, coef = norm_case(hip, sizes, gs, 10.0, 0, split=[slice(0, 46), slice(46, 47)])
    assert coef < 1.0
    both, _ = norm_case(hip, sizes, gs, 10.0, 0, split=[slice(0, 20), slice(20, 47)])
    assert both == norm


def test_grad_norm_table_limits_and_non_finite(hip):
    """47 tensors in one call and max_norm = 0 are argument errors that write nothing; a NaN gradient gives a NaN norm and a
    NaN coefficient, an infinite one an infinite norm and coefficient 0 (IEEE, as torch)."""
    L = hip.lib()
    mem = gd.Arena()
    t = Tensors(mem, 0)
    sizes = [3] * 47
    g = t.inp([np.ones(3, np.float32)] * 47, "g")
    partials = mem.scratch(8 * 47, "partials")
    out2 = mem.out((2,), torch.float32, "out2")
    one = mem.inp(torch.ones(1), "scale")
    rc = L.unet_grad_sumsq(t.ptrs(g), numel_table(sizes), 47, mem.ptr(partials), 0, hip.stream())
    assert rc == -2 and b"n=47" in L.unet_last_error()
    rejected(hip, rc, mem, partials)
    rc = L.unet_grads_scale(t.ptrs(g), numel_table(sizes), 47, mem.ptr(one), hip.stream())
    assert rc == -2 and b"n=47" in L.unet_last_error()
    rc = L.unet_grad_norm_finish(mem.ptr(partials), 47, 0.0, mem.ptr(out2), hip.stream())
    assert rc == -2 and b"max_norm" in L.unet_last_error()
    rejected(hip, rc, mem, out2, partials)
    for bad, want_norm, want_coef in ((np.nan, np.isnan, np.isnan), (np.inf, np.isposinf, lambda c: c == 0.0)):
        vals = np.ones(5000, np.float32); vals[4500] = bad
        gb = mem.inp(torch.from_numpy(vals), "g")
        pb = mem.scratch(16, "partials")
        out2.fill_(7.0)                                                         # poison is a NaN itself: start from a number
        hip.check(L.unet_grad_sumsq(t.ptrs([gb]), numel_table([5000]), 1, mem.ptr(pb), 0, hip.stream()))
        hip.check(L.unet_grad_norm_finish(mem.ptr(pb), 2, 1.0, mem.ptr(out2), hip.stream()))
        torch.cuda.synchronize()
        norm, coef = out2.cpu().numpy()
        assert want_norm(norm) and want_coef(coef), (norm, coef)
    mem.check()
