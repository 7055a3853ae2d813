"""Fixtures and helpers that more than one GPU test module uses, once.  A plain module, not a conftest: a test module gets
a fixture by importing it by name (`from gpu_support import dev, math_mode`; pytest collects a fixture it finds in a
module's namespace), with the scope it is given here.

The library's arithmetic mode, operand staging and stream overlap (unet_set_math, unet_set_lds_dma, unet_set_overlap) are
process-wide: one left flipped changes which kernels every later module of the same pytest process reaches.  They are flipped
through library_state() only, which puts them back.  Importing this module needs neither the library nor a device."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import guarded as gd


def load():
    import _hip
    _hip.lib()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return _hip


# ---- library state ----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def library_state(**knobs):
    """`with library_state(math=2, lds_dma=0) as set_knobs:` sets the given knobs (math, lds_dma, overlap) in the order given;
    set_knobs(overlap=1) flips more inside the block.  On exit math is what unet_get_math() returned on entry, and lds_dma and
    overlap, which have no getter, are their defaults 1 and -1."""
    import _hip
    L = _hip.lib()

    def set_knobs(**kw):
        for name, value in kw.items():
            _hip.check(getattr(L, "unet_set_" + name)(value), "unet_set_" + name)

    default = L.unet_get_math()
    try:
        set_knobs(**knobs)
        yield set_knobs
    finally:
        set_knobs(overlap=-1, lds_dma=1, math=default)


def hip_fixture(**knobs):
    """The `hip` fixture of a module that runs with the library in one state throughout: `hip = hip_fixture(math=2)`."""
    @pytest.fixture(scope="module")
    def hip():
        _hip = load()
        with library_state(**knobs):
            yield _hip
    return hip


@pytest.fixture(scope="module")
def hip():
    return load()


@pytest.fixture(scope="module")
def dev():
    load()
    return torch.device("cuda:0")


@pytest.fixture
def math_mode():
    with library_state() as set_knobs:
        yield lambda m: set_knobs(math=m)


@pytest.fixture(params=[1, 0], ids=["dma", "glds"])
def dma(hip, request):
    with library_state(lds_dma=request.param):
        yield request.param


@pytest.fixture(scope="module")
def net(dev):
    """The two-class net with the seed-0 parameters of oracle.prng."""
    import network
    from oracle import prng
    m = network.Unet()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in prng.make_params(0).items()})
    return m.to(dev)


# ---- errors and test data ---------------------------------------------------------------------------------------------------
def f64(a):
    return a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)


def nerr(a, ref):
    """Normalised max error |a - ref|_inf / |ref|_inf in fp64, of tensors (on any device, with or without grad) or arrays."""
    a, ref = f64(a), f64(ref)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def rnd(*shape, seed=0, scale=1.0, fp32=False):
    """Seeded normal fp64 tensor; fp32=True rounds it through fp32 (values an fp32 kernel sees exactly)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g, dtype=torch.float64) * scale
    return t.float().double() if fp32 else t


def nhwc(t):   # NCHW cpu -> NHWC cuda fp32
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def nchw(t):   # NHWC cuda -> NCHW cpu fp64
    return t.permute(0, 3, 1, 2).double().cpu()


def image(seed, B, H, W, blobs):
    """Smooth blobs plus noise, float32 in roughly [0, 255] (a microscope-like dynamic range; not normalised), no symmetry."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.empty((B, H, W), np.float32)
    for b in range(B):
        f = 40 * rs.rand(H, W)
        for _ in range(blobs):
            cy, cx, r = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(2, max(3.0, min(H, W) / 5))
            f += 200 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
        img[b] = f
    return img


# ---- guarded buffers (tests/guarded.py) -------------------------------------------------------------------------------------
def put(mem, a, label=None):
    """numpy array -> guarded device copy"""
    return mem.inp(torch.from_numpy(np.ascontiguousarray(a)), label)


def still_poison(t):
    return bool((t.view(torch.uint8) == gd.POISON).all())


def rejected(hip, rc, mem, *outs):
    """The call returned an error and wrote nothing: every output is still all poison, every guard intact."""
    assert rc != 0 and hip.lib().unet_last_error()
    torch.cuda.synchronize()
    for o in outs:
        assert still_poison(o)
    mem.verify()


# ---- the whole net through the C ABI, on buffers the test owns ----------------------------------------------------------------
_params = {}


def params_of(base, K):
    if (base, K) not in _params:
        import multiclass_ref as ref
        _params[(base, K)] = ref.head_params(K, base=base)
    return _params[(base, K)]


class Net:
    """One handle, guarded parameters, and forward / backward on caller-owned buffers.  mode is the handle's arithmetic
    (-1: the process default at each forward); params (a state-dict of arrays) defaults to params_of(base, K)."""

    def __init__(self, mode, base, K, params=None):
        import _hip
        self.hip, self.L = _hip, _hip.lib()
        self.K = K
        self.h = _hip.Handle(base, 0, math=mode, n_classes=K)
        self.keep = gd.Arena()
        self.params = params_of(base, K) if params is None else params
        self.plist = [self.keep.inp(torch.from_numpy(v), k) for k, v in self.params.items()]
        self.ptab = _hip.ptr_table(self.plist)

    def inputs(self, B, S, seed=0):
        """Image and dlogits of (B, S); another `seed`, other values."""
        from oracle import prng
        x = self.keep.inp(torch.from_numpy(prng.make_input(1 + 10 * seed, B, S)), "x")
        dl = self.keep.inp(torch.from_numpy(prng.make_cotangent(2 + 10 * seed, (B, self.K, S - 184, S - 184))), "dlogits")
        return x, dl

    def done(self, A, wsa, outs):
        torch.cuda.synchronize()
        A.verify(*outs)
        wsa.check()
        self.keep.check()
        return outs

    def forward(self, A, wsa, ws, nbytes, x, training, dropout=None):
        """unet_forward, or with dropout = (p, seed, step) unet_forward_dropout, on workspace `ws` of arena `wsa`.  Returns the
        logits (a device tensor from `A`), fully written, with every guard of `A`, of the workspace and of the inputs intact."""
        hip, L = self.hip, self.L
        B, _, S, _ = x.shape
        logits = A.out((B, self.K, S - 184, S - 184), torch.float32, "logits")
        wsp = wsa.ptr(ws)
        if dropout is None:
            hip.check(L.unet_forward(self.h.h, self.ptab, hip.ptr(x), hip.ptr(logits), B, S, wsp, nbytes, int(training), hip.stream()), "unet_forward")
        else:
            assert training
            p, seed, step = dropout
            hip.check(L.unet_forward_dropout(self.h.h, self.ptab, hip.ptr(x), hip.ptr(logits), B, S, wsp, nbytes, p, seed, step, hip.stream()),
                      "unet_forward_dropout")
        return self.done(A, wsa, [logits])[0]

    def backward(self, A, wsa, ws, nbytes, dl, want_dx=True):
        """Every backward stage, then (want_dx) unet_backward_input, of the training forward that ran on `ws`.  Returns the 46
        gradients and, with want_dx, dx, checked like forward()'s logits."""
        hip, L = self.hip, self.L
        B, S = dl.shape[0], dl.shape[2] + 184
        wsp = wsa.ptr(ws)
        outs = [A.out(p.shape, torch.float32, "grad %s" % k) for k, p in zip(self.params, self.plist)]
        gtab = hip.ptr_table(outs)
        for s in range(L.unet_backward_stages()):
            hip.check(L.unet_backward_stage(self.h.h, s, self.ptab, hip.ptr(dl), gtab, wsp, nbytes, hip.stream()), "unet_backward_stage %d" % s)
        if want_dx:
            dx = A.out((B, 1, S, S), torch.float32, "dx")
            hip.check(L.unet_backward_input(self.h.h, self.ptab, hip.ptr(dx), wsp, nbytes, hip.stream()), "unet_backward_input")
            outs = outs + [dx]
        return self.done(A, wsa, outs)

    def step(self, A, wsa, ws, nbytes, x, dl, training):
        """Training: forward, every backward stage, unet_backward_input.  Inference: the forward.  Returns the outputs
        (device tensors from `A`), all fully written, with every guard of `A`, of the workspace (arena `wsa`) and of the inputs intact."""
        outs = [self.forward(A, wsa, ws, nbytes, x, training)]
        if training:
            outs += self.backward(A, wsa, ws, nbytes, dl)
        return outs


def strided(mem, x, top=2, left=3, bottom=2, right=3):
    """x [B,K,H,W] as a crop view inside a NaN tensor: (pointer of the view, its batch, class-plane and row strides)."""
    B, K, H, W = x.shape
    Hb, Wb = H + top + bottom, W + left + right
    big = np.full((B, K, Hb, Wb), np.nan, np.float32)
    big[:, :, top:top + H, left:left + W] = x
    d = put(mem, big, "logits inside NaN")
    return C.c_void_p(mem.address(d) + (top * Wb + left) * 4), (K * Hb * Wb, Hb * Wb, Wb)
