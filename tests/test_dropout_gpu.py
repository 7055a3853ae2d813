"""Drop-out at the end of the contracting path (Unet(dropout=p); include/unet_hip.h, unet_forward_dropout) on the GPU.

Everything here is exact except the whole-net gradients: the keep flags are a stated function of (seed, step, site, element
index) that tests/philox_ref.py restates in numpy (held to the published Philox known answers by test_dropout_cpu.py), the
drop is one fp32 multiply per element, and s = 1 / (1 - p) = 2 at p = 0.5 is exact in fp32 and bf16.
  1. unet_dropout_mask against the numpy flags, bit for bit, and the flags' statistics (5 sigma of a fair coin over 2^20 draws);
  2. the per-op forward (with and without the pooled output) and backward, fp32 and bf16 elements, bit for bit, in guarded buffers;
  3. the whole net: the two sites' tensors of a dropped forward against the clean forward and the numpy flags, bit for bit; p = 0
     is the plain training forward and backward, bit for bit;
  4. the whole net's gradients on HIP's own branch: the network as the piecewise-linear map that the dropped forward's ReLU masks
     and pool winners define, in torch fp64, at the bounds of tests/test_net_gpu.py's same-branch test (scaling by 2 adds no rounding);
  5. the module: when drop-out is active, that its state reproduces a forward, and a bit-exact checkpoint resume."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded as gd
import philox_ref
from gpu_support import hip, library_state

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5           # tests/test_net_gpu.py, same-branch test
GRAD_TOL = 3e-4
SIGMA5 = 5 * 0.5 / np.sqrt(1 << 20)      # 0.00244: 5 sigma of the mean of 2^20 fair coin flips
SEED, STEP = 0x123456789ABCDEF, 5
S, B = 188, 2


@pytest.fixture(params=[4, 2], ids=["fp32", "bf16"])
def es(hip, request):
    """Element size of the per-op entries' tensors: they follow unet_set_math (2 = bf16 tensors)."""
    default = hip.lib().unet_get_math()
    with library_state(math=2 if request.param == 2 else default if default != 2 else 3):
        yield request.param


def gpu_flags(hip, seed, step, site, first, n, p):
    mem = gd.Arena()
    keep = mem.out(n, torch.uint8, "keep")
    hip.check(hip.lib().unet_dropout_mask(seed, step, site, first, n, p, mem.ptr(keep), hip.stream()), "unet_dropout_mask")
    torch.cuda.synchronize()
    mem.check()
    return keep.cpu().numpy()


# ---- 1. keep flags --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site", [0, 1])
@pytest.mark.parametrize("p", [0.5, 0.25, 0.0])
@pytest.mark.parametrize("first,step", [(0, 0), (6, STEP), (4099, STEP), ((1 << 34) + 4099, STEP), (3, (1 << 32) + 7), ((1 << 61) + 1, (1 << 62) + 3)],
                         ids=["origin", "first%4=2", "first%4=3", "first>2^34", "step>2^32", "high words"])
def test_keep_flags_equal_the_numpy_philox(hip, site, p, first, step):
    n = 4099
    got = gpu_flags(hip, SEED, step, site, first, n, p)
    want = philox_ref.keep_flags(SEED, step, site, first, n, p)
    assert set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got, want), "%d of %d flags differ, first at %d" % ((got != want).sum(), n, int(np.flatnonzero(got != want)[0]))
    if p == 0.0:
        assert got.all()
    else:
        assert abs(got.mean() - (1 - p)) < 5 * np.sqrt(p * (1 - p) / n)


def test_keep_flags_statistics(hip):
    n = 1 << 20
    a = gpu_flags(hip, SEED, STEP, 0, 0, n, 0.5)
    assert np.array_equal(a, philox_ref.keep_flags(SEED, STEP, 0, 0, n, 0.5))
    nxt = gpu_flags(hip, SEED, STEP + 1, 0, 0, n, 0.5)
    other = gpu_flags(hip, SEED, STEP, 1, 0, n, 0.5)
    kept, d_step, d_site = a.mean(), (a != nxt).mean(), (a != other).mean()
    print("kept %.5f, differ from step+1 %.5f, from site 1 %.5f (5 sigma = %.5f)" % (kept, d_step, d_site, SIGMA5))
    assert abs(kept - 0.5) < SIGMA5
    assert abs(d_step - 0.5) < SIGMA5
    assert abs(d_site - 0.5) < SIGMA5


def test_argument_checks(hip):
    L = hip.lib()
    mem = gd.Arena()
    x = mem.inp(torch.zeros(1, 2, 2, 4), "x")
    st = hip.stream()
    for (H, W, Cc, p, site) in ((3, 2, 4, 0.5, 0), (2, 3, 4, 0.5, 0), (2, 2, 6, 0.5, 0), (2, 2, 4, 1.0, 0), (2, 2, 4, -0.1, 0),
                                (2, 2, 4, float("nan"), 0), (2, 2, 4, 0.5, 2)):
        assert L.unet_dropout_pool_fwd(mem.ptr(x), None, 1, H, W, Cc, p, 0, 0, site, st) == -2, (H, W, Cc, p, site)
    assert L.unet_dropout_bwd(mem.ptr(x), 16, 1.0, st) == -2
    assert L.unet_dropout_mask(0, 0, 0, 0, 16, 1.5, mem.ptr(x), st) == -2
    torch.cuda.synchronize()
    mem.check()
    assert torch.equal(x.cpu(), torch.zeros(1, 2, 2, 4))


# ---- 2. per-op forward and backward -------------------------------------------------------------------------------------------
def dropped(x, keep, p, dtype):
    """where(keep, x * s, 0): one fp32 multiply, stored in `dtype` (bf16: round to nearest even)."""
    y = x.float().numpy() * philox_ref.scale(p)
    assert y.dtype == np.float32
    return torch.where(torch.from_numpy(keep.reshape(x.shape).astype(bool)), torch.from_numpy(y).to(dtype), torch.zeros((), dtype=dtype))


def pool2(t):
    Bq, H, W, Cc = t.shape
    return t.float().view(Bq, H // 2, 2, W // 2, 2, Cc).amax(dim=(2, 4)).to(t.dtype)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("p", [0.5, 0.25])
@pytest.mark.parametrize("shape", [(1, 2, 2, 4), (3, 6, 10, 12), (2, 16, 16, 512)], ids=["one window", "odd", "site 0 at S=188"])
def test_per_op_forward_and_backward_are_exact(hip, es, shape, p):
    L = hip.lib()
    dtype = torch.bfloat16 if es == 2 else torch.float32
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.relu(torch.randn(*shape, generator=g)).to(dtype)            # about half exact zeros: ties in the pool
    n = x.numel()
    Bq, H, W, Cc = shape
    for site, pooled in ((0, True), (1, False), (1, True)):
        mem = gd.Arena()
        xd = mem.inp(x, "x")
        t = mem.out((Bq, H // 2, W // 2, Cc), dtype, "pooled") if pooled else None
        hip.check(L.unet_dropout_pool_fwd(mem.ptr(xd), mem.ptr(t), Bq, H, W, Cc, p, SEED, STEP, site, hip.stream()), "unet_dropout_pool_fwd")
        torch.cuda.synchronize()
        mem.verify(t)
        want = dropped(x, philox_ref.keep_flags(SEED, STEP, site, 0, n, p), p, dtype)
        assert torch.equal(bits(xd.cpu()), bits(want)), "site %d: %d elements differ" % (site, int((bits(xd.cpu()) != bits(want)).sum()))
        if pooled:
            assert torch.equal(bits(t.cpu()), bits(pool2(want)))
    # backward: g * s in place; a length that is no multiple of 4 takes the tail
    gr = torch.randn(n + 3, generator=g).to(dtype)
    for m in (n, n + 3):
        mem = gd.Arena()
        gd_ = mem.inp(gr[:m], "g")
        hip.check(L.unet_dropout_bwd(mem.ptr(gd_), m, p, hip.stream()), "unet_dropout_bwd")
        torch.cuda.synchronize()
        mem.check()
        want = torch.from_numpy(gr[:m].float().numpy() * philox_ref.scale(p)).to(dtype)
        assert torch.equal(bits(gd_.cpu()), bits(want))


# ---- 3. / 4. whole net through the C ABI ---------------------------------------------------------------------------------------
_inputs = {}


def inputs():
    if not _inputs:
        from oracle import prng
        _inputs["params"] = prng.make_params(0)
        _inputs["x"] = prng.make_input(1, B, S)
        _inputs["dl"] = prng.make_cotangent(2, (B, 2, S - 184, S - 184))
    return _inputs["params"], _inputs["x"], _inputs["dl"]


class Step:
    """One training forward (plain, or with drop-out) and optionally its backward on buffers of its own."""

    def __init__(self, hip, h, p=None, seed=SEED, step=STEP, backward=False):
        L = hip.lib()
        params, x, dl = inputs()
        dev = torch.device("cuda", 0)
        self.h = h
        self.names = list(params)
        self.plist = [torch.from_numpy(v).to(dev) for v in params.values()]
        self.nbytes = h.workspace_bytes(B, S, True)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        xd = torch.from_numpy(x).to(dev)
        logits = torch.empty(B, 2, S - 184, S - 184, device=dev)
        ptab = hip.ptr_table(self.plist)
        if p is None:
            hip.check(L.unet_forward(h.h, ptab, hip.ptr(xd), hip.ptr(logits), B, S, hip.ptr(self.ws), self.nbytes, 1, hip.stream()), "unet_forward")
        else:
            hip.check(L.unet_forward_dropout(h.h, ptab, hip.ptr(xd), hip.ptr(logits), B, S, hip.ptr(self.ws), self.nbytes, p, seed, step,
                                             hip.stream()), "unet_forward_dropout")
        self.grads = None
        if backward:
            grads = [torch.empty_like(q) for q in self.plist]
            dld = torch.from_numpy(dl).to(dev)
            hip.check(L.unet_backward(h.h, ptab, hip.ptr(dld), hip.ptr_table(grads), hip.ptr(self.ws), self.nbytes, hip.stream()), "unet_backward")
            self.grads = grads
        torch.cuda.synchronize()
        self.logits = logits

    def view(self, name):
        return self.h.buffer_view(self.ws, B, S, True, name).cpu()


@pytest.fixture(params=[-1, 2], ids=["fp32", "bf16-tensors"])
def handle(hip, request):
    return hip.Handle(64, 0, math=request.param)


def test_whole_net_forward_drops_exactly_the_reference_flags(hip, handle):
    clean = Step(hip, handle)
    drop = Step(hip, handle, p=0.5)
    a23c, a23 = clean.view("a2_3"), drop.view("a2_3")
    keep0 = philox_ref.keep_flags(SEED, STEP, 0, 0, a23.numel(), 0.5).reshape(a23.shape).astype(bool)
    want = torch.where(torch.from_numpy(keep0), a23c * 2, torch.zeros((), dtype=a23c.dtype))
    assert a23.shape == (B, 16, 16, 512) and (a23c > 0).float().mean() > 0.05
    assert torch.equal(bits(a23), bits(want)), "%d elements of a2_3 differ" % int((bits(a23) != bits(want)).sum())
    assert torch.equal(bits(drop.view("t_3")), bits(pool2(want)))
    # site 1 follows other conv5x inputs than the clean run's: the flags and the form of the values
    a24 = drop.view("a2_4")
    keep1 = torch.from_numpy(philox_ref.keep_flags(SEED, STEP, 1, 0, a24.numel(), 0.5).reshape(a24.shape).astype(bool))
    assert a24.shape == (B, 4, 4, 1024)
    assert not a24[~keep1].any()
    assert (a24 >= 0).all() and torch.equal(bits(a24), bits(torch.where(keep1, a24 / 2 * 2, torch.zeros((), dtype=a24.dtype))))
    assert (a24[keep1] > 0).any()                                             # (not vacuous: kept elements are live ReLU outputs)
    assert not torch.equal(drop.logits, clean.logits)
    # another step draws other flags
    again = Step(hip, handle, p=0.5, step=STEP + 1)
    assert not torch.equal(bits(again.view("a2_3")), bits(a23))


def test_p_zero_is_the_plain_training_step(hip, handle):
    clean = Step(hip, handle, backward=True)
    zero = Step(hip, handle, p=0.0, backward=True)
    assert torch.equal(clean.logits, zero.logits)
    for k, a, b in zip(clean.names, clean.grads, zero.grads):
        assert torch.equal(a, b), k
    for name in ("a2_3", "t_3", "a2_4", "g_a2_3", "g_a2_4"):
        assert torch.equal(bits(clean.view(name)), bits(zero.view(name))), name


def piecewise_linear(p, x, masks, sels, s):
    """The network on a fixed branch: ReLU = multiply by the mask, pool = gather of the winner, the two sites followed by s."""
    m = {k: torch.from_numpy(v).double() for k, v in masks.items()}

    def cr(name, buf, t):
        return F.conv2d(t, p[name + ".weight"], p[name + ".bias"]) * m[buf]

    def pool(t, sel):
        Bq, Cc, H, W = t.shape
        win = t.view(Bq, Cc, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(Bq, Cc, H // 2, W // 2, 4)
        return win.gather(-1, torch.from_numpy(sel.astype(np.int64))[..., None])[..., 0]

    def cat(A, Bt):
        c = int((A.size(2) - Bt.size(2)) * 0.5)
        return torch.cat((F.pad(A, (-c, -c, -c, -c)), Bt), 1)

    t, skips = x, []
    for l in range(4):
        t = cr("conv%d1c" % (l + 1), "a1_%d" % l, t)
        t = cr("conv%d2c" % (l + 1), "a2_%d" % l, t)
        if l == 3:
            t = t * s                                                   # site 0
        t = pool(t, sels[l])
        skips.append(t)
    t = cr("conv51c", "a1_4", t)
    t = cr("conv52c", "a2_4", t) * s                                    # site 1
    for l in (3, 2, 1, 0):
        t = F.conv_transpose2d(t, p["upconv%d.weight" % (l + 1)], p["upconv%d.bias" % (l + 1)], stride=2)
        t = cat(skips[l], t)
        t = cr("conv%d1e" % (l + 1), "d1_%d" % l, t)
        t = cr("conv%d2e" % (l + 1), "d2_%d" % l, t)
    return F.conv2d(t, p["finalconv.weight"], p["finalconv.bias"])


def test_whole_net_gradients_on_hips_own_branch(hip):
    from oracle import parity, torch_ref
    h = hip.Handle(64, 0, math=-1)
    run = Step(hip, h, p=0.5, backward=True)
    masks, sels = parity.branch_of(h, run.ws, B, S)
    masks = dict(zip(parity.RELU_BUFS, masks))
    # the dropped elements are in the branch: whatever the reference flags drop is masked (the masks are NCHW)
    for site, buf in ((0, "a2_3"), (1, "a2_4")):
        mk = masks[buf].transpose(0, 2, 3, 1)
        keep = philox_ref.keep_flags(SEED, STEP, site, 0, mk.size, 0.5).reshape(mk.shape).astype(bool)
        assert not mk[~keep].any() and mk[keep].any(), buf
    params, x, dl = inputs()
    p64 = torch_ref.params_to_torch(params, torch.float64, requires_grad=True)
    ref = piecewise_linear(p64, torch.from_numpy(x).double(), masks, sels, 2.0)
    ref.backward(torch.from_numpy(dl).double())
    e_fwd = parity.nerr(run.logits.cpu().numpy(), ref.detach().numpy())
    errs = {k: parity.nerr(g.cpu().numpy(), p64[k].grad.numpy()) for k, g in zip(run.names, run.grads)}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print("drop-out, same branch: fwd %.3g, worst gradient %s %.3g" % (e_fwd, worst[0], worst[1]))
    assert len(errs) == 46
    assert e_fwd < FWD_TOL, e_fwd
    assert worst[1] < GRAD_TOL, worst


# ---- 5. the module ---------------------------------------------------------------------------------------------------------------
def make_net(**kw):
    import network
    params, _, _ = inputs()
    m = network.Unet(**kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return m.to("cuda:0")


def test_module_drops_only_on_training_forwards(hip):
    import tester
    _, x, _ = inputs()
    xd = torch.from_numpy(x).cuda()
    plain, net = make_net(), make_net(dropout=0.5, dropout_seed=9)
    net.train()
    state = net.dropout_state()
    y0 = net(xd).detach().clone()
    assert net.dropout_state() == {"p": 0.5, "seed": 9, "step": 1}
    y1 = net(xd).detach().clone()
    assert net.dropout_step == 2 and not torch.equal(y0, y1)
    net.load_dropout_state(state)
    assert torch.equal(net(xd).detach(), y0)                                  # the state reproduces the forward bit for bit
    want = plain(xd).detach()
    assert not torch.equal(y0, want)
    step = net.dropout_step
    with torch.no_grad():
        assert torch.equal(net(xd), want)                                     # validation inside training(...), tester.testing
    net.eval()
    assert torch.equal(net(xd).detach(), want)
    img = torch.rand(10, 14, generator=torch.Generator().manual_seed(1)).cuda()
    net.train()
    m_a, p_a = tester.segment(net, img, tile_size=188, return_probs=True)
    m_b, p_b = tester.segment(plain, img, tile_size=188, return_probs=True)
    assert torch.equal(m_a, m_b) and torch.equal(p_a, p_b)
    assert net.dropout_step == step                                           # none of these forwards drew a step
    # a backward through the dropped forward gives finite gradients for every parameter
    net.zero_grad(set_to_none=True)
    net(xd).sum().backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in net.parameters())


def test_checkpoint_resume_with_dropout_is_bit_exact(hip, tmp_path):
    """tests/test_net_gpu.py's resume test with drop-out on: two steps, save, two more == load, two steps."""
    import checkpoint
    import optim as hip_optim
    from oracle import prng
    _, x, _ = inputs()
    xd = torch.from_numpy(x).cuda()
    tgt = hip_optim.onehot2(torch.from_numpy(prng.make_labels(3, B, S - 184)), torch.empty(B, 2, S - 184, S - 184, device="cuda"))

    def steps(m, opt, n):
        m.train()
        for _ in range(n):
            opt.zero_grad(set_to_none=True)
            hip_optim.bce_with_logits(m(xd), tgt).backward()
            opt.step()

    def momentum(opt):
        return [opt.state_dict()["state"][i]["momentum_buffer"] for i in sorted(opt.state_dict()["state"])]

    a = make_net(dropout=0.5, dropout_seed=21); oa = hip_optim.SGD(a.parameters(), lr=1e-4, momentum=0.99)
    steps(a, oa, 2)
    path = checkpoint.save_checkpoint(os.path.join(tmp_path, "ck.pth"), a, oa, epoch=7)
    steps(a, oa, 2)
    b = make_net(dropout=0.5); ob = hip_optim.SGD(b.parameters(), lr=1e-4, momentum=0.99)
    assert checkpoint.load_checkpoint(path, b, ob)["epoch"] == 7
    assert b.dropout_state() == {"p": 0.5, "seed": 21, "step": 2}
    steps(b, ob, 2)
    assert a.dropout_state() == b.dropout_state() == {"p": 0.5, "seed": 21, "step": 4}
    assert all(torch.equal(q, r) for q, r in zip(a.parameters(), b.parameters()))
    assert all(torch.equal(q, r) for q, r in zip(momentum(oa), momentum(ob)))
    # without the state the resumed run draws the first two steps' masks again and is another run
    c = make_net(dropout=0.5, dropout_seed=21); oc = hip_optim.SGD(c.parameters(), lr=1e-4, momentum=0.99)
    checkpoint.load_checkpoint(path, c, oc)
    c.dropout_step = 0
    steps(c, oc, 2)
    assert any(not torch.equal(q, r) for q, r in zip(a.parameters(), c.parameters()))
