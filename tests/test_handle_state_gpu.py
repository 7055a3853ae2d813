"""What a handle keeps BETWEEN calls: the plans of training forwards (csrc/plans.hpp, keyed by workspace address), through
the C ABI on buffers the test owns (gpu_support.Net, tests/guarded.py: every pointer a poisoned, guarded buffer, every
workspace of exactly unet_workspace_bytes(...) bytes) and through network.Unet, whose instances share one handle per
(device, base_ch, n_classes).  Everything runs at S = 188, the smallest size, with (1, 220) as the second shape, B <= 2.

The reference of every case is the same step run ALONE: a fresh handle, a fresh workspace, nothing pending (alone()).  The
library is deterministic (tests/test_workspace_gpu.py relies on it), so logits, the 46 gradients and dx are compared bit
for bit.  N identical wrong answers must not pass: per arithmetic mode one case also holds the logits to the fp64 torch
restatement at test_workspace_gpu.FWD_TOL[mode].

  a  two forwards of different shape pending on one handle, their backwards in both orders
  b  pending plans of different arithmetic (a math=-1 handle) and of different drop-out probability
  c  17 forwards pending at once (one more than the finished plans a handle keeps), and one pending forward that waits
     while 16 whole steps run on 16 other live workspaces
  d  a repeated backward: all stages and unet_backward_input twice with no forward in between.  DECIDED BY THE RUN: the
     second backward gives the same bits as the first (every gradient buffer of the workspace is rewritten before it is
     scaled or read), plain and with drop-out p = 0.5, with the weight gradients on the caller's stream and on the
     auxiliary one.  That is what is pinned here and what include/unet_hip.h promises.
  e  refusals: UNET_E_NOTREADY for a workspace no forward ran on, the right workspace at address + 256, another handle's
     pending workspace, and a workspace whose training forward was followed by an inference forward; UNET_E_BADARG for a
     workspace_bytes one byte short.  Nothing is written, and the handle still computes the right step afterwards.
  f  two handles interleaved, one destroyed while the other has a forward pending
  g  knobs between a forward and its backward: lds_dma and overlap (bit-identical but for the fp32 up-conv weight / bias
     gradient the header names, held to 2e-5 against fp64 as in tests/test_kernel_paths_gpu.py), and grad_scale 0.5,
     read when the backward runs (every gradient exactly half)
  h  network.Unet: two modules on the shared handle interleaved, 17 outputs pending, an inference forward in between, and
     the second backward() through one graph, which raises instead of handing the library a null workspace."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded as gd
from gpu_support import Net, library_state, nerr, rejected
from test_workspace_gpu import FWD_TOL

pytestmark = pytest.mark.gpu

X, Y = (2, 188), (1, 220)
NOTREADY, BADARG = -3, -2
N_PENDING = 17                      # the smallest count above the 16 finished plans a handle keeps (the cap on ALL plans before)
UP_TOL = 2e-5                       # fp32 up-conv weight / bias gradient against fp64 (tests/test_kernel_paths_gpu.py)


def names_of(net):
    return ["logits"] + ["grad %s" % k for k in net.params] + ["dx"]


def params_for(base, K, pseed):
    import multiclass_ref as ref
    return ref.head_params(K, base=base, seed=pseed)


def workspace(net, B, S, training=1):
    """(arena, workspace, bytes): exactly unet_workspace_bytes(B, S, training) usable bytes between guards, all poison."""
    nbytes = net.h.workspace_bytes(B, S, training)
    wsa = gd.Arena()
    ws = wsa.scratch(nbytes, "workspace of exactly unet_workspace_bytes(%d, %d, %d)" % (B, S, training))
    assert wsa.address(ws) % 256 == 0
    return wsa, ws, nbytes


def cpu(outs):
    return [t.cpu() for t in outs]


_alone = {}
_f64 = {}


@pytest.fixture(scope="module", autouse=True)
def shared_references():
    """The references are shared by the tests of this module and dropped with it."""
    yield
    _alone.clear()
    _f64.clear()


def alone(mode, base, K, B, S, seed=0, dropout=None, pseed=0):
    """[logits, 46 gradients, dx] (cpu) of the step run alone: fresh handle of arithmetic `mode`, fresh workspace, inputs of
    `seed`, parameters of `pseed`.  Computed once per configuration and shared; nobody changes it."""
    key = (mode, base, K, B, S, seed, dropout, pseed)
    if key not in _alone:
        net = Net(mode, base, K, params_for(base, K, pseed))
        wsa, ws, nbytes = workspace(net, B, S)
        x, dl = net.inputs(B, S, seed)
        A = gd.Arena()
        outs = [net.forward(A, wsa, ws, nbytes, x, 1, dropout)] + net.backward(A, wsa, ws, nbytes, dl)
        _alone[key] = cpu(outs)
        for t in _alone[key]:
            assert not torch.isnan(t).any()
    return _alone[key]


def same_bits(got, want, names, what):
    assert len(got) == len(want) <= len(names)
    for n, a, b in zip(names, got, want):
        a = a.cpu()
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), \
            "%s: %s differs from the step run alone in %d of %d elements, max |d| %.3g" % (
                what, n, int((a != b).sum()), a.numel(), float((a.double() - b.double()).abs().max()))


def fp64(base, K, B, S, grads=False):
    """The fp64 torch restatement on the inputs of seed 0: (logits, {name: gradient}) - gradients only with grads=True."""
    from oracle import prng, torch_ref
    key = (base, K, B, S)
    if key not in _f64 or (grads and _f64[key][1] is None):
        p = torch_ref.params_to_torch(params_for(base, K, 0), dtype=torch.float64, requires_grad=grads)
        x = torch.from_numpy(prng.make_input(1, B, S)).double()
        with torch.enable_grad() if grads else torch.no_grad():
            y = torch_ref.unet_forward(p, x)
            if grads:
                y.backward(torch.from_numpy(prng.make_cotangent(2, (B, K, S - 184, S - 184))).double())
        _f64[key] = (y.detach().numpy(), {k: v.grad.numpy() for k, v in p.items()} if grads else None)
    return _f64[key]


def logits_are_right(mode, base, K, B, S, logits):
    e = nerr(logits, fp64(base, K, B, S)[0])
    print("mode %d base %d K=%d B=%d S=%d: logits %.3g from fp64 (tolerance %.3g)" % (mode, base, K, B, S, e, FWD_TOL[mode]))
    assert e < FWD_TOL[mode]


# ---- a: two pending, both backward orders -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,base,K", [(3, 64, 2), (2, 64, 2), (3, 32, 2), (3, 64, 3)])
def test_two_pending_forwards_backward_in_both_orders(mode, base, K):
    net = Net(mode, base, K)
    names = names_of(net)
    want = {s: alone(mode, base, K, *s) for s in (X, Y)}
    logits_are_right(mode, base, K, *X, want[X][0])
    for order in ((X, Y), (Y, X)):
        run, got = {}, {}
        for s in (X, Y):                                        # both forwards first: two plans pending on one handle
            wsa, ws, nbytes = workspace(net, *s)
            x, dl = net.inputs(*s)
            A = gd.Arena()
            run[s] = (A, wsa, ws, nbytes, dl)
            got[s] = [net.forward(A, wsa, ws, nbytes, x, 1)]
        for s in order:
            A, wsa, ws, nbytes, dl = run[s]
            got[s] += net.backward(A, wsa, ws, nbytes, dl)
        for s in (X, Y):
            run[s][1].check()                                   # the other plan's backward wrote nothing around this workspace
            same_bits(got[s], want[s], names, "(B, S) = %s, backward order %s" % (s, order))


# ---- b: mixed plans on one handle -------------------------------------------------------------------------------------------
def test_pending_plans_of_different_arithmetic_on_a_default_mode_handle():
    net = Net(-1, 64, 2)
    names = names_of(net)
    with library_state() as set_knobs:
        set_knobs(math=3)
        wx = workspace(net, *X)
        x, dlx = net.inputs(*X)
        Ax = gd.Arena()
        got_x = [net.forward(Ax, *wx, x, 1)]
        fp32_bytes_of_y = net.h.workspace_bytes(*Y, 1)
        set_knobs(math=2)                                       # bf16 tensors: another layout in a smaller workspace
        wy = workspace(net, *Y)
        assert wy[2] < fp32_bytes_of_y
        y, dly = net.inputs(*Y)
        Ay = gd.Arena()
        got_y = [net.forward(Ay, *wy, y, 1)]
        set_knobs(math=0)                                       # the backward of a forward keeps that forward's arithmetic
        got_x += net.backward(Ax, *wx, dlx)
        got_y += net.backward(Ay, *wy, dly)
    same_bits(got_x, alone(3, 64, 2, *X), names, "the mode 3 forward, backward with the default at 0")
    same_bits(got_y, alone(2, 64, 2, *Y), names, "the mode 2 forward, backward with the default at 0")
    assert not torch.equal(alone(2, 64, 2, *Y)[0], alone(3, 64, 2, *Y)[0])       # the two arithmetics do tell apart


def test_pending_plans_of_different_dropout_probability():
    drop = (0.5, 20240607, 3)
    net = Net(3, 64, 2)
    names = names_of(net)
    x, dl = net.inputs(*X)
    wd, wp = workspace(net, *X), workspace(net, *X)
    Ad, Ap = gd.Arena(), gd.Arena()
    got_d = [net.forward(Ad, *wd, x, 1, drop)]
    got_p = [net.forward(Ap, *wp, x, 1)]
    got_d += net.backward(Ad, *wd, dl)                          # each backward scales by its own plan's 1 / (1 - p)
    got_p += net.backward(Ap, *wp, dl)
    want_d, want_p = alone(3, 64, 2, *X, dropout=drop), alone(3, 64, 2, *X)
    same_bits(got_d, want_d, names, "p = 0.5 with a plain forward pending")
    same_bits(got_p, want_p, names, "the plain forward with a p = 0.5 forward pending")
    assert sum(not torch.equal(a, b) for a, b in zip(want_d, want_p)) > 40           # drop-out does change the step


# ---- c: more pending than the 16 finished plans a handle keeps --------------------------------------------------------------
def test_seventeen_forwards_pending_at_once():
    net = Net(3, 32, 2)
    names = names_of(net)
    runs = []
    for i in range(N_PENDING):
        wsa, ws, nbytes = workspace(net, 1, 188)
        x, dl = net.inputs(1, 188, seed=i)
        A = gd.Arena()
        runs.append((A, wsa, ws, nbytes, dl, net.forward(A, wsa, ws, nbytes, x, 1)))
    print("base 32, (B, S) = (1, 188): %d bytes per training workspace, %d workspaces alive" % (runs[0][3], len(runs)))
    assert len({r[1].address(r[2]) for r in runs}) == N_PENDING
    for i in reversed(range(N_PENDING)):
        A, wsa, ws, nbytes, dl, logits = runs[i]
        got = [logits] + net.backward(A, wsa, ws, nbytes, dl)
        same_bits(got, alone(3, 32, 2, 1, 188, seed=i), names, "workspace %d of %d pending" % (i, N_PENDING))
    for r in runs:
        r[1].check()
    logits_are_right(3, 32, 2, 1, 188, alone(3, 32, 2, 1, 188)[0])


def test_a_pending_forward_outlives_sixteen_finished_steps():
    net = Net(3, 32, 2)
    names = names_of(net)
    wsa, ws, nbytes = workspace(net, 1, 188)
    x, dl = net.inputs(1, 188, seed=0)
    A = gd.Arena()
    logits = net.forward(A, wsa, ws, nbytes, x, 1)
    others = []                                                 # kept alive: 16 other addresses
    for i in range(1, N_PENDING):
        o = workspace(net, 1, 188)
        xi, dli = net.inputs(1, 188, seed=i)
        others.append(o)
        same_bits(net.step(gd.Arena(), *o, xi, dli, 1), alone(3, 32, 2, 1, 188, seed=i), names, "finished step %d" % i)
    assert len({o[0].address(o[1]) for o in others} | {wsa.address(ws)}) == N_PENDING
    got = [logits] + net.backward(A, wsa, ws, nbytes, dl)
    same_bits(got, alone(3, 32, 2, 1, 188, seed=0), names, "the first forward's backward after 16 finished steps")


# ---- d: a repeated backward -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("dropout", [None, (0.5, 20240607, 3)], ids=["plain", "p=0.5"])
def test_a_repeated_backward_gives_the_same_bits(dropout, overlap):
    net = Net(3, 64, 2)
    names = names_of(net)
    want = alone(3, 64, 2, *X, dropout=dropout)
    with library_state(overlap=overlap):
        w = workspace(net, *X)
        x, dl = net.inputs(*X)
        A = gd.Arena()
        logits = net.forward(A, *w, x, 1, dropout)
        first = net.backward(A, *w, dl)
        second = net.backward(gd.Arena(), *w, dl)               # no forward in between; other output buffers
    same_bits([logits] + first, want, names, "the first backward")
    same_bits([logits] + second, want, names, "the second backward of the same forward")


# ---- e: refusals ------------------------------------------------------------------------------------------------------------
def refused(net, wsp, nbytes, dl, code, *words):
    """Every backward stage and unet_backward_input on `wsp` return `code`, say why, and write nothing."""
    hip, L = net.hip, net.L
    A = gd.Arena()
    grads = [A.out(p.shape, torch.float32, "grad %s" % k) for k, p in zip(net.params, net.plist)]
    gtab = hip.ptr_table(grads)
    B, S = dl.shape[0], dl.shape[2] + 184
    dx = A.out((B, 1, S, S), torch.float32, "dx")
    calls = [("unet_backward_stage %d" % s, lambda s=s: L.unet_backward_stage(net.h.h, s, net.ptab, hip.ptr(dl), gtab, wsp, nbytes, hip.stream()))
             for s in range(L.unet_backward_stages())]
    calls.append(("unet_backward", lambda: L.unet_backward(net.h.h, net.ptab, hip.ptr(dl), gtab, wsp, nbytes, hip.stream())))
    calls.append(("unet_backward_input", lambda: L.unet_backward_input(net.h.h, net.ptab, hip.ptr(dx), wsp, nbytes, hip.stream())))
    for what, call in calls:
        rc = call()
        msg = L.unet_last_error().decode()
        assert rc == code, "%s returned rc == %d, expected %d (%s)" % (what, rc, code, msg)
        for w in words:
            assert w in msg, "%s: the error does not name the cause (%r): %s" % (what, w, msg)
        rejected(hip, rc, A, dx, *grads)
    net.keep.check()


def then_a_correct_step(net, seed=1):
    w = workspace(net, 1, 188)
    x, dl = net.inputs(1, 188, seed=seed)
    same_bits(net.step(gd.Arena(), *w, x, dl, 1), alone(3, 32, 2, 1, 188, seed=seed), names_of(net), "the step after the refusal")


WHY = ("training forward", "workspace")


def test_backward_on_a_workspace_no_forward_ran_on_is_refused():
    net = Net(3, 32, 2)
    wsa, ws, nbytes = workspace(net, 1, 188)
    _, dl = net.inputs(1, 188)
    refused(net, wsa.ptr(ws), nbytes, dl, NOTREADY, *WHY)
    assert bool((ws == gd.POISON).all())
    wsa.check()
    then_a_correct_step(net)


def test_backward_at_another_address_of_the_right_workspace_is_refused():
    net = Net(3, 32, 2)
    wsa, ws, nbytes = workspace(net, 1, 188)
    x, dl = net.inputs(1, 188)
    A = gd.Arena()
    logits = net.forward(A, wsa, ws, nbytes, x, 1)
    before = ws.clone()
    refused(net, C.c_void_p(wsa.address(ws) + 256), nbytes, dl, NOTREADY, *WHY)
    assert torch.equal(ws, before)
    wsa.check()
    # the forward is still pending at its own address
    same_bits([logits] + net.backward(A, wsa, ws, nbytes, dl), alone(3, 32, 2, 1, 188), names_of(net), "the backward at the right address")
    then_a_correct_step(net)


def test_backward_on_another_handles_pending_workspace_is_refused():
    net, other = Net(3, 32, 2), Net(3, 32, 2)                    # plans are per handle
    wsa, ws, nbytes = workspace(other, 1, 188)
    x, dl = other.inputs(1, 188)
    A = gd.Arena()
    logits = other.forward(A, wsa, ws, nbytes, x, 1)
    before = ws.clone()
    refused(net, wsa.ptr(ws), nbytes, dl, NOTREADY, *WHY)
    assert torch.equal(ws, before)
    wsa.check()
    same_bits([logits] + other.backward(A, wsa, ws, nbytes, dl), alone(3, 32, 2, 1, 188), names_of(other), "the owner's backward")
    then_a_correct_step(net)


def test_backward_after_an_inference_forward_on_the_workspace_is_refused():
    """A training forward on P, then unet_forward(training=0) on P: P holds an inference layout, and the training plan is void.
    (The buffer is the training plan's own, so a library that ran the backward all the same would stay inside it.)"""
    net = Net(3, 32, 2)
    wsa, ws, nbytes = workspace(net, 1, 188)
    x, dl = net.inputs(1, 188)
    A = gd.Arena()
    net.forward(A, wsa, ws, nbytes, x, 1)
    net.forward(A, wsa, ws, nbytes, x, 0)
    before = ws.clone()
    refused(net, wsa.ptr(ws), nbytes, dl, NOTREADY, *WHY)
    assert torch.equal(ws, before)
    wsa.check()
    # a new training forward on P plans it again
    same_bits(net.step(gd.Arena(), wsa, ws, nbytes, x, dl, 1), alone(3, 32, 2, 1, 188), names_of(net), "a new step on the same workspace")
    then_a_correct_step(net)


def test_backward_with_workspace_bytes_one_short_is_refused():
    net = Net(3, 32, 2)
    wsa, ws, nbytes = workspace(net, 1, 188)
    x, dl = net.inputs(1, 188)
    A = gd.Arena()
    logits = net.forward(A, wsa, ws, nbytes, x, 1)
    before = ws.clone()
    refused(net, wsa.ptr(ws), nbytes - 1, dl, BADARG, "workspace too small")
    assert torch.equal(ws, before)
    wsa.check()
    same_bits([logits] + net.backward(A, wsa, ws, nbytes, dl), alone(3, 32, 2, 1, 188), names_of(net), "the backward with all its bytes")
    then_a_correct_step(net)


# ---- f: two handles interleaved ---------------------------------------------------------------------------------------------
def test_a_handle_destroyed_while_another_has_a_forward_pending():
    a, b = Net(3, 64, 2), Net(3, 32, 3)
    wa, wb = workspace(a, *X), workspace(b, *X)
    xa, dla = a.inputs(*X)
    xb, dlb = b.inputs(*X)
    Aa, Ab = gd.Arena(), gd.Arena()
    got_a = [a.forward(Aa, *wa, xa, 1)]
    got_b = [b.forward(Ab, *wb, xb, 1)]
    got_b += b.backward(Ab, *wb, dlb)
    same_bits(got_b, alone(3, 32, 3, *X), names_of(b), "handle B between A's forward and backward")
    torch.cuda.synchronize()
    b.h.__del__()                                               # unet_destroy now, not when the collector gets to it
    assert not b.h.h
    got_a += a.backward(Aa, *wa, dla)
    same_bits(got_a, alone(3, 64, 2, *X), names_of(a), "handle A around the life of handle B")


# ---- g: knobs between forward and backward ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [3, 0, 2])
def test_staging_and_overlap_flipped_between_forward_and_backward(mode):
    net = Net(mode, 64, 2)
    names = names_of(net)
    want = alone(mode, 64, 2, *X)                               # the defaults throughout: lds_dma 1, overlap by mode
    logits_are_right(mode, 64, 2, *X, want[0])
    with library_state(lds_dma=1, overlap=0) as set_knobs:
        w = workspace(net, *X)
        x, dl = net.inputs(*X)
        A = gd.Arena()
        got = [net.forward(A, *w, x, 1)]
        set_knobs(lds_dma=0, overlap=1)
        got += net.backward(A, *w, dl)
    # the one exception include/unet_hip.h names: the fp32 up-conv weight and bias gradient sums in another order at lds_dma 0
    loose = {"grad upconv%d.%s" % (l, t) for l in (1, 2, 3, 4) for t in ("weight", "bias")} if mode in (0, 3) else set()
    assert loose <= set(names)
    strict = [i for i, n in enumerate(names) if n not in loose]
    same_bits([got[i] for i in strict], [want[i] for i in strict], [names[i] for i in strict], "mode %d, knobs flipped after the forward" % mode)
    if loose:
        g64 = fp64(64, 2, *X, grads=True)[1]
        for i, n in enumerate(names):
            if n in loose:
                e_flip, e_plain = nerr(got[i], g64[n[5:]]), nerr(want[i], g64[n[5:]])
                print("mode %d %s: %.3g from fp64 with the knobs flipped, %.3g without (tolerance %.3g); %s" % (
                    mode, n, e_flip, e_plain, UP_TOL, "bit-identical" if torch.equal(got[i].cpu(), want[i]) else "other rounding"))
                assert e_flip < UP_TOL and e_plain < UP_TOL


@pytest.mark.parametrize("mode", [3, 2])
def test_grad_scale_is_read_when_the_backward_runs(mode):
    net = Net(mode, 64, 2)
    names = names_of(net)
    want = alone(mode, 64, 2, *X)                               # grad_scale 1
    w = workspace(net, *X)
    x, dl = net.inputs(*X)
    A = gd.Arena()
    got = [net.forward(A, *w, x, 1)]
    net.hip.check(net.L.unet_set_grad_scale(net.h.h, 0.5), "unet_set_grad_scale")
    got += net.backward(A, *w, dl)
    # a power of two is exact in fp32 and in bf16 as long as nothing turns denormal: every gradient is exactly half
    half = [want[0]] + [t * 0.5 for t in want[1:]]
    tiny = float(np.finfo(np.float32).tiny)
    for n, t in zip(names[1:], half[1:]):
        assert int(((t != 0) & (t.abs() < tiny)).sum()) == 0, "%s: halving makes denormals, the equality would not be exact" % n
        assert float(t.abs().max()) > 0
    same_bits(got, half, names, "mode %d, grad_scale 0.5 set after the forward" % mode)


# ---- h: through the module --------------------------------------------------------------------------------------------------
def module(pseed, base=32):
    import network
    m = network.Unet(base_ch=base)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params_for(base, 2, pseed).items()})
    return m.to("cuda:0").train()


def module_inputs(B, S, seed=0):
    from oracle import prng
    return (torch.from_numpy(prng.make_input(1 + 10 * seed, B, S)).cuda(),
            torch.from_numpy(prng.make_cotangent(2 + 10 * seed, (B, 2, S - 184, S - 184))).cuda())


def module_names():
    return ["logits"] + ["grad %s" % k for k in params_for(32, 2, 0)]      # no dx: the image asks for no gradient


def default_mode():
    import _hip
    return _hip.lib().unet_get_math()


def test_two_modules_interleaved_on_the_shared_handle():
    m1, m2 = module(0), module(5)
    assert m1._get_handle(0) is m2._get_handle(0)
    mode = default_mode()
    names = module_names()
    x1, dl1 = module_inputs(*X)
    x2, dl2 = module_inputs(*Y)
    y1 = m1(x1)
    y2 = m2(x2)
    y2.backward(dl2)
    y1.backward(dl1)
    torch.cuda.synchronize()
    same_bits([y1.detach()] + [p.grad for p in m1.parameters()], alone(mode, 32, 2, *X)[:-1], names, "module 1, its backward last")
    same_bits([y2.detach()] + [p.grad for p in m2.parameters()], alone(mode, 32, 2, *Y, pseed=5)[:-1], names, "module 2, its backward first")
    assert not torch.equal(alone(mode, 32, 2, *Y, pseed=5)[0], alone(mode, 32, 2, *Y)[0])


def test_seventeen_outputs_of_one_module_pending():
    m = module(0)
    mode = default_mode()
    names = module_names()
    params = list(m.parameters())
    pend = []
    for i in range(N_PENDING):
        x, dl = module_inputs(1, 188, seed=i)
        pend.append((m(x), dl))
    for i in reversed(range(N_PENDING)):
        y, dl = pend[i]
        grads = torch.autograd.grad(y, params, dl)
        same_bits([y.detach()] + list(grads), alone(mode, 32, 2, 1, 188, seed=i)[:-1], names, "output %d of %d pending" % (i, N_PENDING))


def test_an_inference_forward_between_a_forward_and_its_backward():
    m = module(0)
    mode = default_mode()
    names = module_names()
    x, dl = module_inputs(*X)
    xo, _ = module_inputs(*Y)
    y = m(x)
    with torch.no_grad():
        assert torch.equal(m(x), y) and m(xo).shape == (1, 2, 36, 36)
    y.backward(dl)
    same_bits([y.detach()] + [p.grad for p in m.parameters()], alone(mode, 32, 2, *X)[:-1], names, "a no_grad forward in between")


def test_a_second_backward_through_one_graph_raises():
    m = module(0)
    x, dl = module_inputs(1, 188)
    y = m(x)
    y.backward(dl, retain_graph=True)
    torch.cuda.synchronize()
    first = [p.grad.clone() for p in m.parameters()]
    with pytest.raises(RuntimeError, match="workspace of this forward was released by its first backward"):
        y.backward(dl)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), p.grad.view(torch.int32)) for a, p in zip(first, m.parameters()))
    same_bits([y.detach()] + first, alone(default_mode(), 32, 2, 1, 188)[:-1], module_names(), "the first backward")
