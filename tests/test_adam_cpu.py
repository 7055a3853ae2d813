"""tests/adam_ref.py itself, and the host side of Adam / AdamW / clip_grad_norm_, without a device: the fp64 reference is pinned
to torch.optim.Adam / AdamW and torch.nn.utils.clip_grad_norm_ in float64, the element-wise bound holds for the kernel's
arithmetic emulated in numpy fp32 (and for torch's other form of the first moment) and rejects the usual mistakes, and the
option checks of optim.Adam and trainer.check_optimizer_options raise before anything touches a device."""
import numpy as np
import pytest
import torch

import adam_ref as aref

SIZES = [1, 257, 0, 4099]
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
PIN = 2.0 ** -40            # fp64 order-of-operation differences only; 16 binary orders below the fp32 rounding (2^-24)


@pytest.mark.parametrize("decoupled,wd", [(False, 0.0), (False, 0.1), (True, 0.0), (True, 0.1)])
def test_reference_is_torch_adam_in_float64(decoupled, wd):
    """5 steps of adam_ref.update (scalars left in double) against torch.optim.Adam / AdamW on float64 CPU tensors: every
    element within 2^-40 of the tensor's largest |p|."""
    ps = [torch.from_numpy(p.astype(np.float64)).requires_grad_(True) for p in aref.make_params(SIZES)]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ps, weight_decay=wd, **HYPER)
    mine = [(p.detach().numpy().copy(), np.zeros(p.shape), np.zeros(p.shape)) for p in ps]
    for step in range(1, 6):
        gs = aref.make_grads(SIZES, step)
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        sc = aref.scalars(HYPER["lr"], HYPER["betas"], HYPER["eps"], wd, step, rounded=False)
        mine = [aref.update(p, m, v, g, sc, decoupled) for (p, m, v), g in zip(mine, gs)]
        for p, (q, m, v) in zip(ps, mine):
            if q.size:
                t = p.detach().numpy()
                assert np.abs(t - q).max() <= PIN * np.abs(t).max(), (step, np.abs(t - q).max())
                st = opt.state[p]
                assert np.abs(st["exp_avg"].numpy() - m).max() <= PIN * max(np.abs(m).max(), 1e-300)
                assert np.abs(st["exp_avg_sq"].numpy() - v).max() <= PIN * max(np.abs(v).max(), 1e-300)


@pytest.mark.parametrize("max_norm", [1e-3, 1.0, 1e9])
def test_norm_reference_is_torch_clip_grad_norm_in_float64(max_norm):
    gs = aref.make_grads(SIZES, 7)
    ps = [torch.zeros(n, dtype=torch.float64, requires_grad=True) for n in SIZES]
    for p, g in zip(ps, gs):
        p.grad = torch.from_numpy(g.astype(np.float64))
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    norm, coef = aref.grad_norm(gs, max_norm)
    assert abs(total - norm) <= PIN * total
    assert (coef < 1.0) == (max_norm < norm) and coef == min(1.0, max_norm / (norm + 1e-6))
    assert 1.0 < norm < 1e9                                                # so the three max_norm clip hard, clip, and do not clip
    for p, g in zip(ps, gs):
        if g.size:
            assert np.abs(p.grad.numpy() - g.astype(np.float64) * coef).max() <= PIN * np.abs(g).max()
    assert aref.grad_norm([np.zeros(5, np.float32)], 1.0) == (0.0, 1.0)
    assert aref.partial_count([1, 4095, 4096, 0, 4097, 8192, 70001]) == 1 + 1 + 1 + 0 + 2 + 2 + 18
    assert 2.0 ** -24 < aref.norm_rel_bound(24) < 1.02 * 2.0 ** -24


CASES = [(decoupled, wd, c) for decoupled in (False, True) for wd in (0.0, 0.1) for c in (None, 0.5)]


def run_variant(variant, decoupled, wd, c, steps=3):
    """`steps` updates of the emulated fp32 arithmetic beside the Tracker; returns the number of elements that left the bound."""
    state = [(p, np.zeros_like(p), np.zeros_like(p)) for p in aref.make_params(SIZES)]
    trackers = [aref.Tracker(p) for p, _, _ in state]
    for step in range(1, steps + 1):
        gs = aref.make_grads(SIZES, step, tiny=True)
        sc = aref.scalars(HYPER["lr"], HYPER["betas"], HYPER["eps"], wd, step)
        state = [aref.emulate(p, m, v, g, HYPER["lr"], HYPER["betas"], HYPER["eps"], wd, step, decoupled, c, variant)
                 for (p, m, v), g in zip(state, gs)]
        for t, g in zip(trackers, gs):
            want = aref.update(t.p, t.m, t.v, g, sc, decoupled, c)
            t.step(g, sc, decoupled, c)
            assert all(np.array_equal(a, b) for a, b in zip(want, (t.p, t.m, t.v)))      # the Tracker's values are update()'s
    return sum(t.misses(*s) for t, s in zip(trackers, state))


@pytest.mark.parametrize("decoupled,wd,c", CASES)
def test_bound_holds_for_both_legal_orders(decoupled, wd, c):
    """The stated order in numpy fp32, and the same with m = beta1 * m + om1 * g, stay inside the bound on every element of
    every input (gradients whose squares underflow included)."""
    assert run_variant("stated", decoupled, wd, c) == 0
    assert run_variant("mul_add", decoupled, wd, c) == 0


@pytest.mark.parametrize("variant", ["no_bias_correction", "eps_in_sqrt", "swapped_decay", "beta2_in_first_moment", "scale_ignored"])
def test_bound_rejects_wrong_updates(variant):
    """Each mistake leaves the bound on at least one element of the same inputs, in every case in which it changes anything
    (a swapped decay needs wd != 0, an ignored scale a scale)."""
    for decoupled, wd, c in CASES:
        if (variant == "swapped_decay" and wd == 0.0) or (variant == "scale_ignored" and c is None):
            continue
        assert run_variant(variant, decoupled, wd, c) > 0, (variant, decoupled, wd, c)


def test_bound_at_a_late_step():
    """step = 100000: both corrections round to 1 (step_size = lr, rbc2 = 1); the emulation stays inside."""
    sc = aref.scalars(1e-3, (0.9, 0.999), 1e-8, 0.0, 100000)
    assert sc.step_size == aref.f32(1e-3) and sc.rbc2 == 1.0
    ps, gs = aref.make_params(SIZES), aref.make_grads(SIZES, 3)
    for p, g in zip(ps, gs):
        m0, v0 = np.abs(g) * np.float32(0.5), g * g
        t = aref.Tracker(p)
        t.m[:] = m0; t.v[:] = v0
        t.step(g, sc, False)
        assert t.misses(*aref.emulate(p, m0, v0, g, 1e-3, (0.9, 0.999), 1e-8, 0.0, 100000, False)) == 0


def test_adam_constructor_value_errors():
    import optim
    w = [torch.zeros(3, requires_grad=True)]
    for kw in (dict(eps=0.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)), dict(betas=(-0.1, 0.9)), dict(lr=-1e-3),
               dict(weight_decay=-0.1), dict(betas=0.9), dict(eps=float("nan"))):
        for cls in (optim.Adam, optim.AdamW):
            with pytest.raises(ValueError):
                cls(w, **kw)
    a = optim.Adam(w)
    assert a.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False)
    b = optim.AdamW(w)
    assert b.defaults["decoupled"] is True and b.defaults["weight_decay"] == 1e-2
    assert isinstance(b, optim.Adam) and isinstance(a, torch.optim.Optimizer)
    w[0].grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):               # host tensors raise, and leave no state behind
        a.step()
    assert len(a.state) == 0 or "step" not in a.state[w[0]]
    with pytest.raises(ValueError):
        optim.clip_grad_norm_(w, 0.0)
    with pytest.raises(ValueError):
        optim.clip_grad_norm_([torch.zeros(2, requires_grad=True)], 1.0)     # no gradient anywhere


def test_check_optimizer_options():
    import trainer
    assert trainer.check_optimizer_options() == dict(lr=0.0001, momentum=0.99)
    assert trainer.check_optimizer_options("adam") == dict(lr=0.0001)
    assert trainer.check_optimizer_options("adamw", dict(weight_decay=0.05, betas=(0.8, 0.9)), 1.0) == dict(lr=0.0001, weight_decay=0.05,
                                                                                                             betas=(0.8, 0.9))
    assert trainer.check_optimizer_options("sgd", dict(lr=0.01)) == dict(lr=0.01, momentum=0.99)
    for args in (("rmsprop",), ("adam", dict(momentum=0.9)), ("sgd", dict(betas=(0.9, 0.99))), ("adam", dict(amsgrad=True)),
                 ("adam", dict(eps=0.0)), ("adamw", dict(betas=(0.9, 1.0))), ("adam", dict(lr=-1.0)), ("adamw", dict(weight_decay=-1.0)),
                 ("sgd", dict(momentum=-0.5)), ("sgd", None, 0.0), ("adam", None, -1.0), ("adam", None, "1"), ("sgd", None, float("inf"))):
        with pytest.raises(ValueError):
            trainer.check_optimizer_options(*args)
