"""optim.Adam / AdamW, optim.clip_grad_norm_ and trainer.training(optimizer=..., clip_grad_norm=...) on the whole net at S = 188,
B = 2: one real step against the fp64 reference of tests/adam_ref.py, the trainer against the same epochs written out over the
public ops, checkpoint and resume, and the untouched defaults."""
import copy
import os

import numpy as np
import pytest
import torch

import adam_ref as aref
from gpu_support import dev
from test_multiclass_gpu import knet

pytestmark = pytest.mark.gpu

S, B, K = 188, 2, 3


def small_net(dev):
    """The K-class net at base_ch = 32 (a quarter of the parameters, the same 46 tensors) for the tests that write checkpoints."""
    return knet(K, dev, base=32)


def loader(seed, n):
    """n batches of images [B,1,S,S] and labels [B,1,4,4] in [0, K), most of them background (sparse foreground)."""
    from oracle import prng
    rs = np.random.RandomState(seed)
    return [(torch.from_numpy(prng.make_input(seed * 10 + i, B, S)),
             torch.from_numpy((rs.randint(0, K, (B, 1, 4, 4)) * (rs.rand(B, 1, 4, 4) < 0.4)).astype(np.int64))) for i in range(n)]


@pytest.mark.parametrize("cls,wd,base", [("Adam", 0.01, 32), ("AdamW", 0.01, 64)])
def test_one_real_step_matches_the_reference(dev, cls, wd, base):
    """forward, softmax_ce_step, backward, step(): the fp64 reference applied to the gradients and the old parameters read back
    reproduces all 46 tensors, and their moments, inside the element-wise bound (the real shapes, the Python chunking).  One
    step, and Adam on the base_ch = 32 net: the reference walks every element (31 M at base_ch = 64) in fp64 on the host; later
    steps are test_step_skips_...'s and the per-op tests'."""
    import optim
    net = knet(K, dev, base=base)
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    opt = getattr(optim, cls)(net.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=wd)
    params = list(net.parameters())
    assert len(params) == 46
    trackers = [aref.Tracker(p.detach().cpu().numpy()) for p in params]
    for step, (images, labels) in enumerate(loader(3, 1), 1):
        opt.zero_grad()
        loss, _ = optim.softmax_ce_step(net(images.to(dev)), labels.to(dev), want_mask=False)
        loss.backward()
        grads = [p.grad.cpu().numpy().copy() for p in params]
        opt.step()
        sc = aref.scalars(lr, betas, eps, wd, step)
        worst = 0.0
        for p, g, tr in zip(params, grads, trackers):
            st = opt.state[p]
            assert st["step"] == step and type(st["step"]) is int
            got = [t.detach().cpu().numpy() for t in (p, st["exp_avg"], st["exp_avg_sq"])]
            tr.step(g, sc, cls == "AdamW")
            assert tr.misses(*got) == 0, (step, tuple(p.shape), tr.worst(*got))
            worst = max(worst, *tr.worst(*got))
        assert any(np.abs(g).max() > 0 for g in grads)
        print("%s wd=%g step %d: max err / bound %.3g" % (cls, wd, step, worst))


def test_step_skips_parameters_without_gradient_and_groups_by_step(dev):
    """A parameter whose grad is None is skipped (no state); one that joins later starts at step 1 beside the others' step 2."""
    import optim
    a = torch.nn.Parameter(torch.randn(5000, device=dev)); b = torch.nn.Parameter(torch.randn(300, device=dev))
    a0, b0 = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    opt = optim.Adam([a, b], lr=1e-2)
    ga, gb = torch.randn(5000, device=dev), torch.randn(300, device=dev)
    a.grad = ga
    opt.step()
    assert opt.state[a]["step"] == 1 and len(opt.state[b]) == 0 and np.array_equal(b.detach().cpu().numpy(), b0)
    b.grad = gb
    opt.step()
    assert opt.state[a]["step"] == 2 and opt.state[b]["step"] == 1
    ta, tb = aref.Tracker(a0), aref.Tracker(b0)
    for step in (1, 2):
        ta.step(ga.cpu().numpy(), aref.scalars(1e-2, (0.9, 0.999), 1e-8, 0.0, step), False)
    tb.step(gb.cpu().numpy(), aref.scalars(1e-2, (0.9, 0.999), 1e-8, 0.0, 1), False)
    for p, t in ((a, ta), (b, tb)):
        st = opt.state[p]
        assert t.misses(p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()) == 0


def test_clip_grad_norm_matches_torch_and_scales_in_place(dev):
    """48 gradients (two sum-of-squares launches): the norm within the derived bound of torch's float64 one, both results 0-dim
    views of one [2] buffer, scale=True scales in place by the fp32 coefficient exactly, scale=False leaves the gradients."""
    import optim
    sizes = [(61 * i) % 900 + 1 for i in range(47)] + [9001]
    ps = [torch.nn.Parameter(torch.zeros(n, device=dev)) for n in sizes] + [torch.nn.Parameter(torch.zeros(3, device=dev))]
    gs = aref.make_grads(sizes, 5)
    for p, g in zip(ps, gs):
        p.grad = torch.from_numpy(g).to(dev)                                  # the last parameter has no gradient
    norm64, _ = aref.grad_norm(gs, 1.0)
    for max_norm in (0.25 * norm64, 4.0 * norm64):
        norm, coef = optim.clip_grad_norm_(ps, max_norm, scale=False)
        assert norm.dim() == 0 and coef.dim() == 0 and norm.dtype == torch.float32 and norm.is_cuda
        assert coef.data_ptr() == norm.data_ptr() + 4
        assert all(np.array_equal(p.grad.cpu().numpy(), g) for p, g in zip(ps, gs))
        n32 = np.float32(norm.item())
        assert abs(float(n32) - norm64) <= aref.norm_rel_bound(aref.partial_count(sizes)) * norm64
        assert np.float32(coef.item()) == aref.coef_fp32(n32, max_norm)
        assert (coef.item() < 1.0) == (max_norm < norm64)
    norm, coef = optim.clip_grad_norm_(ps, 0.25 * norm64)
    c32 = np.float32(coef.item())
    assert c32 < 1 and all(np.array_equal(p.grad.cpu().numpy(), g * c32) for p, g in zip(ps, gs))


def hand_loop(net, train, val, dev, epochs, max_norm, **adamw):
    """The trainer's epochs written out over the public ops: forward, dice_step (CE + Dice), backward, clip_grad_norm_ without
    the in-place scale, AdamW.step(grad_scale=coef).  Returns the two loss series and every step's (norm, coef)."""
    import optim
    opt = optim.AdamW(net.parameters(), **adamw)
    losses, vlosses, clips = [], [], []

    def step_loss(images, labels):
        return optim.dice_step(net(images.to(dev)), labels.to(dev), ce_weight=1.0, dice_weight=1.0, want_mask=False)[0]

    for _ in range(epochs):
        tot = 0
        for images, labels in train:
            opt.zero_grad()
            loss = step_loss(images, labels)
            loss.backward()
            norm, coef = optim.clip_grad_norm_(net.parameters(), max_norm, scale=False)
            opt.step(grad_scale=coef)
            clips.append((norm.clone(), coef.clone()))
            tot += loss.detach()
        vt = 0
        with torch.no_grad():
            for images, labels in val:
                vt += step_loss(images, labels)
        losses.append((tot / (len(train) * B)).item())
        vlosses.append((vt / (len(val) * B)).item())
    return np.array(losses, np.float64), np.array(vlosses, np.float64), [(n.item(), c.item()) for n, c in clips]


# The gradient norms of the four steps of the loop below are about 1750, 21700, 1490 and 655 (printed by the test; read from a
# run at max_norm = 1, and Adam's update hardly depends on the scale of the gradient): 1000 clips the first three steps, not the last
MAX_NORM = 1000.0


def test_training_adamw_with_clipping_matches_hand_loop(dev, tmp_path):
    """training(optimizer='adamw', clip_grad_norm=MAX_NORM, loss='ce_dice') for 2 epochs of 2 batches: the weights and the loss
    series equal, bit for bit, the hand-written loop; MAX_NORM clips in at least one step and not in at least one other."""
    import trainer
    train, val = loader(1, 2), loader(2, 1)
    net = knet(K, dev)
    ref_net = copy.deepcopy(net)
    options = dict(lr=1e-3, weight_decay=0.05, betas=(0.9, 0.99))
    trainer.training(net, train, val, 1, B, dev, str(tmp_path), "synthetic", loss="ce_dice", loss_weights="none", optimizer="adamw",
                     optimizer_options=options, clip_grad_norm=MAX_NORM)
    losses, vlosses, clips = hand_loop(ref_net, train, val, dev, 2, MAX_NORM, **options)
    print("gradient norms and coefficients of the four steps:", clips)
    assert np.array_equal(np.loadtxt(str(tmp_path / "progress" / "loss.out")), losses)
    assert np.array_equal(np.loadtxt(str(tmp_path / "progress" / "loss_val.out")), vlosses)
    assert np.isfinite(losses).all() and (losses > 0).all()
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), ref_net.parameters()))
    assert any(c < 1.0 for _, c in clips) and any(c == 1.0 for _, c in clips), clips


def test_training_sgd_with_clipping_scales_in_place(dev, tmp_path):
    """optimizer='sgd' (the default) with clip_grad_norm: clip_grad_norm_ scales the gradients in place, then optim.SGD; bit-equal
    to the same written out by hand, and different from the unclipped run."""
    import optim
    import trainer
    train, val = loader(1, 2), loader(2, 1)
    net = small_net(dev)
    ref_net = copy.deepcopy(net)
    trainer.training(net, train, val, 0, B, dev, str(tmp_path), "synthetic", loss="softmax_ce", loss_weights="none", clip_grad_norm=1e-3)
    opt = optim.SGD(ref_net.parameters(), lr=0.0001, momentum=0.99)
    coefs = []
    for images, labels in train:
        opt.zero_grad()
        loss, _ = optim.softmax_ce_step(ref_net(images.to(dev)), labels.to(dev), want_mask=False)
        loss.backward()
        coefs.append(optim.clip_grad_norm_(ref_net.parameters(), 1e-3)[1].item())
        opt.step()
    assert all(c < 1.0 for c in coefs), coefs
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), ref_net.parameters()))


def test_adam_checkpoint_resume_is_bit_exact(dev, tmp_path):
    """An interrupted-and-resumed Adam run is the uninterrupted one, bit for bit: step, exp_avg and exp_avg_sq survive the
    checkpoint, and the file loads with weights_only=True."""
    import checkpoint
    import optim
    (x, y), = loader(4, 1)
    x, y = x.to(dev), y.to(dev)
    net = small_net(dev)

    def steps(m, opt, n):
        for _ in range(n):
            opt.zero_grad(set_to_none=True)
            optim.softmax_ce_step(m(x), y, want_mask=False)[0].backward()
            opt.step()

    a = copy.deepcopy(net); oa = optim.AdamW(a.parameters(), lr=1e-3)
    steps(a, oa, 2)
    path = checkpoint.save_checkpoint(os.path.join(tmp_path, "ck.pth"), a, oa, epoch=7)
    steps(a, oa, 2)
    b = copy.deepcopy(net); ob = optim.AdamW(b.parameters(), lr=1e-3)
    assert checkpoint.load_checkpoint(path, b, ob)["epoch"] == 7
    st = ob.state[next(b.parameters())]
    assert st["step"] == 2 and type(st["step"]) is int and st["exp_avg"].is_cuda and st["exp_avg_sq"].is_cuda
    steps(b, ob, 2)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert all(ob.state[q]["step"] == 4 for q in b.parameters())
    c = copy.deepcopy(net); oc = optim.SGD(c.parameters())
    with pytest.raises(ValueError, match="another kind of optimiser"):
        checkpoint.load_checkpoint(path, c, oc)
    assert len(oc.state) == 0


@pytest.fixture(scope="module")
def default_run(dev, tmp_path_factory):
    """training() with no new argument for one epoch, its checkpoint kept."""
    import trainer
    out = tmp_path_factory.mktemp("default")
    trainer.training(small_net(dev), loader(1, 1), loader(2, 1), 0, B, dev, str(out), "synthetic", loss="softmax_ce", loss_weights="none",
                     save_optimizer=True)
    return os.path.join(str(out), "models", "checkpoint_latest.pth")


def test_defaults_build_todays_sgd(default_run):
    """No new argument: an optim.SGD with lr 1e-4 and momentum 0.99, as the saved checkpoint's param_groups and state show."""
    ck = torch.load(default_run, weights_only=True)
    (group,) = ck["optimizer"]["param_groups"]
    assert sorted(group) == ["lr", "momentum", "params"] and group["lr"] == 0.0001 and group["momentum"] == 0.99
    assert len(group["params"]) == 46
    assert all(sorted(s) == ["momentum_buffer"] for s in ck["optimizer"]["state"].values()) and len(ck["optimizer"]["state"]) == 46


def test_resuming_adam_from_an_sgd_checkpoint_raises(dev, default_run, tmp_path):
    import trainer
    for kind in ("adam", "adamw"):
        with pytest.raises(ValueError, match="another kind of optimiser"):
            trainer.training(small_net(dev), loader(1, 1), loader(2, 1), 1, B, dev, str(tmp_path), "synthetic", loss="softmax_ce",
                             loss_weights="none", optimizer=kind, resume_from=default_run)


def test_training_adam_resume_is_the_interrupted_run(dev, tmp_path):
    """training(optimizer='adam', save_optimizer=True): epochs 0..2 uninterrupted against epoch 0, then a resume for 1..2 from
    checkpoint_latest.pth: the progress series and the last checkpoint's weights and Adam state are bit-equal."""
    import trainer
    full, part = str(tmp_path / "full"), str(tmp_path / "part")
    kw = dict(loss="ce_dice", loss_weights="none", optimizer="adam", optimizer_options=dict(lr=1e-3, weight_decay=0.01), clip_grad_norm=MAX_NORM,
              save_optimizer=True)
    trainer.training(small_net(dev), loader(1, 2), loader(2, 1), 2, B, dev, full, "synthetic", **kw)
    trainer.training(small_net(dev), loader(1, 2), loader(2, 1), 0, B, dev, part, "synthetic", **kw)
    last = os.path.join(part, "models", "checkpoint_latest.pth")
    trainer.training(small_net(dev), loader(1, 2), loader(2, 1), 2, B, dev, part, "synthetic", resume_from=last, **kw)
    for f in sorted(os.listdir(os.path.join(full, "progress"))):
        a = np.atleast_1d(np.loadtxt(os.path.join(full, "progress", f)))
        b = np.atleast_1d(np.loadtxt(os.path.join(part, "progress", f)))
        assert a.shape == (3,) and np.array_equal(a, b), (f, a, b)
    ca = torch.load(os.path.join(full, "models", "checkpoint_latest.pth"), weights_only=True)
    cb = torch.load(last, weights_only=True)
    assert all(torch.equal(ca["model"][k], cb["model"][k]) for k in ca["model"])
    for i, sa in ca["optimizer"]["state"].items():
        sb = cb["optimizer"]["state"][i]
        assert sa["step"] == sb["step"] == 6 and torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
