"""K-class nets on the device (Unet(n_classes=K), 2 < K <= 16): the K-class head per op, the whole net, the softmax
cross-entropy step (the paper's eq. 1), the K-way argmax and confusion counts, overlap-tile segmentation and the trainer's
loss='softmax_ce'.  References: fp64 numpy / torch (tests/multiclass_ref.py), oracle.torch_ref in fp64, and the binary path."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multiclass_ref as ref
import segment_ref
from gpu_support import dev, math_mode, nerr

pytestmark = pytest.mark.gpu

EPS = ref.EPS32
FWD_TOL = 2e-5              # normalised forward error against fp64 (tests/test_net_gpu.py)
GRAD_TOL = 3e-4


def knet(K, dev, base=64, seed=0):
    import network
    m = network.Unet(base_ch=base, n_classes=K)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in ref.head_params(K, base=base, seed=seed).items()})
    return m.to(dev)


# ---- head per op -----------------------------------------------------------------------------------------------------------

def to_bf16(x):
    return x.to(torch.bfloat16)


# every K x C x dtype at a ragged pixel count and at B = 8, 388^2 (the training step's head); at B = 16, 388^2 (2.4M pixels,
# more than 4096 blocks x 512 pixels) the K > 2 backward's blocks take two chunks each
HEAD_CASES = ([(shape, K, C_, dt) for shape in ((1, 37, 29), (8, 388, 388)) for K in (2, 3, 4, 5, 8, 16) for C_ in (32, 64)
               for dt in ("fp32", "bf16")] +
              [((16, 388, 388), 3, 64, "fp32"), ((16, 388, 388), 16, 64, "bf16"), ((16, 388, 388), 5, 32, "fp32")])


@pytest.mark.parametrize("shape,K,C_,dtype", HEAD_CASES)
def test_head1xk_per_op(dev, math_mode, dtype, C_, K, shape):
    """unet_head1xk_fwd / _bwd against fp64, per element within the forward, dz and dw / db chain-length bounds stated in
    multiclass_ref.head_reference_and_bounds (shared with tests/test_multiclass_ops_gpu.py).
    bf16 activations (mode 2) are exact bf16 inputs here, so the same bounds hold for the fp32 outputs.
    At K = 2 the entry points are the head1x1 kernels: bit-identical to unet_head1x1_*."""
    import _hip
    L = _hip.lib()
    math_mode(2 if dtype == "bf16" else 3)
    B, H, W = shape
    n = B * H * W
    g = torch.Generator(device="cpu").manual_seed(K * 100 + C_)
    x = torch.randn(B, H, W, C_, generator=g)
    if dtype == "bf16":
        x = x.to(torch.bfloat16).float()
    w = torch.randn(K, C_, 1, 1, generator=g) * 0.2
    b = torch.randn(K, generator=g) * 0.1
    dl = torch.randn(B, K, H, W, generator=g) * 1e-3
    xd = (to_bf16(x) if dtype == "bf16" else x).to(dev).contiguous()
    wd, bd, dld = w.to(dev), b.to(dev), dl.to(dev)
    y = torch.full((B, K, H, W), float("nan"), device=dev)
    _hip.run("unet_head1xk_fwd", dev, _hip.ptr(xd), B, H, W, C_, K, _hip.ptr(wd), _hip.ptr(bd), _hip.ptr(y))
    sb = L.unet_head1xk_bwd_scratch_bytes(B, H, W, C_, K)
    sc = torch.empty(sb, dtype=torch.uint8, device=dev)
    dz = torch.empty_like(xd)
    dw = torch.full((K, C_, 1, 1), float("nan"), device=dev)
    db = torch.full((K,), float("nan"), device=dev)
    _hip.run("unet_head1xk_bwd", dev, _hip.ptr(xd), B, H, W, C_, K, _hip.ptr(wd), _hip.ptr(dld), _hip.ptr(dz), _hip.ptr(dw),
             _hip.ptr(db), _hip.ptr(sc))
    torch.cuda.synchronize()
    if K == 2:
        y1 = torch.empty_like(y)
        _hip.run("unet_head1x1_fwd", dev, _hip.ptr(xd), B, H, W, C_, _hip.ptr(wd), _hip.ptr(bd), _hip.ptr(y1))
        assert L.unet_head1x1_bwd_scratch_bytes(B, H, W, C_) == sb
        dz1, dw1, db1 = torch.empty_like(dz), torch.empty_like(dw), torch.empty_like(db)
        _hip.run("unet_head1x1_bwd", dev, _hip.ptr(xd), B, H, W, C_, _hip.ptr(wd), _hip.ptr(dld), _hip.ptr(dz1), _hip.ptr(dw1),
                 _hip.ptr(db1), _hip.ptr(sc))
        torch.cuda.synchronize()
        assert torch.equal(y, y1) and torch.equal(dz, dz1) and torch.equal(dw, dw1) and torch.equal(db, db1)
    nb = sb // ((K * C_ + K) * 4)
    r = ref.head_reference_and_bounds(x, w, b, dl, nb, dtype == "bf16")
    yk = y.permute(0, 2, 3, 1).reshape(n, K).double().cpu()
    assert ((yk - r["y"]).abs() <= r["yb"]).all()
    dzk = dz.float().reshape(n, C_).double().cpu()
    assert ((dzk - r["dz"]).abs() <= r["dzb"]).all()
    assert ((dw.reshape(K, C_).double().cpu() - r["dw"]).abs() <= r["dwb"]).all()
    assert ((db.double().cpu() - r["db"]).abs() <= r["dbb"]).all()


def test_head1xk_rejects_bad_arguments(dev):
    import _hip
    L = _hip.lib()
    x = torch.zeros(1, 4, 4, 64, device=dev)
    y = torch.zeros(1, 17, 4, 4, device=dev)
    w = torch.zeros(17, 64, device=dev)
    for K, C_ in ((17, 64), (1, 64), (3, 48)):
        assert L.unet_head1xk_fwd(_hip.ptr(x), 1, 4, 4, C_, K, _hip.ptr(w), _hip.ptr(w), _hip.ptr(y), _hip.stream()) != 0


# ---- whole net -------------------------------------------------------------------------------------------------------------

def abi_fwd_bwd(h, plist, x, dl):
    """unet_forward(training) + unet_backward through the C ABI; returns (logits, grads, workspace)."""
    import _hip
    L = _hip.lib()
    B, _, S, _ = x.shape
    nbytes = h.workspace_bytes(B, S, True)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    logits = torch.empty(B, h.n_classes, S - 184, S - 184, device=x.device)
    ptab = _hip.ptr_table(plist)
    _hip.check(L.unet_forward(h.h, ptab, _hip.ptr(x), _hip.ptr(logits), B, S, _hip.ptr(ws), nbytes, 1, _hip.stream()), "unet_forward")
    grads = [torch.empty_like(p) for p in plist]
    _hip.check(L.unet_backward(h.h, ptab, _hip.ptr(dl), _hip.ptr_table(grads), _hip.ptr(ws), nbytes, _hip.stream()), "unet_backward")
    torch.cuda.synchronize()
    return logits, grads, ws


@pytest.mark.parametrize("mode", [3, 0])
@pytest.mark.parametrize("S", [188, 220])
@pytest.mark.parametrize("K", [3, 8])
def test_whole_net_k_classes(dev, math_mode, mode, S, K):
    """Logits within FWD_TOL of oracle.torch_ref in fp64; finalconv's gradients and conv12e's dz within 2e-5 of fp64 on the
    HIP's own activations; the upstream gradients, by linearity, equal those of binary nets that share the upstream
    parameters: head rows (w0, w1) with dlogits (d0, d1), then (wk, 0) with (dk, 0) for each further class k; their sum
    within 2 x GRAD_TOL (normalised)."""
    import _hip
    import network
    from oracle import prng, torch_ref
    math_mode(mode)
    B = 2
    params = ref.head_params(K)
    names = list(params)
    plist = [torch.from_numpy(params[k]).to(dev) for k in names]
    x = torch.from_numpy(prng.make_input(1, B, S)).to(dev)
    So = S - 184
    dl = torch.from_numpy(prng.make_cotangent(2, (B, K, So, So))).to(dev)
    h = _hip.Handle(64, 0, n_classes=K)
    assert _hip.lib().unet_n_classes(h.h) == K
    n = C.c_size_t()
    _hip.check(_hip.lib().unet_param_count(h.h, 44, C.byref(n)), "param_count")
    assert n.value == K * 64
    _hip.check(_hip.lib().unet_param_count(h.h, 45, C.byref(n)), "param_count")
    assert n.value == K
    logits, grads, ws = abi_fwd_bwd(h, plist, x, dl)
    with torch.no_grad():
        p64 = torch_ref.params_to_torch(params, dtype=torch.float64)
        want = torch_ref.unet_forward(p64, x.double().cpu())
    assert tuple(logits.shape) == (B, K, So, So)
    assert nerr(logits.cpu().numpy(), want.numpy()) < FWD_TOL
    d2 = h.buffer_view(ws, B, S, True, "d2_0").double().cpu().reshape(-1, 64)
    dl64 = dl.double().cpu().permute(0, 2, 3, 1).reshape(-1, K)
    w64 = torch.from_numpy(params["finalconv.weight"]).double().reshape(K, 64)
    assert nerr(grads[44].cpu().numpy().reshape(K, 64), (dl64.T @ d2).numpy()) < 2e-5
    assert nerr(grads[45].cpu().numpy(), dl64.sum(0).numpy()) < 2e-5
    gdz = h.buffer_view(ws, B, S, True, "g_d2_0").double().cpu().reshape(-1, 64)
    assert nerr(gdz.numpy(), ((dl64 @ w64) * (d2 > 0)).numpy()) < 2e-5
    # linearity: the binary net's upstream gradients, one pair of head rows at a time
    h2 = network._handle(0)
    total = None
    pairs = [(0, 1)] + [(k, None) for k in range(2, K)]
    for a, b in pairs:
        wp = torch.zeros(2, 64, 1, 1, device=dev)
        bp = torch.zeros(2, device=dev)
        dp = torch.zeros(B, 2, So, So, device=dev)
        for j, k in enumerate((a, b)):
            if k is not None:
                wp[j] = plist[44][k]
                bp[j] = plist[45][k]
                dp[:, j] = dl[:, k]
        _, g2, _ = abi_fwd_bwd(h2, plist[:44] + [wp, bp], x, dp.contiguous())
        up = [g.double().cpu() for g in g2[:44]]
        total = up if total is None else [t + u for t, u in zip(total, up)]
    worst = max(nerr(grads[i].cpu().numpy(), total[i].numpy()) for i in range(44))
    print("K=%d S=%d mode %d: upstream vs binary sum %.3g" % (K, S, mode, worst))
    assert worst < 2 * GRAD_TOL


def test_grad_scale_dp_and_no_grad_forward_k3(dev):
    """unet_set_grad_scale(0.5) halves every gradient bit for bit; a one-rank data-parallel K = 3 step equals the plain step;
    the no-grad forward equals the training forward bit for bit."""
    import _hip
    import network
    from oracle import prng
    L = _hip.lib()
    net = knet(3, dev)
    x = torch.from_numpy(prng.make_input(1, 2, 220)).to(dev)
    dl = torch.from_numpy(prng.make_cotangent(2, (2, 3, 36, 36))).to(dev)

    def step(m):
        m.zero_grad(set_to_none=True)
        y = m(x)
        y.backward(dl)
        torch.cuda.synchronize()
        return y.detach().clone(), [p.grad.clone() for p in m.parameters()]

    y0, g0 = step(net)
    with torch.no_grad():
        y_ng = net(x)
    assert torch.equal(y0, y_ng)
    h = network._handle(0, 64, 3)
    assert h.n_classes == 3 and L.unet_n_classes(h.h) == 3
    try:
        _hip.check(L.unet_set_grad_scale(h.h, 0.5), "unet_set_grad_scale")
        _, gh = step(net)
    finally:
        _hip.check(L.unet_set_grad_scale(h.h, 1.0), "unet_set_grad_scale")
    assert all(torch.equal(a * 0.5, b) for a, b in zip(g0, gh))
    m = copy.deepcopy(net)
    m.enable_data_parallel(backend="rccl")
    assert m._get_handle(0).n_classes == 3 and m._get_handle(0) is not h
    y1, g1 = step(m)
    assert torch.equal(y0, y1) and all(torch.equal(a, b) for a, b in zip(g0, g1))


# ---- softmax cross-entropy step ----------------------------------------------------------------------------------------------

def ce_inputs(K, seed, B=2, H=45, W=53, pad=3):
    """Logits [B,K,H+2pad,W+2pad] with planted ties (the centre crop is the view the step reads), labels in [0, K), a
    per-pixel weight map."""
    rs = np.random.RandomState(seed)
    full = (rs.randn(B, K, H + 2 * pad, W + 2 * pad) * 2).astype(np.float32)
    crop = full[:, :, pad:pad + H, pad:pad + W]
    crop[0, :, 0, :5] = crop[0, 0, 0, :5]                          # every class tied
    crop[1, K - 1, 3, :7] = crop[1, :, 3, :7].max(axis=0)          # tie between the max and the last class
    crop[1, 1, 4, :7] = crop[1, :, 4, :7].max(axis=0)
    lab = rs.randint(0, K, (B, H, W)).astype(np.int64)
    w = rs.uniform(0.1, 4.0, (B, H, W)).astype(np.float32)
    return full, lab, w


def run_ce(dev, full, lab, w, pad, grad_scale=1.0, validate=True, want_mask=True, weight_view=None):
    import optim
    fd = torch.from_numpy(full).to(dev).requires_grad_(True)
    H, W = lab.shape[1:]
    view = fd[:, :, pad:pad + H, pad:pad + W]
    wt = None if w is None else (weight_view if weight_view is not None else torch.from_numpy(w).to(dev))
    loss, mask = optim.softmax_ce_step(view, torch.from_numpy(lab).to(dev), weight=wt, grad_scale=grad_scale,
                                       validate=validate, want_mask=want_mask)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), mask, fd.grad[:, :, pad:pad + H, pad:pad + W]


@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("weighted", [False, True])
def test_softmax_ce_step(dev, K, weighted):
    """On a strided crop view: loss within 1e-6 relative of fp64 (each pixel's term is (m - l_label) + log(sum exp(l - m)),
    two non-negative terms with a few ulp each, summed in double); dlogits within (w / n) (2R + K + 12) EPS of fp64
    (the softmax bound of multiclass_ref.softmax_bound, plus the roundings of w / n and of p - onehot); the mask bit-exact
    against torch.argmax with planted ties; grad_scale halves dlogits bit for bit."""
    pad = 3
    full, lab, w = ce_inputs(K, 10 + K)
    H, W = lab.shape[1:]
    crop = full[:, :, pad:pad + H, pad:pad + W]
    loss, mask, d = run_ce(dev, full, lab, w if weighted else None, pad)
    want_loss, want_d, _, _ = ref.softmax_ce(crop, lab, w if weighted else None)
    assert abs(loss.item() - want_loss) <= 1e-6 * abs(want_loss)
    R = float((crop.max(axis=1, keepdims=True) - crop).max())
    wmax = float(w.max()) if weighted else 1.0
    bound = wmax / lab.size * (2 * R + K + 12) * EPS
    err = np.abs(d.cpu().numpy() - want_d).max()
    print("K=%d weighted=%s: loss rel err %.3g, dlogits err %.3g (bound %.3g)" % (K, weighted, abs(loss.item() - want_loss) / want_loss,
                                                                                 err, bound))
    assert err <= bound
    assert np.array_equal(mask.cpu().numpy(), torch.argmax(torch.from_numpy(np.ascontiguousarray(crop)), dim=1).numpy())
    _, _, d2 = run_ce(dev, full, lab, w if weighted else None, pad, grad_scale=0.5)
    assert torch.equal(d * 0.5, d2)


def test_softmax_ce_weight_broadcast_and_invalid_labels(dev):
    """A [H,W] map and a strided [B,H,W] view weight every sample per pixel; labels outside [0, K) add no loss and no
    gradient, are counted, and raise with validate=True."""
    import optim
    K, pad = 4, 2
    full, lab, w = ce_inputs(K, 7, pad=pad)
    H, W = lab.shape[1:]
    crop = full[:, :, pad:pad + H, pad:pad + W]
    big = torch.from_numpy(np.repeat(np.repeat(w[:1], 2, axis=0), 2, axis=2)).to(dev)[:, :, ::2]   # [B,H,W], column stride 2
    loss, _, d = run_ce(dev, full, lab, w, pad, weight_view=big)
    want, want_d, _, _ = ref.softmax_ce(crop, lab, w[:1])
    assert abs(loss.item() - want) <= 1e-6 * abs(want)
    loss2, _, d2 = run_ce(dev, full, lab, w, pad, weight_view=torch.from_numpy(w[0]).to(dev))
    assert torch.equal(loss, loss2) and torch.equal(d, d2)
    bad = lab.copy()
    bad[0, 1, :4] = [-1, K, 1000, -7]
    bad[1, 0, 0] = K
    with pytest.raises(ValueError, match="5 label"):
        run_ce(dev, full, bad, None, pad)
    loss, mask, d = run_ce(dev, full, bad, None, pad, validate=False)
    want, want_d, _, nbad = ref.softmax_ce(crop, bad, None)
    assert nbad == 5 and abs(loss.item() - want) <= 1e-6 * abs(want)
    dd = d.cpu().numpy()
    assert (dd[0, :, 1, :4] == 0).all() and (dd[1, :, 0, 0] == 0).all()
    assert np.abs(dd - want_d).max() <= (2 * float((crop.max(axis=1, keepdims=True) - crop).max()) + K + 12) * EPS / bad.size
    with pytest.raises(ValueError):
        optim.softmax_ce_step(torch.zeros(2, 3, 4, 4, device=dev), torch.zeros(2, 4, 4, dtype=torch.int64, device=dev),
                              weight=torch.ones(3, 4, 4, device=dev))


def test_softmax_ce_repeat_and_side_stream_determinism(dev):
    K, pad = 8, 3
    full, lab, w = ce_inputs(K, 21, B=3, H=130, W=127)
    a = run_ce(dev, full, lab, w, pad)
    b = run_ce(dev, full, lab, w, pad)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = run_ce(dev, full, lab, w, pad)
    s.synchronize()
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2])


# ---- argmax and confusion counts --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [2, 3, 5, 16])
def test_argmaxk_and_confusion_exact(dev, K):
    import optim
    from functions import metrics_from_confusion, metrics_from_counts
    rs = np.random.RandomState(K)
    B, So, n = 3, 68, 60
    lg = rs.randint(-3, 4, (B, K, So, So)).astype(np.float32)          # small integers: many ties
    lab = rs.randint(0, K, (B, n, n)).astype(np.int64)
    lab[2, 5, :3] = [-1, K, 99]
    lgd = torch.from_numpy(lg).to(dev)
    am = optim.argmaxk(lgd[:, :, 1:-1, 2:])
    assert np.array_equal(am.cpu().numpy(), ref.argmax_first(lg[:, :, 1:-1, 2:]))
    mask, conf, invalid = optim.crop_argmax_confusion(lgd, torch.from_numpy(lab).to(dev), return_invalid=True)
    pad = (So - n) // 2
    want_mask = ref.argmax_first(lg[:, :, pad:pad + n, pad:pad + n])
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    wc, wb = ref.confusion(want_mask, lab, K)
    assert np.array_equal(conf.cpu().numpy(), wc) and np.array_equal(invalid.cpu().numpy(), wb)
    m2, none = optim.crop_argmax_confusion(lgd)
    assert none is None and np.array_equal(m2.cpu().numpy(), ref.argmax_first(lg))
    if K == 2:
        lab2 = np.clip(lab, 0, 1)
        _, conf2 = optim.crop_argmax_confusion(lgd, torch.from_numpy(lab2).to(dev))
        _, stats = optim.crop_argmax_metrics(lgd, torch.from_numpy(lab2).to(dev))
        for b in range(B):
            inter, union, diff = (int(v) for v in stats[b].tolist())
            assert np.array_equal(metrics_from_confusion(conf2[b].cpu().numpy()), metrics_from_counts(inter, union, diff, n * n))


# ---- overlap-tile segmentation -------------------------------------------------------------------------------------------

def seg_image(seed, B, H, W):
    rs = np.random.RandomState(seed)
    return (rs.rand(B, H, W) * 255).astype(np.float32)


@pytest.mark.parametrize("mode", [3, 2])
@pytest.mark.parametrize("B,H,W,S,mb", [(1, 91, 157, 220, 16), (2, 130, 77, 220, 3), (1, 300, 301, None, 16)])
def test_segment_k3(dev, math_mode, mode, B, H, W, S, mb):
    """The mask is bit-identical to numpy reflect-pad -> Unet.forward per chunk -> numpy K-way stitch; the probabilities are
    within multiclass_ref.softmax_bound of the fp64 softmax of the same logits."""
    import tester
    math_mode(mode)
    net = knet(3, dev)
    img = seg_image(H + W + mode, B, H, W)
    S_used = S or tester.auto_tile_size(H, W)
    tl = torch.from_numpy(segment_ref.tiles(img, S_used, norm=True)).to(dev)
    with torch.no_grad():
        lg = torch.cat([net(tl[a:a + mb]) for a in range(0, tl.shape[0], mb)]).cpu().numpy()
    want_m, want_p = ref.stitch_k(lg, B, H, W, S_used)
    m, p = tester.segment(net, torch.from_numpy(img).to(dev), tile_size=S, max_batch=mb, return_probs=True)
    assert m.shape == (B, H, W) and p.shape == (B, 3, H, W) and p.dtype == torch.float32
    assert np.array_equal(m.cpu().numpy(), want_m)
    assert np.abs(p.cpu().numpy() - want_p).max() <= ref.softmax_bound(lg, 3)
    m1, p1 = tester.segment(net, torch.from_numpy(img[0]).to(dev), tile_size=S, max_batch=mb, return_probs=True)
    assert m1.shape == (H, W) and p1.shape == (3, H, W) and torch.equal(m1, m[0])


def test_segment_k2_unchanged(dev):
    """A net made with n_classes=2 segments exactly as today's binary path: unet_tile_stitch's mask and probability."""
    import tester
    net = knet(2, dev)
    img = seg_image(3, 1, 250, 190)
    S = 220
    tl = torch.from_numpy(segment_ref.tiles(img, S, norm=True)).to(dev)
    with torch.no_grad():
        lg = net(tl).cpu().numpy()
    want_m, want_p = segment_ref.stitch(lg, 1, 250, 190, S)
    m, p = tester.segment(net, torch.from_numpy(img).to(dev), tile_size=S, return_probs=True)
    assert p.shape == (1, 250, 190) and np.array_equal(m.cpu().numpy(), want_m)
    assert np.abs(p.cpu().numpy() - want_p).max() <= 4e-7


def test_tile_stitch_k_rejects_bad_arguments(dev):
    import _hip
    L = _hip.lib()
    lg = torch.zeros(1, 17, 4, 4, device=dev)
    mask = torch.zeros(1, 4, 4, dtype=torch.int64, device=dev)
    assert L.unet_tile_stitch_k(_hip.ptr(lg), 4, 17, 0, 0, 1, 1, 0, 1, 1, 4, 4, _hip.ptr(mask), None, _hip.stream()) != 0
    assert L.unet_tile_stitch_k(_hip.ptr(lg), 4, 3, 0, 0, 1, 1, 0, 2, 1, 4, 4, _hip.ptr(mask), None, _hip.stream()) != 0


# ---- trainer ----------------------------------------------------------------------------------------------------------------

def tiny_loader(seed, n, B, S, K):
    from oracle import prng
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        x = torch.from_numpy(prng.make_input(seed * 10 + i, B, S))
        y = torch.from_numpy(rs.randint(0, K, (B, 1, S - 184 - 8, S - 184 - 8)).astype(np.int64))
        out.append((x, y))
    return out


def test_training_softmax_ce_k3_matches_hand_loop(dev, tmp_path):
    """training(loss='softmax_ce', loss_weights='none') of a K = 3 net for 2 epochs: the loss series equals, bit for bit, a
    hand-written loop over the public ops (forward, centre crop, softmax_ce_step, backward, optim.SGD); progress written."""
    import optim
    import trainer
    S, B = 220, 2
    train, val = tiny_loader(1, 2, B, S, 3), tiny_loader(2, 1, B, S, 3)
    net = knet(3, dev)
    ref_net = copy.deepcopy(net)
    trainer.training(net, train, val, 1, B, dev, str(tmp_path), "synthetic", loss="softmax_ce", loss_weights="none")
    opt = optim.SGD(ref_net.parameters(), lr=0.0001, momentum=0.99)
    losses, vlosses = [], []
    for _ in range(2):
        tot = 0
        for images, labels in train:
            opt.zero_grad()
            preds = ref_net(images.to(dev))
            n = labels.shape[-1]
            pad = (preds.shape[-1] - n) // 2
            loss, _ = optim.softmax_ce_step(preds[:, :, pad:pad + n, pad:pad + n], labels.to(dev), want_mask=False)
            loss.backward()
            opt.step()
            tot += loss.detach()
        vt = 0
        with torch.no_grad():
            for images, labels in val:
                preds = ref_net(images.to(dev))
                pad = (preds.shape[-1] - labels.shape[-1]) // 2
                vt += optim.softmax_ce_step(preds[:, :, pad:pad + labels.shape[-1], pad:pad + labels.shape[-1]], labels.to(dev),
                                            want_mask=False)[0]
        losses.append((tot / (len(train) * B)).item())
        vlosses.append((vt / (len(val) * B)).item())
    got = np.loadtxt(str(tmp_path / "progress" / "loss.out"))
    got_v = np.loadtxt(str(tmp_path / "progress" / "loss_val.out"))
    assert np.array_equal(got, np.array(losses, np.float64)) and np.array_equal(got_v, np.array(vlosses, np.float64))
    for f in ("train_eval_iou.out", "train_eval_pe.out", "val_eval_iou.out", "val_eval_pe.out"):
        v = np.loadtxt(str(tmp_path / "progress" / f))
        assert v.shape == (2,)
    pe = np.loadtxt(str(tmp_path / "progress" / "train_eval_pe.out"))
    assert ((pe >= 0) & (pe <= 1)).all()


def test_training_softmax_ce_k2_class_balance_first_loss(dev, tmp_path):
    """K = 2 with loss_weights='class_balance': one step of one epoch; the step's loss (loss.out x batch) is within 1e-6 of
    the fp64 mean of w * CE on the logits of the untrained net, w = the class-balance map."""
    import trainer
    S, B = 220, 2
    train = tiny_loader(5, 1, B, S, 2)
    net = knet(2, dev)
    with torch.no_grad():
        lg = net(train[0][0].to(dev)).double().cpu()
    trainer.training(net, train, train, 0, B, dev, str(tmp_path), "synthetic", loss="softmax_ce", loss_weights="class_balance")
    lab = train[0][1][:, 0]
    n = lab.shape[-1]
    pad = (lg.shape[-1] - n) // 2
    crop = lg[:, :, pad:pad + n, pad:pad + n]
    ce = F.cross_entropy(crop, lab, reduction="none")
    n1 = lab.sum(dim=(1, 2), keepdim=True).double()
    n0 = n * n - n1
    w = torch.where(lab != 0, torch.ones_like(ce), n1 / n0)
    want = (w * ce).mean().item()
    got = float(np.loadtxt(str(tmp_path / "progress" / "loss.out"))) * B
    assert abs(got - want) <= 1e-6 * abs(want)


def test_training_bce_unweighted_first_loss(dev, tmp_path):
    """loss='bce' with loss_weights='none' (a binary net): the reference's BCE on the one-hot target without a weight map;
    the step's loss is within 1e-6 of the fp64 mean over [B,2,H,W] of BCE-with-logits on the untrained net's logits."""
    import network
    import trainer
    from oracle import prng
    S, B = 220, 2
    train = tiny_loader(6, 1, B, S, 2)
    net = network.Unet()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in prng.make_params(0).items()})
    net = net.to(dev)
    with torch.no_grad():
        lg = net(train[0][0].to(dev)).double().cpu()
    trainer.training(net, train, train, 0, B, dev, str(tmp_path), "synthetic", loss="bce", loss_weights="none")
    lab = train[0][1][:, 0].double()
    n = lab.shape[-1]
    pad = (lg.shape[-1] - n) // 2
    crop = lg[:, :, pad:pad + n, pad:pad + n]
    target = torch.stack([1 - lab, lab], dim=1)
    want = F.binary_cross_entropy_with_logits(crop, target).item()
    got = float(np.loadtxt(str(tmp_path / "progress" / "loss.out"))) * B
    assert abs(got - want) <= 1e-6 * abs(want)


def test_k_class_handle_sizes_and_flops(dev):
    """unet_workspace_bytes / unet_flops of a K-class handle: K = 2 is the binary handle's exactly; the head adds
    2 B So^2 C (K - 2) FLOPs to the forward and three times that to forward + backward."""
    import _hip
    import network
    h2 = network._handle(0)
    for K in (2, 3, 16):
        h = _hip.Handle(64, 0, n_classes=K)
        for B, S in ((1, 188), (8, 572)):
            So = S - 184
            extra = 2.0 * B * So * So * 64 * (K - 2)
            assert h.flops(B, S, False) - h2.flops(B, S, False) == pytest.approx(extra, rel=1e-12, abs=1e-3)
            assert h.flops(B, S, True) - h2.flops(B, S, True) == pytest.approx(3 * extra, rel=1e-12, abs=1e-3)
            for tr in (0, 1):
                if K == 2:
                    assert h.workspace_bytes(B, S, tr) == h2.workspace_bytes(B, S, tr)
                else:
                    assert h.workspace_bytes(B, S, tr) >= h2.workspace_bytes(B, S, tr)
