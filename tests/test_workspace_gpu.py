"""Whole-net independence of the workspace's contents, through _hip.Handle and the C ABI directly so that the test owns
every buffer (tests/guarded.py): the workspace has exactly unet_workspace_bytes(...) usable bytes; parameters, image,
dlogits, logits, dx and the 46 gradient tensors are guarded buffers.

The library may assume nothing about what the workspace holds: every region it reads it must have written during the same
forward / backward.  So the same step is run with the workspace preset to 0x00, to 0xFF (NaN in fp32 and bf16), to seeded
random bytes (NaN, Inf and denormals among them), and once more after a step of ANOTHER plan ran in the same allocation
and left its activations behind.  The library is deterministic, so logits, all 46 gradients and dx must be bit-identical
across the four runs, free of NaN, fully written, and no guard byte may change - the bytes right after
unet_workspace_bytes(...) included.  Bit-identity between four wrong answers must not pass: the logits of the 0xFF run
are held to fp64 (oracle.torch_ref, and the reference's golden where one exists: base 64, 2 classes, (B, S) = (2, 188)) at
the tolerance tests/test_net_gpu.py uses for the mode."""
import os

import numpy as np
import pytest
import torch

import guarded as gd
from gpu_support import nerr

pytestmark = pytest.mark.gpu

# forward tolerance per arithmetic mode (normalised max error against fp64), as in tests/test_net_gpu.py: FWD_TOL for the fp32
# modes 3 and 0, test_bf16x3_mode_keeps_fp32_class_accuracy's 2e-4 for mode 1, test_bf16_compute_mode's 5e-2 for mode 2
FWD_TOL = {3: 2e-5, 0: 2e-5, 1: 2e-4, 2: 5e-2}
OTHER = (1, 188)                    # the plan that leaves stale activations behind: smaller than either plan under test
PATTERNS = ("0x00", "0xFF", "random", "stale")

_params = {}


def params_of(base, K):
    if (base, K) not in _params:
        import multiclass_ref as ref
        _params[(base, K)] = ref.head_params(K, base=base)
    return _params[(base, K)]


class Net:
    """One handle, guarded parameters, and the step under test on caller-owned buffers."""

    def __init__(self, mode, base, K):
        import _hip
        self.hip, self.L = _hip, _hip.lib()
        self.K = K
        self.h = _hip.Handle(base, 0, math=mode, n_classes=K)
        self.keep = gd.Arena()
        self.params = params_of(base, K)
        self.plist = [self.keep.inp(torch.from_numpy(v), k) for k, v in self.params.items()]
        self.ptab = _hip.ptr_table(self.plist)

    def inputs(self, B, S):
        from oracle import prng
        x = self.keep.inp(torch.from_numpy(prng.make_input(1, B, S)), "x")
        dl = self.keep.inp(torch.from_numpy(prng.make_cotangent(2, (B, self.K, S - 184, S - 184))), "dlogits")
        return x, dl

    def step(self, A, wsa, ws, nbytes, x, dl, training):
        """Training: forward, every backward stage, unet_backward_input.  Inference: the forward.  Returns the outputs
        (device tensors from `A`), all fully written, with every guard of `A`, of the workspace (arena `wsa`) and of the inputs intact."""
        hip, L = self.hip, self.L
        B, _, S, _ = x.shape
        logits = A.out((B, self.K, S - 184, S - 184), torch.float32, "logits")
        wsp = wsa.ptr(ws)
        hip.check(L.unet_forward(self.h.h, self.ptab, hip.ptr(x), hip.ptr(logits), B, S, wsp, nbytes, int(training), hip.stream()), "unet_forward")
        outs = [logits]
        if training:
            grads = [A.out(p.shape, torch.float32, "grad %s" % k) for k, p in zip(self.params, self.plist)]
            gtab = hip.ptr_table(grads)
            for s in range(L.unet_backward_stages()):
                hip.check(L.unet_backward_stage(self.h.h, s, self.ptab, hip.ptr(dl), gtab, wsp, nbytes, hip.stream()), "unet_backward_stage %d" % s)
            dx = A.out((B, 1, S, S), torch.float32, "dx")
            hip.check(L.unet_backward_input(self.h.h, self.ptab, hip.ptr(dx), wsp, nbytes, hip.stream()), "unet_backward_input")
            outs += grads + [dx]
        torch.cuda.synchronize()
        A.verify(*outs)
        wsa.check()
        self.keep.check()
        return outs

    def four_runs(self, B, S, training):
        """The step with the workspace preset four ways; returns {pattern: [cpu tensors]}."""
        nbytes = self.h.workspace_bytes(B, S, training)
        ob, os_ = OTHER
        assert self.h.workspace_bytes(ob, os_, training) <= nbytes
        wsa = gd.Arena()
        ws = wsa.scratch(nbytes, "workspace of exactly unet_workspace_bytes(%d, %d, %d)" % (B, S, training))
        assert wsa.address(ws) % 256 == 0
        x, dl = self.inputs(B, S)
        xo, dlo = self.inputs(ob, os_)
        res = {}
        for pat in PATTERNS:
            if pat == "0x00":
                ws.zero_()
            elif pat == "0xFF":
                ws.fill_(0xFF)
            elif pat == "random":
                g = torch.Generator(device="cuda"); g.manual_seed(20240607)
                ws.random_(0, 256, generator=g)
            else:                                   # what a step of another plan leaves in the same allocation
                self.step(gd.Arena(), wsa, ws, nbytes, xo, dlo, training)
            outs = self.step(gd.Arena(), wsa, ws, nbytes, x, dl, training)
            res[pat] = [t.cpu() for t in outs]
        return res


def names_of(net, training):
    return ["logits"] + (["grad %s" % k for k in net.params] + ["dx"] if training else [])


@pytest.mark.parametrize("B,S", [(2, 188), (1, 220)])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("mode,base", [(3, 64), (0, 64), (1, 64), (2, 64), (3, 32)])
def test_results_do_not_depend_on_workspace_contents(golden_dir, mode, base, K, B, S):
    from oracle import prng, torch_ref
    net = Net(mode, base, K)
    with torch.no_grad():
        want = torch_ref.unet_forward(torch_ref.params_to_torch(net.params, dtype=torch.float64),
                                      torch.from_numpy(prng.make_input(1, B, S)).double()).numpy()
    for training in (1, 0):
        res = net.four_runs(B, S, training)
        names = names_of(net, training)
        for pat in PATTERNS:
            for n, t in zip(names, res[pat]):
                assert not torch.isnan(t).any(), "%s is NaN with the workspace preset to %s (training=%d)" % (n, pat, training)
        for pat in PATTERNS[1:]:
            for n, a, b in zip(names, res["0x00"], res[pat]):
                assert torch.equal(a, b), "%s differs between a workspace preset to 0x00 and to %s (training=%d): %d of %d elements, max |d| %.3g" % (
                    n, pat, training, int((a != b).sum()), a.numel(), float((a.double() - b.double()).abs().max()))
        # four identical answers must also be right ones
        logits = res["0xFF"][0].numpy()
        e = nerr(logits, want)
        print("mode %d base %d K=%d B=%d S=%d training=%d: logits %.3g from fp64 (tolerance %.3g)" % (mode, base, K, B, S, training, e, FWD_TOL[mode]))
        assert e < FWD_TOL[mode]
        if base == 64 and K == 2 and (B, S) == (2, 188):
            g = np.load(os.path.join(golden_dir, "unet_S188.npz"))
            assert nerr(logits, g["logits_f64"]) < FWD_TOL[mode]
