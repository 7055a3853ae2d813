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
from gpu_support import Net, nerr

pytestmark = pytest.mark.gpu

# forward tolerance per arithmetic mode (normalised max error against fp64), as in tests/test_net_gpu.py: FWD_TOL for the fp32
# modes 3 and 0, test_bf16x3_mode_keeps_fp32_class_accuracy's 2e-4 for mode 1, test_bf16_compute_mode's 5e-2 for mode 2
FWD_TOL = {3: 2e-5, 0: 2e-5, 1: 2e-4, 2: 5e-2}
OTHER = (1, 188)                    # the plan that leaves stale activations behind: smaller than either plan under test
PATTERNS = ("0x00", "0xFF", "random", "stale")


def four_runs(net, B, S, training):
    """The step with the workspace preset four ways; returns {pattern: [cpu tensors]}."""
    nbytes = net.h.workspace_bytes(B, S, training)
    ob, os_ = OTHER
    assert net.h.workspace_bytes(ob, os_, training) <= nbytes
    wsa = gd.Arena()
    ws = wsa.scratch(nbytes, "workspace of exactly unet_workspace_bytes(%d, %d, %d)" % (B, S, training))
    assert wsa.address(ws) % 256 == 0
    x, dl = net.inputs(B, S)
    xo, dlo = net.inputs(ob, os_)
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
            net.step(gd.Arena(), wsa, ws, nbytes, xo, dlo, training)
        outs = net.step(gd.Arena(), wsa, ws, nbytes, x, dl, training)
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
        res = four_runs(net, B, S, training)
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
