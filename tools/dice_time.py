"""Device time of unet_dice_step with gradient (optim.dice_step's library call), for the Dice loss alone (ce_weight 0,
dice_weight 1) and for CE + Dice (1, 1), against unet_softmax_ce_step with gradient on the same inputs, at the training
step's shapes 8 x 2 x 388^2 and 8 x 3 x 388^2 (and 8 x 16 x 388^2 for the register-heavy end).  Logits randn x 2, labels
uniform over the classes, a dense weight map wherever a CE term is computed, the argmax mask asked for in both ops.  Events
around the library call alone (buffers preallocated, no host sync inside), median, minimum and maximum of --reps, after 3
warm-up calls.  The ratio to expect from the bytes moved is printed beside the measured one: the CE step reads K logits, a
label and a weight and writes K gradients and a mask per pixel; the Dice step reads the logits and the label twice.

    timeout -k 10 300 python tools/dice_time.py [--reps 200] [--json profiles/dice_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dl-unet_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import _hip  # noqa: E402
from instances_time import event_median  # noqa: E402


def time_case(dev, B, K, H, W, reps):
    L = _hip.lib()
    g = torch.Generator(device="cpu").manual_seed(K)
    x = (torch.randn(B, K, H, W, generator=g) * 2).to(dev)
    y = torch.randint(0, K, (B, H, W), generator=g).to(dev)
    w = (torch.rand(B, H, W, generator=g) * 3.9 + 0.1).to(dev)
    dl = torch.empty_like(x)
    mask = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    loss = torch.empty(3, device=dev)
    coeffs = torch.empty(B, K, device=dev)
    invalid = torch.empty((), dtype=torch.int64, device=dev)
    sc_ce = torch.empty(L.unet_softmax_ce_scratch_bytes(B * H * W), dtype=torch.uint8, device=dev)
    sc = torch.empty(L.unet_dice_scratch_bytes(B, K, H, W), dtype=torch.uint8, device=dev)
    xs = (x.stride(0), x.stride(1), x.stride(2))
    ws = (H * W, W, 1)

    def ce():
        _hip.run("unet_softmax_ce_step", dev, _hip.ptr(x), *xs, K, _hip.ptr(y), _hip.ptr(w), *ws, B, H, W, _hip.ptr(loss), _hip.ptr(dl), 1.0,
                 _hip.ptr(mask), _hip.ptr(invalid), _hip.ptr(sc_ce))

    def dice(cw, dw, grad=True):
        wp, wst = (_hip.ptr(w), ws) if cw else (None, (0, 0, 0))
        _hip.run("unet_dice_step", dev, _hip.ptr(x), *xs, K, _hip.ptr(y), wp, *wst, B, H, W, cw, dw, 1.0, 0, _hip.ptr(loss), _hip.ptr(coeffs),
                 _hip.ptr(dl) if grad else None, 1.0, _hip.ptr(mask), _hip.ptr(invalid), _hip.ptr(sc))

    r = {"B": B, "K": K, "H": H, "W": W, "reps": reps}
    r["softmax_ce_ms"] = event_median(ce, reps)
    r["dice_0_1_ms"] = event_median(lambda: dice(0.0, 1.0), reps)
    r["dice_1_1_ms"] = event_median(lambda: dice(1.0, 1.0), reps)
    r["dice_1_1_no_grad_ms"] = event_median(lambda: dice(1.0, 1.0, False), reps)
    ce_bytes = 4 * K + 8 + 4 + 4 * K + 8
    r["bytes_per_pixel"] = {"softmax_ce": ce_bytes, "dice_0_1": 2 * (4 * K + 8) + 4 * K + 8, "dice_1_1": 2 * (4 * K + 8 + 4) + 4 * K + 8}
    r["ratio_0_1"] = r["dice_0_1_ms"][0] / r["softmax_ce_ms"][0]
    r["ratio_1_1"] = r["dice_1_1_ms"][0] / r["softmax_ce_ms"][0]
    r["ratio_1_1_by_bytes"] = r["bytes_per_pixel"]["dice_1_1"] / ce_bytes
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = []
    for B, K, H, W in ((8, 2, 388, 388), (8, 3, 388, 388), (8, 16, 388, 388)):
        r = time_case(dev, B, K, H, W, a.reps)
        res.append(r)
        print("%d x %d x %d x %d: softmax_ce_step %.4f ms [%.4f .. %.4f] | dice_step (0,1) %.4f ms [%.4f .. %.4f] = %.2f x | (1,1) %.4f ms "
              "[%.4f .. %.4f] = %.2f x (%.2f x by bytes) | (1,1) without gradient %.4f ms"
              % (B, K, H, W, *r["softmax_ce_ms"], *r["dice_0_1_ms"], r["ratio_0_1"], *r["dice_1_1_ms"], r["ratio_1_1"], r["ratio_1_1_by_bytes"],
                 r["dice_1_1_no_grad_ms"][0]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
