"""Device time of the multi-tensor update and clipping passes over the 46 real parameter tensors of Unet() (31 M fp32 elements):
unet_sgd_momentum (20 B per element), unet_adam_step (28 B), unet_adam_step with a grad_scale_dev (28 B), unet_grad_sumsq +
unet_grad_norm_finish (4 B) and unet_grads_scale (8 B).  Events around the library call alone (buffers preallocated, pointer
tables built once, no host sync inside), median, minimum and maximum of --reps, after 3 warm-up calls.  The figure that matters
is unet_adam_step / unet_sgd_momentum on the same tensors in the same run: 28 / 20 = 1.4 by bytes; its allowance is the spread
(max / min over the repeats) the unchanged SGD kernel shows in that run, recorded beside the ratio.

    timeout -k 10 300 python tools/adam_time.py [--reps 200] [--json profiles/adam_time.json]
"""
import argparse
import ctypes as C
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import network
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = _hip.lib()
    g = torch.Generator(device="cpu").manual_seed(0)
    ps = [p.detach() for p in network.Unet().to(dev).parameters()]
    gs = [(torch.randn(p.shape, generator=g) * 1e-3).to(dev) for p in ps]
    bufs, ms, vs = ([torch.zeros_like(p) for p in ps] for _ in range(3))
    n = len(ps)
    numel = (C.c_size_t * n)(*[p.numel() for p in ps])
    total = sum(p.numel() for p in ps)
    tp, tg, tb, tm, tv = (_hip.ptr_table(t) for t in (ps, gs, bufs, ms, vs))
    n_partials = L.unet_grad_sumsq_partials(numel, n)
    partials = torch.empty(n_partials, dtype=torch.float64, device=dev)
    out2 = torch.empty(2, device=dev)
    one = torch.ones(1, device=dev)

    def sgd():
        _hip.run("unet_sgd_momentum", dev, tp, tg, tb, numel, n, 1e-4, 0.99, 0)

    def adam(scale=None):
        _hip.run("unet_adam_step", dev, tp, tg, tm, tv, numel, n, 1e-4, 0.9, 0.999, 1e-8, 0.01, 1, 7, _hip.ptr(scale))

    def norm():
        _hip.run("unet_grad_sumsq", dev, tg, numel, n, _hip.ptr(partials), 0)
        _hip.run("unet_grad_norm_finish", dev, _hip.ptr(partials), n_partials, 1.0, _hip.ptr(out2))

    def scale():
        _hip.run("unet_grads_scale", dev, tg, numel, n, _hip.ptr(one))

    r = {"tensors": n, "elements": total, "reps": a.reps, "aligned16": all(t.data_ptr() % 16 == 0 for t in ps + gs + bufs + ms + vs),
         "tail_elements": sum(p.numel() % 4096 for p in ps)}
    cases = (("sgd_momentum", sgd, 20), ("adam_step", adam, 28), ("adam_step_grad_scale", lambda: adam(one), 28), ("grad_norm", norm, 4),
             ("grads_scale", scale, 8))
    for name, call, bytes_per in cases:
        med, lo, hi = event_median(call, a.reps)
        r[name] = {"median_ms": med, "min_ms": lo, "max_ms": hi, "bytes_per_element": bytes_per, "tb_per_s_at_median": bytes_per * total / med / 1e9}
        print("%-22s %.4f ms [%.4f .. %.4f]  %2d B/element  %.2f TB/s" % (name, med, lo, hi, bytes_per, r[name]["tb_per_s_at_median"]), flush=True)
    r["adam_over_sgd"] = r["adam_step"]["median_ms"] / r["sgd_momentum"]["median_ms"]
    r["adam_over_sgd_by_bytes"] = 28 / 20
    r["sgd_spread_max_over_min"] = r["sgd_momentum"]["max_ms"] / r["sgd_momentum"]["min_ms"]
    print("adam_step / sgd_momentum = %.3f (1.4 by bytes; SGD's own max / min over the repeats %.3f)"
          % (r["adam_over_sgd"], r["sgd_spread_max_over_min"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
