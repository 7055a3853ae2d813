"""Throughput of overlap-tile segmentation (tester.segment) by tile size, chunk size and arithmetic, and the share of its
time spent in the tile gather + stitch kernels.

For each image (one 4096^2 and one 696x520, the PhC-U373 frame), tile input size S in --sizes, max_batch in {4, 16} and
math in {3: fp32 Winograd (default), 2: bf16 tensors}: output megapixels/s of segment() end to end (events around the
call, after warm-up, median of --reps), and the device time of the same call's gathers and stitches alone (the same
chunks, without the forwards) as a share of it.  The 64-base-channel net, random weights.

    timeout -k 10 900 python tools/segment_time.py [--reps 3] [--json out.json]

--views times segment(views='d4') instead: one call that averages the 8 dihedral views, against the composite one would
write by hand without it (8 segment(return_probs=True) calls on apply_view(x, v).contiguous(), undo_view, a torch mean and a
threshold), at 1 x 520x696, 30 x 512^2 (the ISBI stack) and 1 x 4096^2, fp32 and bf16, automatic tile size, max_batch 16;
the same events, warm-up and median.

    timeout -k 10 900 python tools/segment_time.py --views [--reps 3] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dl-unet_amd"))

import torch  # noqa: E402
import _hip  # noqa: E402
import network  # noqa: E402
import tester  # noqa: E402


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def gather_stitch_fn(x, S, mb):
    """The gathers and stitches segment() issues for x at tile size S, chunk mb (normalised, with probabilities)."""
    L = _hip.lib()
    B, H, W = x.shape
    So = S - 184
    ny, nx, oy0, ox0 = tester.tile_grid(H, W, S)
    T = B * ny * nx
    nb = min(mb, T)
    dev = x.device
    mm = torch.empty(B, 2, device=dev)
    _hip.run("unet_minmax", dev, _hip.ptr(x), B, H * W, _hip.ptr(mm))
    tiles = torch.empty(nb, 1, S, S, device=dev)
    logits = torch.zeros(nb, 2, So, So, device=dev)
    mask = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    prob = torch.empty(B, H, W, device=dev)
    st = _hip.stream(dev)

    def fn():
        for t0 in range(0, T, nb):
            n = min(nb, T - t0)
            _hip.check(L.unet_tile_gather(_hip.ptr(x), B, H, W, _hip.ptr(mm), S, oy0, ox0, ny, nx, t0, n, _hip.ptr(tiles), st))
            _hip.check(L.unet_tile_stitch(_hip.ptr(logits), So, oy0, ox0, ny, nx, t0, n, B, H, W, _hip.ptr(mask), _hip.ptr(prob), st))
    return fn, T


def composite_d4(net, x):
    """What segment(views='d4') replaces: a segment per materialised view, brought back and averaged with torch ops."""
    acc = None
    for v in tester.parse_views('d4'):
        _, p = tester.segment(net, tester.apply_view(x, v).contiguous(), return_probs=True)
        p = tester.undo_view(p, v)
        acc = p if acc is None else acc + p
    prob = acc / 8
    return prob > 0.5, prob


def time_views(a, net, L):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    images = {"1x520x696": torch.rand(1, 520, 696, generator=g, device=dev) * 255,
              "30x512x512": torch.rand(30, 512, 512, generator=g, device=dev) * 255,
              "1x4096x4096": torch.rand(1, 4096, 4096, generator=g, device=dev) * 255}
    rows = []
    for math in (int(m) for m in a.maths.split(",")):
        _hip.check(L.unet_set_math(math), "unet_set_math")
        for name, x in images.items():
            one = median_ms(lambda: tester.segment(net, x, return_probs=True, views='d4'), a.reps, warm=1)
            torch.cuda.empty_cache()
            comp = median_ms(lambda: composite_d4(net, x), a.reps, warm=1)
            torch.cuda.empty_cache()
            rows.append({"math": math, "image": name, "views_ms": one, "composite_ms": comp, "ratio": comp / one})
            print("math %d  %-12s  segment(views='d4') %9.2f ms   composite of 8 calls %9.2f ms   composite / one call %.3f" %
                  (math, name, one, comp, comp / one), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="572,700,828,956,1212")
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--maths", default="3,2")
    ap.add_argument("--json", default=None)
    ap.add_argument("--views", action="store_true", help="time segment(views='d4') against the composite of 8 calls")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = _hip.lib()
    default_math = L.unet_get_math()
    net = network.Unet().to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    images = {"4096x4096": torch.rand(1, 4096, 4096, generator=g, device=dev) * 255,
              "520x696": torch.rand(1, 520, 696, generator=g, device=dev) * 255}
    rows = []
    if a.views:
        try:
            rows = time_views(a, net, L)
        finally:
            L.unet_set_math(default_math)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows, f, indent=1)
        return
    try:
        for math in (int(m) for m in a.maths.split(",")):
            _hip.check(L.unet_set_math(math), "unet_set_math")
            for name, x in images.items():
                for S in (int(s) for s in a.sizes.split(",")):
                    for mb in (int(b) for b in a.batches.split(",")):
                        ms = median_ms(lambda: tester.segment(net, x, tile_size=S, max_batch=mb, return_probs=True), a.reps)
                        fn, T = gather_stitch_fn(x, S, mb)
                        gs = median_ms(fn, a.reps)
                        r = {"math": math, "image": name, "S": S, "max_batch": mb, "tiles": T, "ms": ms,
                             "mpix_per_s": x[0].numel() / ms / 1e3, "gather_stitch_ms": gs, "gather_stitch_share": gs / ms,
                             "useful_fraction": (S - 184) ** 2 / S ** 2}
                        rows.append(r)
                        print("math %d  %-9s  S=%-4d mb=%-2d  tiles %3d  %9.2f ms  %7.2f Mpx/s  gather+stitch %.3f ms (%.2f %%)" %
                              (math, name, S, mb, T, ms, r["mpix_per_s"], gs, 100 * gs / ms), flush=True)
                        torch.cuda.empty_cache()
    finally:
        L.unet_set_math(default_math)
    for math in sorted({r["math"] for r in rows}):
        for name in images:
            best = max((r for r in rows if r["math"] == math and r["image"] == name), key=lambda r: r["mpix_per_s"])
            print("best math %d %s: S=%d max_batch=%d %.2f Mpx/s" % (math, name, best["S"], best["max_batch"], best["mpix_per_s"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
