"""Device time of the per-cell table: unet_cell_sums without an image, with a uint8 and with a float32 image, and
unet_remap_labels, next to unet_label_components on the same input (the mask labels != 0) in the same run, and next to the host
route a user takes today: labels.cpu() and image.cpu() plus the scipy.ndimage calls of tests/measure_ref.scipy_route (wall clock).
Shapes: B = 30, 512 x 512 and B = 1, 4096 x 4096, each with about 10, 100 and 1000 cells per image (seeded discs painted in
turn, ids 1..n).  Events around the library call alone (buffers preallocated, no host sync inside), 3 warm-ups, median, minimum
and maximum of --reps.  The structural claim, that the device time at a fixed size does not grow with the number of cells, is the
comparison of the three rows of a shape.

    timeout -k 10 900 python tools/measure_time.py [--reps 30] [--host-reps 2] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dl-unet_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import _hip  # noqa: E402
import functions  # noqa: E402
import measure_ref  # noqa: E402
from instances_time import event_median  # noqa: E402


def cells(seed, B, H, W, n):
    """[B,H,W] int32: n discs per image painted in turn inside their own windows (cheap at 4096 x 4096), ids 1..n."""
    rs = np.random.RandomState(seed)
    out = np.zeros((B, H, W), np.int32)
    rmax = max(2.0, 0.4 * np.sqrt(H * W / n))
    for b in range(B):
        for i in range(1, n + 1):
            cy, cx, r = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(0.5 * rmax, rmax)
            y0, y1, x0, x1 = max(0, int(cy - r)), min(H, int(cy + r) + 2), max(0, int(cx - r)), min(W, int(cx + r) + 2)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            out[b, y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = i
    return out


def time_case(dev, name, lab_np, reps, host_reps):
    L = _hip.lib()
    B, H, W = lab_np.shape
    n_max = int(lab_np.max())
    N = n_max + 1
    rs = np.random.RandomState(1)
    img8_np = rs.randint(0, 256, lab_np.shape).astype(np.uint8)
    lab, img8 = torch.from_numpy(lab_np).to(dev), torch.from_numpy(img8_np).to(dev)
    imgf = img8.float() * 0.37 - 11.0
    r = {"name": name, "B": B, "H": H, "W": W, "cells": n_max, "foreground": float((lab_np != 0).mean())}
    area = torch.empty(B, N, dtype=torch.int64, device=dev)
    bbox = torch.empty(B, N, 4, dtype=torch.int32, device=dev)
    moments = torch.empty(B, N, 5, dtype=torch.int64, device=dev)
    edges = torch.empty(B, N, 3, dtype=torch.int64, device=dev)
    vsum = torch.empty(B, N, 2, dtype=torch.int64, device=dev)
    vrange = torch.empty(B, N, 2, dtype=torch.int32, device=dev)
    present = torch.empty(B, N, dtype=torch.bool, device=dev)
    status = torch.empty(B, 2, dtype=torch.int64, device=dev)
    scr = torch.empty(L.unet_cell_sums_scratch_bytes(B, n_max), dtype=torch.uint8, device=dev)

    def sums(img, code):
        return lambda: _hip.run("unet_cell_sums", dev, _hip.ptr(lab), 2, _hip.ptr(img), code, B, H, W, n_max, _hip.ptr(area), _hip.ptr(bbox),
                                _hip.ptr(moments), _hip.ptr(edges), _hip.ptr(vsum), _hip.ptr(vrange), _hip.ptr(present), _hip.ptr(status),
                                _hip.ptr(scr))
    r["sums_ms"] = event_median(sums(None, 0), reps)
    r["sums_uint8_ms"] = event_median(sums(img8, 3), reps)
    assert int(status.sum()) == 0 and int(area.sum()) == B * H * W and int(vsum[..., 0].sum()) == int(img8_np.sum(dtype=np.int64))
    r["sums_float_ms"] = event_median(sums(imgf, 1), reps)
    table = torch.arange(N, dtype=torch.int32, device=dev)
    out = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    r["remap_ms"] = event_median(lambda: _hip.run("unet_remap_labels", dev, _hip.ptr(lab), 2, B, H, W, _hip.ptr(table), n_max, 0, _hip.ptr(out),
                                                  _hip.ptr(status)), reps)
    assert torch.equal(out, lab)
    mask64 = (lab != 0).long()
    labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    nobj = torch.empty(B, dtype=torch.int32, device=dev)
    lscr = torch.empty(L.unet_label_components_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    r["label_ms"] = event_median(lambda: _hip.run("unet_label_components", dev, _hip.ptr(mask64), 0, B, H, W, _hip.ptr(labels), _hip.ptr(nobj),
                                                  _hip.ptr(lscr)), reps)

    def wrapper():
        functions.props_from_sums(functions.cell_sums(lab, imgf, n_max=n_max))
    ts = []
    for _ in range(max(1, host_reps)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wrapper()
        ts.append((time.perf_counter() - t0) * 1e3)
    r["cell_props_wall_ms"] = min(ts)

    def host():
        l, f = lab.cpu().numpy(), imgf.cpu().numpy()
        for b in range(B):
            measure_ref.scipy_route(l[b], f[b], n_max)
    ts = []
    for _ in range(host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()
        ts.append((time.perf_counter() - t0) * 1e3)
    r["host_scipy_wall_ms"] = min(ts) if ts else None
    for k in ("sums_ms", "sums_uint8_ms", "sums_float_ms", "remap_ms"):
        r[k[:-3] + "_over_label"] = r[k][0] / r["label_ms"][0]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = []
    for B, S in ((30, 512), (1, 4096)):
        for n in (10, 100, 1000):
            r = time_case(dev, "%dx%dx%d, %d cells" % (B, S, S, n), cells(n, B, S, S, n), a.reps, a.host_reps)
            res.append(r)
            print("%-26s fg %.2f | cell_sums %.3f ms, uint8 image %.3f, float image %.3f | remap %.3f | label_components %.3f | "
                  "cell_props wall %.1f ms | host scipy route wall %s ms"
                  % (r["name"], r["foreground"], r["sums_ms"][0], r["sums_uint8_ms"][0], r["sums_float_ms"][0], r["remap_ms"][0], r["label_ms"][0],
                     r["cell_props_wall_ms"], "%.1f" % r["host_scipy_wall_ms"] if r["host_scipy_wall_ms"] is not None else "-"), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
