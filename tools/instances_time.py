"""Device time of functions.label_cells (unet_label_components) and functions.seg_measure (unet_instance_overlap) after
warm-up, next to the host route on the same data, at 388^2, 520 x 696 and 4096^2 with 10, 100 and 1000 blobs each:
  label_cells   events around the library call alone (buffers preallocated, no host sync inside)
  overlap       events around unet_instance_overlap alone, on the device labels against a shifted copy as ground truth
  seg_measure   wall time of the whole Python call (two read-backs: the maxima, then the integers)
  host          wall time of mask.cpu() + scipy.ndimage.label, and of the numpy restatement tests/instances_ref.seg
Median of --reps (host: of --host-reps).  The structural claim to look at: at a fixed image size the device columns should
not grow with the blob count.

    timeout -k 10 600 python tools/instances_time.py [--reps 30] [--host-reps 3] [--json out.json]
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
import instances_ref as ref  # noqa: E402


def blobs(seed, n, H, W):
    """n discs on a jittered grid, small enough not to touch: n components."""
    rs = np.random.RandomState(seed)
    ny = max(1, int(round(np.sqrt(n * H / W))))
    nx = -(-n // ny)
    py, px = H / ny, W / nx
    r = max(1.0, 0.3 * min(py, px))
    m = np.zeros((H, W), bool)
    for k in range(n):
        cy = (k // nx + 0.5) * py + rs.uniform(-0.1, 0.1) * py
        cx = (k % nx + 0.5) * px + rs.uniform(-0.1, 0.1) * px
        y0, y1, x0, x1 = int(max(0, cy - r - 1)), int(min(H, cy + r + 2)), int(max(0, cx - r - 1)), int(min(W, cx + r + 2))
        yy, xx = np.mgrid[y0:y1, x0:x1]
        m[y0:y1, x0:x1] |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return m


def event_median(call, reps):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); call(); b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0], ms[-1]


def wall_median(call, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def time_case(dev, H, W, n, reps, host_reps):
    L = _hip.lib()
    mask_np = blobs(n, n, H, W)
    mask = torch.from_numpy(mask_np.astype(np.int64))[None].to(dev)
    labels = torch.empty(1, H, W, dtype=torch.int32, device=dev)
    nobj = torch.empty(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(L.unet_label_components_scratch_bytes(1, H, W), dtype=torch.uint8, device=dev)
    lab_ms = event_median(lambda: _hip.run("unet_label_components", dev, _hip.ptr(mask), 0, 1, H, W, _hip.ptr(labels), _hip.ptr(nobj),
                                           _hip.ptr(scratch)), reps)
    count = int(nobj.item())
    gt = torch.roll(labels, shifts=(2, 1), dims=(1, 2)).contiguous()          # the same cells two rows down, one column right
    slots = 1 << (8 * count + 1024 - 1).bit_length()
    outs = [torch.empty(1, count + 1, dtype=torch.int32, device=dev) for _ in range(4)]
    status = torch.empty(1, 2, dtype=torch.int64, device=dev)
    oscr = torch.empty(L.unet_instance_overlap_scratch_bytes(1, count, count, slots), dtype=torch.uint8, device=dev)
    ov_ms = event_median(lambda: _hip.run("unet_instance_overlap", dev, _hip.ptr(gt), _hip.ptr(labels), 1, H, W, count, count, slots,
                                          *(_hip.ptr(o) for o in outs), _hip.ptr(status), _hip.ptr(oscr)), reps)
    assert status.cpu().tolist() == [[0, 0]]
    seg = functions.seg_measure(labels, gt)
    seg_ms = wall_median(lambda: functions.seg_measure(labels, gt), max(3, reps // 3))
    host_lab_ms = wall_median(lambda: ref.label(mask[0].cpu().numpy()), host_reps)
    gt_np, lab_np = gt.cpu().numpy(), labels.cpu().numpy()
    host_seg_ms = wall_median(lambda: ref.seg(gt_np, lab_np), host_reps)
    return {"H": H, "W": W, "blobs": n, "components": count, "label_ms": lab_ms[0], "label_min_ms": lab_ms[1], "label_max_ms": lab_ms[2],
            "overlap_ms": ov_ms[0], "overlap_min_ms": ov_ms[1], "overlap_max_ms": ov_ms[2], "seg_measure_wall_ms": seg_ms,
            "host_label_ms": host_lab_ms, "host_seg_ms": host_seg_ms, "seg": float(seg.seg), "n_matched": seg.n_matched}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = []
    print("%-11s %6s | %9s %9s %11s | %10s %9s" % ("size", "blobs", "label ms", "overlap", "seg_measure", "host label", "host seg"))
    for H, W in ((388, 388), (520, 696), (4096, 4096)):
        for n in (10, 100, 1000):
            r = time_case(dev, H, W, n, a.reps, a.host_reps)
            res.append(r)
            print("%4dx%-6d %6d | %9.4f %9.4f %11.3f | %10.2f %9.2f   (%d components, SEG %.4f)" %
                  (H, W, n, r["label_ms"], r["overlap_ms"], r["seg_measure_wall_ms"], r["host_label_ms"], r["host_seg_ms"],
                   r["components"], r["seg"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
