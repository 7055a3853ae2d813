"""Device time of the boundary scores: unet_surface_sums (buffers preallocated, events around the library call alone, no host sync
inside) and the wall time of functions.boundary_scores, next to the route a user of this package had before, timed in the same
run: the two contours by ATen shifts and compares, functions.distance_map of the complement of each contour (the full-plane row
scan), boolean-mask gathers, torch.quantile, max, mean and a count per image and direction, and one read-back.  Inputs: the
foreground masks of instances_ref.cells_case (prediction against ground truth) and the ground truth against itself shifted by 2
pixels, 30 x 512 x 512 and 8 x 388 x 388.  3 warm-ups, median, minimum and maximum of --reps.

    timeout -k 10 600 python tools/boundary_time.py [--reps 30] [--json profiles/boundary_time.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dl-unet_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import _hip  # noqa: E402
import functions  # noqa: E402
import instances_ref  # noqa: E402
from hull_time import wall  # noqa: E402
from instances_time import event_median  # noqa: E402


def aten_contour(m):
    """bool [B,H,W]: region pixels with a 4-neighbour outside the region, pixels past the image being outside"""
    p = F.pad(m, (1, 1, 1, 1))
    return m & ~(p[:, :-2, 1:-1] & p[:, 2:, 1:-1] & p[:, 1:-1, :-2] & p[:, 1:-1, 2:])


def old_route(pred, gt, tol2=1):
    """[B, 2, 4] float64 on the host: per image and direction max, 95th percentile, mean distance and share within the tolerance"""
    cp, cg = aten_contour(pred != 0), aten_contour(gt != 0)
    d_to_g = functions.distance_map((~cg).to(torch.uint8), edge='ignore')
    d_to_p = functions.distance_map((~cp).to(torch.uint8), edge='ignore')
    rows = []
    for b in range(pred.shape[0]):
        for on, d2 in ((cp[b], d_to_g[b]), (cg[b], d_to_p[b])):
            v = d2[on]
            d = v.double().sqrt()
            rows.append(torch.stack([d.max(), torch.quantile(d, 0.95), d.mean(), (v <= tol2).double().mean()]))
    return torch.stack(rows).view(-1, 2, 4).cpu().numpy()


def time_case(dev, name, pred_np, gt_np, reps):
    L = _hip.lib()
    B, H, W = pred_np.shape
    pred, gt = torch.from_numpy(pred_np).to(dev), torch.from_numpy(gt_np).to(dev)
    r = {"name": name, "B": B, "H": H, "W": W}
    record = torch.empty(B, 2, 10, dtype=torch.int64, device=dev)
    scratch = torch.empty(L.unet_surface_sums_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    t2 = (ctypes.c_int * 4)(1, 4, 0, 0)
    r["surface_sums_ms"] = event_median(lambda: _hip.run("unet_surface_sums", dev, _hip.ptr(pred), 3, -1, _hip.ptr(gt), 3, -1, B, H, W, 4, 1, 19, 20,
                                                         t2, 2, _hip.ptr(record), None, None, _hip.ptr(scratch)), reps)
    first = record.clone()
    _hip.run("unet_surface_sums", dev, _hip.ptr(pred), 3, -1, _hip.ptr(gt), 3, -1, B, H, W, 4, 1, 19, 20, t2, 2, _hip.ptr(record), None, None,
             _hip.ptr(scratch))
    assert torch.equal(first, record)
    rec = record.cpu().numpy()
    r["contour_pixels"] = int(rec[:, :, 0].sum())
    r["contour_share"] = r["contour_pixels"] / (2.0 * B * H * W)
    r["max_d2"] = int(rec[:, :, 1].max())
    r["boundary_scores_wall_ms"] = wall(lambda: functions.boundary_scores(pred, gt, tolerances=(1.0, 2.0)), 5)
    got = []
    r["old_route_wall_ms"] = wall(lambda: got.append(old_route(pred, gt)), 5)
    new = functions.boundary_scores(pred, gt, tolerances=(1.0,))
    assert np.array_equal(np.sqrt(rec[:, :, 1].astype(np.float64)), got[0][:, :, 0])                # the same maxima both ways
    n = rec[:, :, 0].astype(np.float64)
    assert np.allclose((got[0][:, :, 2] * n).sum(axis=1) / n.sum(axis=1), new.assd, rtol=1e-9, atol=0)      # and the same mean distance
    r["hausdorff_mean"], r["hd95_mean"], r["assd_mean"], r["nsd1_mean"] = (float(np.mean(v)) for v in (new.hausdorff, new.hd_percentile, new.assd,
                                                                                                      new.nsd[:, 0]))
    r["old_over_new_wall"] = r["old_route_wall_ms"] / r["boundary_scores_wall_ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = []
    for B, S, n in ((30, 512, 170), (8, 388, 100)):
        pairs = [instances_ref.cells_case(100 + b % 6, n, S, S) for b in range(B)]
        gt = np.stack([g > 0 for g, _ in pairs]).astype(np.uint8)
        pred = np.stack([p > 0 for _, p in pairs]).astype(np.uint8)
        shifted = np.zeros_like(gt)
        shifted[:, :, 2:] = gt[:, :, :-2]
        for what, p in (("cells", pred), ("shifted by 2", shifted)):
            r = time_case(dev, "%dx%dx%d %s" % (B, S, S, what), p, gt, a.reps)
            res.append(r)
            print("%-24s contour %.1f%% of the pixels, max d2 %d | unet_surface_sums %.3f ms (min %.3f, max %.3f) | boundary_scores wall %.2f ms | "
                  "distance_map + ATen + quantile wall %.2f ms | HD %.2f HD95 %.2f ASSD %.3f NSD@1 %.3f"
                  % (r["name"], 100 * r["contour_share"], r["max_d2"], *r["surface_sums_ms"], r["boundary_scores_wall_ms"], r["old_route_wall_ms"],
                     r["hausdorff_mean"], r["hd95_mean"], r["assd_mean"], r["nsd1_mean"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
