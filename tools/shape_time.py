"""Device time of the ops behind functions.shape_seeds: unet_distance_map, each of the two reconstructions
(unet_reconstruct_sweeps, every launch the case needs in one call) and shape_seeds as a whole, next to unet_label_components,
unet_geodesic_sweeps and unet_grow_labels at the same shapes in the same run: B = 30, 512 x 512 and B = 8, 388 x 388.  The masks
are seeded cell images (tests/instances_ref.cells_case, the prediction's foreground), as in tools/split_time.py; h = 2, edge
'ignore'.  The geodesic growth timed is split_cells' own on the seeds shape_seeds returns.
Events around the library call alone (buffers preallocated, no host sync inside), 3 warm-ups, median, minimum and maximum of --reps;
the plane a sweep changes is restored in front of every repetition, outside the timed region.  functions.shape_seeds and
tester.split_by_shape as wall time of the whole Python call (read-backs included).  --connectivity 8 times the 8-connected
reconstructions, labelling and growth (the _conn entries; 4 goes through the same entries).

    timeout -k 10 600 python tools/shape_time.py [--reps 50] [--connectivity {4,8}] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dl-unet_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import _hip  # noqa: E402
import functions  # noqa: E402
import tester  # noqa: E402
import instances_ref  # noqa: E402
from instances_time import event_median, wall_median  # noqa: E402
from warp_time import event_median_after  # noqa: E402


def time_reconstruction(dev, marker, under, mask, reps, conn=4):
    """(init ms, sweeps ms, launches, pixels raised, finish ms, R) of one reconstruction of int32 planes inside a uint8 mask."""
    L = _hip.lib()
    B, H, W = marker.shape
    out, info = functions.reconstruct(marker, under, mask=mask, connectivity=conn)
    status = torch.empty(B, dtype=torch.int64, device=dev)
    raised = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(L.unet_reconstruct_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    init = lambda: _hip.run("unet_reconstruct_init", dev, _hip.ptr(marker), 2, _hip.ptr(under), 2, _hip.ptr(mask), 3, B, H, W, _hip.ptr(status),
                            _hip.ptr(scratch))
    init_ms = event_median(init, reps)
    plane = scratch[:B * H * W * 4]
    plane0 = plane.clone()
    n = info.launches
    slots = torch.empty(n, B, dtype=torch.int32, device=dev)
    sweeps = lambda: _hip.run("unet_reconstruct_sweeps_conn", dev, B, H, W, conn, n, _hip.ptr(slots), 0, _hip.ptr(scratch))
    sweeps_ms = event_median_after(lambda: plane.copy_(plane0), sweeps, reps)
    assert bool(slots[:-1].any(dim=1).all()) and not bool(slots[-1].any())
    res = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    finish_ms = event_median(lambda: _hip.run("unet_reconstruct_finish", dev, B, H, W, _hip.ptr(res), _hip.ptr(raised), _hip.ptr(scratch)), reps)
    assert torch.equal(res, out)
    return init_ms, sweeps_ms, n, int(info.raised.sum()), finish_ms, out


def time_case(dev, B, H, W, cells, reps, h=2.0, conn=4):
    L = _hip.lib()
    mask = torch.from_numpy(np.stack([instances_ref.cells_case(100 + b % 6, cells, H, W)[1] > 0 for b in range(B)]).astype(np.uint8)).to(dev)
    r = {"B": B, "H": H, "W": W, "cells": cells, "h": h, "connectivity": conn, "components": int(functions.label_cells(mask)[1].sum())}
    labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    nobj = torch.empty(B, dtype=torch.int32, device=dev)
    lscr = torch.empty(L.unet_label_components_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    mask64 = mask.long()
    r["label_ms"] = event_median(lambda: _hip.run("unet_label_components", dev, _hip.ptr(mask64), 0, B, H, W, _hip.ptr(labels), _hip.ptr(nobj),
                                                  _hip.ptr(lscr)), reps)
    seeds, n_seeds = functions.shape_seeds(mask, h, connectivity=conn)
    r["seeds"] = int(n_seeds.sum())
    gscr = torch.empty(L.unet_grow_labels_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    r["grow_ms"] = event_median(lambda: _hip.run("unet_grow_labels", dev, _hip.ptr(seeds), B, H, W, -1, _hip.ptr(labels), _hip.ptr(gscr)), reps)

    out, info = functions.split_cells(seeds, mask, connectivity=conn)                                # the growth these seeds are for
    r["geodesic_launches"], r["cells_after"] = info.launches, int(sum(len(np.unique(o)) - 1 for o in out.cpu().numpy()))
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int64, device=dev)
    escr = torch.empty(L.unet_geodesic_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    _hip.run("unet_geodesic_init", dev, _hip.ptr(seeds), _hip.ptr(mask), 3, B, H, W, _hip.ptr(counts), _hip.ptr(status), _hip.ptr(escr))
    keys = escr[:B * H * W * 8]
    keys0 = keys.clone()
    gslots = torch.empty(info.launches, B, dtype=torch.int32, device=dev)
    r["geodesic_ms"] = event_median_after(lambda: keys.copy_(keys0), lambda: _hip.run("unet_geodesic_sweeps_conn", dev, B, H, W, -1, conn, info.launches,
                                                                                      _hip.ptr(gslots), 0, _hip.ptr(escr)), reps)

    d2 = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    dscr = torch.empty(L.unet_distance_map_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    for name, edge in (("distance_ms", 0), ("distance_background_ms", 1)):
        r[name] = event_median(lambda: _hip.run("unet_distance_map", dev, _hip.ptr(mask), 3, B, H, W, edge, _hip.ptr(d2), _hip.ptr(dscr)), reps)
    _hip.run("unet_distance_map", dev, _hip.ptr(mask), 3, B, H, W, 0, _hip.ptr(d2), _hip.ptr(dscr))
    r["max_distance"] = float(d2.max().item()) ** 0.5
    hq = int(round(16 * h))
    q, lifted, lowered = torch.empty_like(d2), torch.empty_like(d2), torch.empty_like(d2)
    r["heights_ms"] = event_median(lambda: _hip.run("unet_shape_heights", dev, _hip.ptr(d2), B, H, W, hq, _hip.ptr(q), _hip.ptr(lifted)), reps)
    r["r1_init_ms"], r["r1_sweeps_ms"], r["r1_launches"], r["r1_raised"], r["r1_finish_ms"], r1 = time_reconstruction(dev, q, lifted, mask, reps, conn)
    r["lower_ms"] = event_median(lambda: _hip.run("unet_shape_lower", dev, _hip.ptr(r1), B, H, W, 1, _hip.ptr(lowered)), reps)
    r["r2_init_ms"], r["r2_sweeps_ms"], r["r2_launches"], r["r2_raised"], r["r2_finish_ms"], r2 = time_reconstruction(dev, lowered, r1, mask, reps, conn)
    peaks = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    r["maxima_ms"] = event_median(lambda: _hip.run("unet_shape_maxima", dev, _hip.ptr(r1), _hip.ptr(r2), B, H, W, 0, _hip.ptr(peaks)), reps)
    assert torch.equal(functions.label_cells(peaks, connectivity=conn)[0], seeds)
    r["shape_seeds_wall_ms"] = wall_median(lambda: functions.shape_seeds(mask, h, connectivity=conn), max(3, reps // 5))
    r["split_by_shape_wall_ms"] = wall_median(lambda: tester.split_by_shape(mask, h, connectivity=conn), max(3, reps // 5))
    r["device_ms"] = sum(r[k][0] for k in ("distance_ms", "heights_ms", "r1_init_ms", "r1_sweeps_ms", "r1_finish_ms", "lower_ms", "r2_init_ms",
                                           "r2_sweeps_ms", "r2_finish_ms", "maxima_ms", "label_ms"))
    for other in ("label_ms", "geodesic_ms", "grow_ms"):
        for mine in ("distance_ms", "r1_sweeps_ms", "r2_sweeps_ms"):
            r["%s_over_%s" % (mine[:-3], other[:-3])] = r[mine][0] / r[other][0]
        r["device_over_%s" % other[:-3]] = r["device_ms"] / r[other][0]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--connectivity", type=int, choices=(4, 8), default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = []
    for B, H, W, cells in ((30, 512, 512, 170), (8, 388, 388, 99)):
        r = time_case(dev, B, H, W, cells, a.reps, conn=a.connectivity)
        res.append(r)
        print("connectivity %d | B %d, %d x %d: %d components -> %d seeds -> %d cells, largest distance %.1f | label %.3f ms | geodesic sweeps %.3f ms (%d launches) | "
              "grow_labels %.3f ms | distance_map %.3f ms (background %.3f) | heights %.3f ms | R1: init %.3f, sweeps %.3f (%d launches, %d raised), "
              "finish %.3f ms | lower %.3f ms | R2: init %.3f, sweeps %.3f (%d launches, %d raised), finish %.3f ms | maxima %.3f ms | "
              "device total with the labelling %.3f ms | shape_seeds %.2f ms wall | split_by_shape %.2f ms wall"
              % (a.connectivity, B, H, W, r["components"], r["seeds"], r["cells_after"], r["max_distance"], r["label_ms"][0], r["geodesic_ms"][0],
                 r["geodesic_launches"], r["grow_ms"][0], r["distance_ms"][0], r["distance_background_ms"][0], r["heights_ms"][0],
                 r["r1_init_ms"][0], r["r1_sweeps_ms"][0], r["r1_launches"], r["r1_raised"], r["r1_finish_ms"][0], r["lower_ms"][0],
                 r["r2_init_ms"][0], r["r2_sweeps_ms"][0], r["r2_launches"], r["r2_raised"], r["r2_finish_ms"][0], r["maxima_ms"][0],
                 r["device_ms"], r["shape_seeds_wall_ms"], r["split_by_shape_wall_ms"]), flush=True)
        print("   ratios: " + ", ".join("%s %.2f" % (k, v) for k, v in r.items() if "_over_" in k), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
