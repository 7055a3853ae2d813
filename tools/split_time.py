"""Device time of the sweeps behind functions.split_cells (unet_geodesic_sweeps), next to unet_label_components (what
segment(return_instances=True) pays today) and unet_grow_labels (the growth in the plane) at the same shapes in the same run:
B = 30, 512 x 512 and B = 8, 388 x 388.  The masks are seeded cell images (tests/instances_ref.cells_case, the prediction's
foreground); the seeds are the cells eroded by 5 px: the mask pixels that functions.grow_cells(background, 5) does not reach,
labelled.  One call of unet_geodesic_sweeps enqueues every launch the growth needs (the number is taken from functions.split_cells
first; the final launch that changes nothing included), the key plane restored in front of every repetition outside the timed
region; and two launches on the converged state.
Events around the library call alone (buffers preallocated, no host sync inside), 3 warm-ups, median, minimum and maximum of --reps.
functions.split_cells as wall time of the whole Python call (read-backs included).  --connectivity 8 times the 8-connected growth
(unet_geodesic_sweeps_conn; 4 goes through the same entry).

    timeout -k 10 600 python tools/split_time.py [--reps 50] [--connectivity {4,8}] [--json out.json]
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
import instances_ref  # noqa: E402
from instances_time import event_median, wall_median  # noqa: E402
from warp_time import event_median_after  # noqa: E402


def time_case(dev, B, H, W, cells, reps, erode=5, conn=4):
    L = _hip.lib()
    mask = torch.from_numpy(np.stack([instances_ref.cells_case(100 + b % 6, cells, H, W)[1] > 0 for b in range(B)]).astype(np.uint8)).to(dev)
    near_bg = functions.grow_cells((mask == 0).int(), erode)
    seeds, n_seeds = functions.label_cells((mask != 0) & (near_bg == 0))
    r = {"B": B, "H": H, "W": W, "cells": cells, "erode": erode, "connectivity": conn, "seeds": int(n_seeds.sum()),
         "components": int(functions.label_cells(mask)[1].sum())}
    labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    nobj = torch.empty(B, dtype=torch.int32, device=dev)
    lscr = torch.empty(L.unet_label_components_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    mask64 = mask.long()
    r["label_ms"] = event_median(lambda: _hip.run("unet_label_components", dev, _hip.ptr(mask64), 0, B, H, W, _hip.ptr(labels), _hip.ptr(nobj),
                                                  _hip.ptr(lscr)), reps)
    gscr = torch.empty(L.unet_grow_labels_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    for name, d2 in (("grow_unlimited_ms", -1), ("grow_reach5_ms", 25)):
        r[name] = event_median(lambda: _hip.run("unet_grow_labels", dev, _hip.ptr(seeds), B, H, W, d2, _hip.ptr(labels), _hip.ptr(gscr)), reps)

    out, info = functions.split_cells(seeds, mask, connectivity=conn)
    r["launches"], r["unreached"], r["max_distance"] = info.launches, int(info.unreached.sum()), int(info.max_distance.max())
    r["cells_after"] = int(sum(len(np.unique(o)) - 1 for o in out.cpu().numpy()))
    counts = torch.empty(3, B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int64, device=dev)
    scratch = torch.empty(L.unet_geodesic_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    init = lambda: _hip.run("unet_geodesic_init", dev, _hip.ptr(seeds), _hip.ptr(mask), 3, B, H, W, _hip.ptr(counts[0]), _hip.ptr(status),
                            _hip.ptr(scratch))
    r["init_ms"] = event_median(init, reps)
    plane = scratch[:B * H * W * 8]
    plane0 = plane.clone()
    n = info.launches
    slots = torch.empty(n, B, dtype=torch.int32, device=dev)
    sweeps = lambda k=n: _hip.run("unet_geodesic_sweeps_conn", dev, B, H, W, -1, conn, k, _hip.ptr(slots), 0, _hip.ptr(scratch))
    r["sweeps_ms"] = event_median_after(lambda: plane.copy_(plane0), sweeps, reps)
    assert bool(slots[:-1].any(dim=1).all()) and not bool(slots[-1].any())
    r["lowered"] = int(slots.sum())
    r["idle_launches_ms"] = event_median(lambda: sweeps(2), reps)                   # the state is converged now: two no-op launches
    assert not bool(slots[0].any())
    dist = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    r["finish_ms"] = event_median(lambda: _hip.run("unet_geodesic_finish", dev, B, H, W, -1, _hip.ptr(labels), _hip.ptr(dist), _hip.ptr(counts[1]),
                                                   _hip.ptr(counts[2]), _hip.ptr(scratch)), reps)
    assert torch.equal(labels, out)
    r["split_cells_wall_ms"] = wall_median(lambda: functions.split_cells(seeds, mask, connectivity=conn), max(3, reps // 5))
    r["sweeps_over_label"] = r["sweeps_ms"][0] / r["label_ms"][0]
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
        print("connectivity %d | B %d, %d x %d: %d components, %d seeds -> %d cells, %d unreached, largest distance %d | label %.3f ms | grow_labels %.3f ms "
              "(reach 5: %.3f) | init %.3f ms | sweeps to convergence %.3f ms (%d launches, %d keys lowered) = %.2f x label | "
              "two idle launches %.4f ms | finish %.3f ms | split_cells %.2f ms wall"
              % (a.connectivity, B, H, W, r["components"], r["seeds"], r["cells_after"], r["unreached"], r["max_distance"], r["label_ms"][0],
                 r["grow_unlimited_ms"][0], r["grow_reach5_ms"][0], r["init_ms"][0], r["sweeps_ms"][0], r["launches"], r["lowered"],
                 r["sweeps_over_label"], r["idle_launches_ms"][0], r["finish_ms"][0], r["split_cells_wall_ms"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
