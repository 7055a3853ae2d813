"""Device time of the seeded watershed (functions.watershed: unet_flood_init / unet_flood_sweeps / unet_flood_assign /
unet_flood_finish) at B = 30, 512 x 512 and B = 8, 388 x 388, with 16, 64 and 256 levels, next to what the same seeds cost without
it in the same run: one geodesic growth (unet_geodesic_sweeps, blind to the image) and the level loop over functions.split_cells
(for h = 0 .. levels - 1: labels = split_cells(labels, mask & (v <= h | labels > 0))), which computes the same labels and is what
the library could do before the fused op.  The masks are seeded cell images (tests/instances_ref.cells_case, the prediction's
foreground) and the seeds the cells eroded by 5 px, as in tools/split_time.py; the landscape is float32, 0.9 * (1 - r / max r) with
r the distance to the background (functions.distance_map) plus 0.1 * seeded uniform noise: low in the middle of a cell, rising to
its rim, rough enough for minimax paths to meander.
Each stage is one library call that enqueues every launch the stage needs (the numbers are taken from functions.watershed first; the
final launch that changes nothing included), its plane restored in front of every repetition outside the timed region.  Events around
the library call alone (buffers preallocated, no host sync inside), 3 warm-ups, median, minimum and maximum of --reps.  The level loop
and functions.watershed as wall time of the whole Python call (read-backs included); the loop's labels are compared with the
watershed's.  --connectivity 8 times the 8-connected flood and growth (the _conn entries; 4 goes through the same entries).

    timeout -k 10 900 python tools/flood_time.py [--reps 30] [--connectivity {4,8}] [--json out.json]
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

LEVELS = (16, 64, 256)


def align256(n):
    return (n + 255) // 256 * 256


def inputs(dev, B, H, W, cells, erode):
    mask = torch.from_numpy(np.stack([instances_ref.cells_case(100 + b % 6, cells, H, W)[1] > 0 for b in range(B)]).astype(np.uint8)).to(dev)
    near_bg = functions.grow_cells((mask == 0).int(), erode)
    seeds, n_seeds = functions.label_cells((mask != 0) & (near_bg == 0))
    r = functions.distance_map(mask).float().sqrt()
    noise = torch.from_numpy(np.random.RandomState(9).rand(B, H, W).astype(np.float32)).to(dev)
    image = 0.9 * (1 - r / r.amax(dim=(1, 2), keepdim=True).clamp(min=1)) + 0.1 * noise
    return mask, seeds, int(n_seeds.sum()), image.contiguous()


def level_loop(seeds, v, region, levels, conn=4):
    labels = torch.where(region, seeds, torch.zeros_like(seeds))
    for h in range(levels):
        labels = functions.split_cells(labels, region & ((v <= h) | (labels > 0)), connectivity=conn)[0]
    return labels


def time_case(dev, B, H, W, cells, reps, erode=5, conn=4):
    L = _hip.lib()
    mask, seeds, n_seeds, image = inputs(dev, B, H, W, cells, erode)
    npx = B * H * W
    res = {"B": B, "H": H, "W": W, "cells": cells, "erode": erode, "connectivity": conn, "seeds": n_seeds, "levels": {}}
    counts = torch.empty(3, B, dtype=torch.int32, device=dev)
    labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)

    out, info = functions.split_cells(seeds, mask, connectivity=conn)                                    # the geodesic growth of the same seeds
    gscr = torch.empty(L.unet_geodesic_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    gstatus = torch.empty(B, dtype=torch.int64, device=dev)
    _hip.run("unet_geodesic_init", dev, _hip.ptr(seeds), _hip.ptr(mask), 3, B, H, W, _hip.ptr(counts[0]), _hip.ptr(gstatus), _hip.ptr(gscr))
    gplane = gscr[:npx * 8]
    gplane0 = gplane.clone()
    gslots = torch.empty(info.launches, B, dtype=torch.int32, device=dev)
    res["geodesic_launches"] = info.launches
    res["geodesic_ms"] = event_median_after(lambda: gplane.copy_(gplane0), lambda: _hip.run(
        "unet_geodesic_sweeps_conn", dev, B, H, W, -1, conn, info.launches, _hip.ptr(gslots), 0, _hip.ptr(gscr)), reps)
    assert bool(gslots[:-1].any(dim=1).all()) and not bool(gslots[-1].any())

    scratch = torch.empty(L.unet_flood_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    status = torch.empty(2, B, dtype=torch.int64, device=dev)
    keys, ids = scratch[:npx * 8], scratch[2 * align256(npx * 8):][:npx * 4]         # plane 0 of each pair
    lev, dist = torch.empty(2, B, H, W, dtype=torch.int32, device=dev)
    for levels in LEVELS:
        r = res["levels"][levels] = {}
        want, finfo = functions.watershed(seeds, image, mask=mask, levels=levels, connectivity=conn)
        n1, n2 = r["launches"] = finfo.launches
        r["unreached"], r["max_level"] = int(finfo.unreached.sum()), int(finfo.max_level.max())
        init = lambda: _hip.run("unet_flood_init", dev, _hip.ptr(seeds), _hip.ptr(image), 1, levels, _hip.ptr(mask), 3, B, H, W,
                                _hip.ptr(counts[0]), _hip.ptr(status), _hip.ptr(scratch))
        r["init_ms"] = event_median(init, reps)
        keys0, ids0 = keys.clone(), ids.clone()
        slots1 = torch.empty(n1, B, dtype=torch.int32, device=dev)
        r["stage1_ms"] = event_median_after(lambda: keys.copy_(keys0), lambda: _hip.run(
            "unet_flood_sweeps_conn", dev, B, H, W, -1, conn, n1, _hip.ptr(slots1), 0, _hip.ptr(scratch)), reps)
        assert bool(slots1[:-1].any(dim=1).all()) and not bool(slots1[-1].any())
        slots2 = torch.empty(n2, B, dtype=torch.int32, device=dev)
        r["stage2_ms"] = event_median_after(lambda: ids.copy_(ids0), lambda: _hip.run(
            "unet_flood_assign_conn", dev, B, H, W, conn, n2, _hip.ptr(slots2), 0, _hip.ptr(scratch)), reps)
        assert bool(slots2[:-1].any(dim=1).all()) and not bool(slots2[-1].any())
        r["lowered"] = (int(slots1.sum()), int(slots2.sum()))
        r["finish_ms"] = event_median(lambda: _hip.run("unet_flood_finish", dev, B, H, W, _hip.ptr(labels), _hip.ptr(lev), _hip.ptr(dist),
                                                       _hip.ptr(counts[1]), _hip.ptr(counts[2]), _hip.ptr(scratch)), reps)
        assert torch.equal(labels, want)
        r["device_ms"] = r["init_ms"][0] + r["stage1_ms"][0] + r["stage2_ms"][0] + r["finish_ms"][0]
        r["watershed_wall_ms"] = wall_median(lambda: functions.watershed(seeds, image, mask=mask, levels=levels, connectivity=conn), max(3, reps // 5))
        v = (image * float(levels)).floor().clamp(0, levels - 1).int()                # the kernel's rule, the product in fp32
        region = mask != 0
        assert torch.equal(level_loop(seeds, v, region, levels, conn), want)
        r["level_loop_wall_ms"] = wall_median(lambda: level_loop(seeds, v, region, levels, conn), 3)
        r["loop_over_watershed"] = r["level_loop_wall_ms"] / r["watershed_wall_ms"]
        r["device_over_geodesic"] = r["device_ms"] / res["geodesic_ms"][0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--connectivity", type=int, choices=(4, 8), default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = []
    for B, H, W, cells in ((30, 512, 512, 170), (8, 388, 388, 99)):
        c = time_case(dev, B, H, W, cells, a.reps, conn=a.connectivity)
        res.append(c)
        print("connectivity %d | B %d, %d x %d: %d seeds | geodesic sweeps %.3f ms (%d launches)" % (a.connectivity, B, H, W, c["seeds"], c["geodesic_ms"][0], c["geodesic_launches"]),
              flush=True)
        for levels, r in c["levels"].items():
            print("  %3d levels: init %.3f ms | stage 1 %.3f ms (%d launches) | stage 2 %.3f ms (%d launches) | finish %.3f ms | device total "
                  "%.3f ms = %.2f x geodesic | watershed %.2f ms wall | level loop over split_cells %.1f ms wall = %.1f x watershed | "
                  "%d unreached, top level %d"
                  % (levels, r["init_ms"][0], r["stage1_ms"][0], r["launches"][0], r["stage2_ms"][0], r["launches"][1], r["finish_ms"][0],
                     r["device_ms"], r["device_over_geodesic"], r["watershed_wall_ms"], r["level_loop_wall_ms"], r["loop_over_watershed"],
                     r["unreached"], r["max_level"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
