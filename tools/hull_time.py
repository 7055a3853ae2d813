"""Device time of the per-cell convex hulls and of the contact list: unet_cell_hulls (boxes and level offsets prepared before, as
functions.cell_hulls prepares them) and unet_cell_contacts, next to unet_cell_sums on the same input in the same run, and next to
the host route a user takes today: labels.cpu() plus a loop over the cells with scipy.spatial.ConvexHull on each cell's corner
points (wall clock).  Inputs: 30 x 512 x 512 with about 170 cells per frame and 8 x 388 x 388 (seeded discs painted in turn, so
that cells touch and overlap into concave shapes).  Events around the library call alone (buffers preallocated, no host sync
inside), 3 warm-ups, median, minimum and maximum of --reps; the wall time of the whole functions.cell_hulls / cell_neighbours calls
beside them.

    timeout -k 10 600 python tools/hull_time.py [--reps 30] [--host-reps 1] [--json profiles/hull_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402
from scipy.spatial import ConvexHull  # noqa: E402
import _hip  # noqa: E402
import functions  # noqa: E402
from instances_time import event_median  # noqa: E402
from measure_time import cells  # noqa: E402


def host_route(lab):
    """What a user does on the host today: per image find_objects, per cell the corner points and scipy's hull; returns the summed
    doubled areas, for the check against the device."""
    total = 0.0
    for m in lab:
        for i, sl in enumerate(ndimage.find_objects(m), 1):
            if sl is None:
                continue
            ys, xs = np.nonzero(m[sl] == i)
            pts = np.concatenate([np.stack([xs + dx, ys + dy], axis=1) for dy in (0, 1) for dx in (0, 1)])
            total += 2 * ConvexHull(pts).volume
    return total


def wall(call, reps):
    ts = []
    for _ in range(max(1, reps)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts)


def time_case(dev, name, lab_np, reps, host_reps):
    L = _hip.lib()
    B, H, W = lab_np.shape
    n_max = int(lab_np.max())
    N = n_max + 1
    lab = torch.from_numpy(lab_np).to(dev)
    r = {"name": name, "B": B, "H": H, "W": W, "ids": n_max, "cells": int(sum(len(np.unique(m)) - 1 for m in lab_np)),
         "foreground": float((lab_np != 0).mean())}
    area = torch.empty(B, N, dtype=torch.int64, device=dev)
    bbox = torch.empty(B, N, 4, dtype=torch.int32, device=dev)
    moments = torch.empty(B, N, 5, dtype=torch.int64, device=dev)
    edges = torch.empty(B, N, 3, dtype=torch.int64, device=dev)
    present = torch.empty(B, N, dtype=torch.bool, device=dev)
    status = torch.empty(B, 2, dtype=torch.int64, device=dev)
    scr = torch.empty(L.unet_cell_sums_scratch_bytes(B, n_max), dtype=torch.uint8, device=dev)
    r["sums_ms"] = event_median(lambda: _hip.run("unet_cell_sums", dev, _hip.ptr(lab), 2, None, 0, B, H, W, n_max, _hip.ptr(area), _hip.ptr(bbox),
                                                 _hip.ptr(moments), _hip.ptr(edges), None, None, _hip.ptr(present), _hip.ptr(status), _hip.ptr(scr)),
                                reps)

    levels = torch.where(present, (bbox[..., 2] - bbox[..., 0] + 1).long(), torch.zeros((), dtype=torch.int64, device=dev))
    levels[:, 0] = 0
    offset = torch.zeros(B * N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(levels.flatten(), dim=0, out=offset[1:])
    nl = int(offset[-1])
    r["levels"] = nl
    nv = torch.empty(B, N, dtype=torch.int32, device=dev)
    a2, f2 = torch.empty(B, N, dtype=torch.int64, device=dev), torch.empty(B, N, dtype=torch.int64, device=dev)
    wd = torch.empty(B, N, 2, dtype=torch.int64, device=dev)
    vt = torch.empty(2 * nl, 2, dtype=torch.int32, device=dev)
    hscr = torch.empty(L.unet_cell_hulls_scratch_bytes(nl), dtype=torch.uint8, device=dev)
    r["hulls_ms"] = event_median(lambda: _hip.run("unet_cell_hulls", dev, _hip.ptr(lab), 2, B, H, W, n_max, _hip.ptr(bbox), _hip.ptr(offset), nl,
                                                  _hip.ptr(nv), _hip.ptr(a2), _hip.ptr(f2), _hip.ptr(wd), _hip.ptr(vt), _hip.ptr(status),
                                                  _hip.ptr(hscr)), reps)
    assert int(status.sum()) == 0
    r["max_vertices"] = int(nv.max())

    slots = 1 << (8 * n_max + 1024 - 1).bit_length()
    keys, counts = torch.empty(slots, dtype=torch.int64, device=dev), torch.empty(slots, dtype=torch.int32, device=dev)
    n_pairs = torch.empty(1, dtype=torch.int64, device=dev)
    cscr = torch.empty(L.unet_cell_contacts_scratch_bytes(B, slots), dtype=torch.uint8, device=dev)
    r["contacts_ms"] = event_median(lambda: _hip.run("unet_cell_contacts", dev, _hip.ptr(lab), 2, B, H, W, n_max, slots, _hip.ptr(keys),
                                                     _hip.ptr(counts), _hip.ptr(n_pairs), _hip.ptr(status), _hip.ptr(cscr)), reps)
    assert int(status.sum()) == 0
    r["pairs"], r["table_slots"] = int(n_pairs), slots
    assert 2 * int(counts[:r["pairs"]].sum()) == int(edges[:, 1:, 2].sum())               # every side once here, once per cell there

    r["cell_hulls_wall_ms"] = wall(lambda: functions.hull_props(functions.cell_hulls(lab, n_max=n_max), functions.CellSums(
        area, bbox, moments, edges[..., 0], edges[..., 1], edges[..., 2], None, None, None, None, present)), 3)
    r["cell_neighbours_wall_ms"] = wall(lambda: functions.cell_neighbours(lab), 3)
    got = []
    r["host_scipy_wall_ms"] = wall(lambda: got.append(host_route(lab.cpu().numpy())), host_reps) if host_reps > 0 else None
    if got:
        assert abs(got[0] - int(a2.sum())) <= 1e-9 * int(a2.sum()), (got[0], int(a2.sum()))
    for k in ("hulls_ms", "contacts_ms"):
        r[k[:-3] + "_over_sums"] = r[k][0] / r["sums_ms"][0]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = []
    for B, S, n in ((30, 512, 170), (8, 388, 100)):
        r = time_case(dev, "%dx%dx%d" % (B, S, S), cells(S + n, B, S, S, n), a.reps, a.host_reps)
        res.append(r)
        print("%-11s %d cells in all, fg %.2f, %d levels, %d pairs | cell_sums %.3f ms | cell_hulls %.3f ms (max %d vertices) | "
              "cell_contacts %.3f ms | cell_hulls + hull_props wall %.1f ms, cell_neighbours wall %.1f ms | host scipy ConvexHull loop wall %s ms"
              % (r["name"], r["cells"], r["foreground"], r["levels"], r["pairs"], r["sums_ms"][0], r["hulls_ms"][0], r["max_vertices"],
                 r["contacts_ms"][0], r["cell_hulls_wall_ms"], r["cell_neighbours_wall_ms"],
                 "%.1f" % r["host_scipy_wall_ms"] if r["host_scipy_wall_ms"] is not None else "-"), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
