"""Device time of functions.grow_cells (unet_grow_labels, unlimited and max_distance = 4) and of the pair table behind
functions.rand_scores (unet_partition_pairs) after warm-up, next to unet_label_components at the same shapes in the same run:
B = 30, 512 x 512 (the ISBI 2012 stack) and B = 8, 388 x 388.  The id maps are what the ops see in use: seeded cell images
(tests/instances_ref.cells_case), carved and labelled on the device (data.binary_target, functions.label_cells), grown, and
counted against the uncarved ids.  Events around the library call alone (buffers preallocated, no host sync inside), median,
minimum and maximum of --reps; pair_table and rand_scores also as wall time of the whole Python call (read-backs included).

    timeout -k 10 600 python tools/rand_time.py [--reps 50] [--json out.json]
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
import data  # noqa: E402
import functions  # noqa: E402
import instances_ref  # noqa: E402
from instances_time import event_median, wall_median  # noqa: E402


def time_case(dev, B, H, W, cells, reps):
    L = _hip.lib()
    gt = torch.from_numpy(np.stack([instances_ref.cells_case(100 + b % 6, cells, H, W)[0] for b in range(B)])).to(dev)
    mask = (data.binary_target(gt) > 0).long()
    labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    nobj = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(L.unet_label_components_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    r = {"B": B, "H": H, "W": W, "cells": cells}
    r["label_ms"] = event_median(lambda: _hip.run("unet_label_components", dev, _hip.ptr(mask), 0, B, H, W, _hip.ptr(labels), _hip.ptr(nobj),
                                                  _hip.ptr(scratch)), reps)
    grown = torch.empty_like(labels)
    gscr = torch.empty(L.unet_grow_labels_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    for name, d2 in (("grow4_ms", 16), ("grow_ms", -1)):
        r[name] = event_median(lambda: _hip.run("unet_grow_labels", dev, _hip.ptr(labels), B, H, W, d2, _hip.ptr(grown), _hip.ptr(gscr)), reps)
    ng, npred = int(gt.max()), int(grown.max())
    slots = 1 << (4 * (ng + npred) + 1024 - 1).bit_length()
    keys = torch.empty(slots, dtype=torch.int64, device=dev)
    counts = torch.empty(slots, dtype=torch.int32, device=dev)
    n_pairs = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(B, 2, dtype=torch.int64, device=dev)
    pscr = torch.empty(L.unet_partition_pairs_scratch_bytes(B, slots), dtype=torch.uint8, device=dev)
    r["pairs_ms"] = event_median(lambda: _hip.run("unet_partition_pairs", dev, _hip.ptr(gt), _hip.ptr(grown), B, H, W, ng, npred, slots,
                                                  _hip.ptr(keys), _hip.ptr(counts), _hip.ptr(n_pairs), _hip.ptr(status), _hip.ptr(pscr)), reps)
    assert int(status.sum()) == 0
    r["n_pairs"], r["slots"] = int(n_pairs.item()), slots
    r["pair_table_wall_ms"] = wall_median(lambda: functions.pair_table(grown, gt), max(3, reps // 5))
    r["rand_scores_wall_ms"] = wall_median(lambda: functions.rand_scores(grown, gt), max(3, reps // 5))
    s = functions.rand_scores(labels, gt, grow=True)
    r["rand_error_mean"], r["rand_error_mean_ungrown"] = float(s.rand_error_mean), float(functions.rand_scores(labels, gt).rand_error_mean)
    r["labelled_fraction"] = float((labels > 0).float().mean())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = []
    for B, H, W, cells in ((30, 512, 512, 170), (8, 388, 388, 99)):
        r = time_case(dev, B, H, W, cells, a.reps)
        res.append(r)
        print("B %d, %d x %d (%.0f%% labelled): label %.3f ms | grow(4) %.3f ms  grow(unlimited) %.3f ms [%.3f .. %.3f] | pairs %.3f ms "
              "(%d pairs, %d slots) | pair_table %.2f ms wall, rand_scores %.2f ms wall | Rand error %.4f -> %.4f grown"
              % (B, H, W, 100 * r["labelled_fraction"], r["label_ms"][0], r["grow4_ms"][0], *r["grow_ms"], r["pairs_ms"][0], r["n_pairs"],
                 r["slots"], r["pair_table_wall_ms"], r["rand_scores_wall_ms"], r["rand_error_mean_ungrown"], r["rand_error_mean"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
