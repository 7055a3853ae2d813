"""Device time of unet_link_frames (functions.link_frames) after warm-up, wall time of functions.track_cells, and wall time of
the only way there was before: functions.pair_table of consecutive frames, read back, and an arg-max per cell on the host.
T = 30, 512 x 512 (170 cells) and T = 8, 388 x 388 (99 cells): seeded cell images (tests/instances_ref.cells_case) sliding two
pixels per frame along both axes, the ids dealt anew in every frame (tests/track_ref.shifted_cells).  Events around the library
call alone (buffers preallocated, no host sync inside), median, minimum and maximum of --reps; the wall times are whole Python
calls, read-backs included, median of --reps / 5.  The host way's links are compared with the device's: they must be equal.

    timeout -k 10 600 python tools/link_time.py [--reps 50] [--json out.json]
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
import track_ref  # noqa: E402
from instances_time import event_median, wall_median  # noqa: E402


def host_links(labels, n_max):
    """pred, pred_overlap [T][n_max+1] the parent commit's way: the pair table of (frame t, frame t-1), sorted on the host."""
    T = labels.shape[0]
    pred, over = np.zeros((T, n_max + 1), np.int64), np.zeros((T, n_max + 1), np.int64)
    if T > 1:
        b, g, p, n = functions.pair_table(labels[1:], labels[:-1])       # g: ids of frame t-1, p: ids of frame t (0 = background)
        on = p > 0
        b, g, p, n = b[on], g[on], p[on], n[on]
        order = np.lexsort((g, -n, p, b))                                # per (b, p): the largest n first, the smaller g among equals
        b, g, p, n = b[order], g[order], p[order], n[order]
        first = np.ones(len(b), bool)
        first[1:] = (b[1:] != b[:-1]) | (p[1:] != p[:-1])
        pred[b[first] + 1, p[first]], over[b[first] + 1, p[first]] = g[first], n[first]
    return pred, over


def time_case(dev, T, H, W, cells, reps):
    L = _hip.lib()
    labels = torch.from_numpy(track_ref.shifted_cells(100, T, H, W, cells)).to(dev)
    n_max = int(labels.max())
    slots = 1 << (min(4 * (T - 1) * n_max, T * H * W) + 1024 - 1).bit_length()
    out = torch.empty(3, T, n_max + 1, dtype=torch.int32, device=dev)
    status = torch.empty(T, 2, dtype=torch.int64, device=dev)
    scratch = torch.empty(L.unet_link_frames_scratch_bytes(T, n_max, slots), dtype=torch.uint8, device=dev)
    r = {"T": T, "H": H, "W": W, "cells": cells, "n_max": n_max, "slots": slots}
    r["link_ms"] = event_median(lambda: _hip.run("unet_link_frames", dev, _hip.ptr(labels), _hip.ptr(labels), T, H, W, n_max, slots,
                                                 _hip.ptr(out[0]), _hip.ptr(out[1]), _hip.ptr(out[2]), _hip.ptr(status), _hip.ptr(scratch)), reps)
    assert int(status.sum()) == 0
    walls = max(3, reps // 5)
    r["link_frames_wall_ms"] = wall_median(lambda: functions.link_frames(labels), walls)
    r["link_frames_reach2_wall_ms"] = wall_median(lambda: functions.link_frames(labels, reach=2), walls)
    r["track_cells_wall_ms"] = wall_median(lambda: functions.track_cells(labels), walls)
    links = functions.link_frames(labels)
    r["tracks_from_links_host_ms"] = wall_median(lambda: functions.tracks_from_links(links), walls)
    r["host_way_wall_ms"] = wall_median(lambda: host_links(labels, n_max), walls)
    pred, over = host_links(labels, n_max)
    assert np.array_equal(pred, links.pred) and np.array_equal(over, links.pred_overlap)
    tracks = functions.track_cells(labels)[1]
    r["tracks"], r["divisions"] = len(tracks.table), int((tracks.table[:, 3] > 0).sum())
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
    for T, H, W, cells in ((30, 512, 512, 170), (8, 388, 388, 99)):
        r = time_case(dev, T, H, W, cells, a.reps)
        res.append(r)
        print("T %d, %d x %d (%.0f%% labelled, ids to %d, %d slots): unet_link_frames %.3f ms [%.3f .. %.3f] | link_frames %.2f ms wall, "
              "reach=2 %.2f ms | track_cells %.2f ms wall (tracks_from_links %.2f ms of it, %d tracks, %d daughters) | "
              "pair_table + host arg-max %.2f ms wall"
              % (T, H, W, 100 * r["labelled_fraction"], r["n_max"], r["slots"], *r["link_ms"], r["link_frames_wall_ms"],
                 r["link_frames_reach2_wall_ms"], r["track_cells_wall_ms"], r["tracks_from_links_host_ms"], r["tracks"], r["divisions"],
                 r["host_way_wall_ms"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
