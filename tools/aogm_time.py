"""Device time of unet_aogm_counts (the graph stage of ctc.aogm_counts) after warm-up, alone and behind unet_instance_overlap on
the same stream, next to unet_instance_overlap alone: that call is what functions.seg_measure spends on the same maps, so the
difference is what DET and TRA add on top of SEG.  Then the wall time of ctc.tra_measure, read-backs included.
T = 30, 512 x 512 (170 cells) and T = 8, 388 x 388 (99 cells): the time-lapses of tools/link_time.py, tracked by
functions.track_cells as the reference; the result is the same time-lapse moved one pixel to the right and tracked again.
Events around the library calls alone (buffers preallocated, no host sync inside), median, minimum and maximum of --reps; the wall
time is the whole Python call, median of --reps / 5.

    timeout -k 10 600 python tools/aogm_time.py [--reps 50] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dl-unet_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import _hip  # noqa: E402
import ctc  # noqa: E402
import functions  # noqa: E402
import track_ref  # noqa: E402
from instances_time import event_median, wall_median  # noqa: E402

LAUNCHES = {"unet_instance_overlap": "7 memsets, 2 launches", "unet_aogm_counts": "3 launches"}


def time_case(dev, T, H, W, cells, reps):
    labels = torch.from_numpy(track_ref.shifted_cells(100, T, H, W, cells)).to(dev)
    gt, gt_tracks = functions.track_cells(labels)
    res, res_tracks = functions.track_cells(torch.roll(labels, 1, dims=2))
    ng, nr = int(gt.max()), int(res.max())
    slots = 1 << (4 * (ng + nr) + 1024 - 1).bit_length()

    def words(*shape, dtype=torch.int32):
        return torch.empty(*shape, dtype=dtype, device=dev)

    area_gt, area_res, match, inter = words(T, ng + 1), words(T, nr + 1), words(T, ng + 1), words(T, ng + 1)
    status = words(T, 2, dtype=torch.int64)
    ov_scratch = _hip.scratch("unet_instance_overlap", dev, T, ng, nr, slots)
    rows_gt = ctc._device_rows(ctc.tracks_table(gt_tracks), ng, dev)
    rows_res = ctc._device_rows(ctc.tracks_table(res_tracks), nr, dev)
    outs = [words(T, nr + 1), words(T, nr + 1), words(T, ng + 1, 2), words(T, nr + 1, 2), words(T, ng + 1, dtype=torch.uint8),
            words(T, nr + 1, dtype=torch.uint8), words(T, 12, dtype=torch.int64)]
    scratch = _hip.scratch("unet_aogm_counts", dev, T, ng, nr)

    def overlap():
        _hip.run("unet_instance_overlap", dev, _hip.ptr(gt), _hip.ptr(res), T, H, W, ng, nr, slots, _hip.ptr(area_gt), _hip.ptr(area_res),
                 _hip.ptr(match), _hip.ptr(inter), _hip.ptr(status), _hip.ptr(ov_scratch))

    def graph():
        _hip.run("unet_aogm_counts", dev, _hip.ptr(area_gt), _hip.ptr(area_res), _hip.ptr(match), _hip.ptr(rows_gt), _hip.ptr(rows_res), T, ng, nr,
                 *(_hip.ptr(o) for o in outs), _hip.ptr(scratch))

    def both():
        overlap()
        graph()

    r = {"T": T, "H": H, "W": W, "cells": cells, "ng_max": ng, "nr_max": nr, "slots": slots, "launches": LAUNCHES}
    r["overlap_ms"] = event_median(overlap, reps)
    assert int(status.sum()) == 0
    r["aogm_ms"] = event_median(graph, reps)
    r["overlap_and_aogm_ms"] = event_median(both, reps)
    r["added_fraction"] = r["overlap_and_aogm_ms"][0] / r["overlap_ms"][0] - 1
    walls = max(3, reps // 5)
    r["tra_measure_wall_ms"] = wall_median(lambda: ctc.tra_measure(res, res_tracks, gt, gt_tracks), walls)
    r["seg_measure_wall_ms"] = wall_median(lambda: functions.seg_measure(res, gt), walls)
    got = ctc.tra_measure(res, res_tracks, gt, gt_tracks)
    assert outs[6].cpu().numpy().sum(axis=0).tolist() == list(got.counts.total())
    r["counts"] = dict(zip(ctc.COUNT_NAMES, got.counts.total()))
    r["tra"], r["det"] = float(got.scores.tra), float(got.scores.det)
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
        print("T %d, %d x %d (%d / %d tracks, %d slots): unet_instance_overlap %.3f ms [%.3f .. %.3f] | unet_aogm_counts %.3f ms "
              "[%.3f .. %.3f] | both %.3f ms [%.3f .. %.3f] = overlap + %.1f%% | tra_measure %.2f ms wall, seg_measure %.2f ms wall | "
              "TRA %.4f DET %.4f"
              % (T, H, W, r["ng_max"], r["nr_max"], r["slots"], *r["overlap_ms"], *r["aogm_ms"], *r["overlap_and_aogm_ms"],
                 100 * r["added_fraction"], r["tra_measure_wall_ms"], r["seg_measure_wall_ms"], r["tra"], r["det"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
