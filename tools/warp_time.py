"""Device time of the sweeps behind functions.warp_labels / functions.warping_error (unet_warp_sweeps) at 4, 8 and 16 passes per
launch, next to unet_label_components at the same shapes in the same run: B = 30, 512 x 512 (the ISBI 2012 stack) and B = 8,
388 x 388.  The masks are seeded cell images against their predictions (tests/instances_ref.cells_case, foreground = id > 0).
For every P, one call of unet_warp_sweeps that enqueues the launches the warp needs to converge from the initial state (the
number of sweeps is taken from functions.warp_labels first; the final empty sweep included), the state restored in front of every
repetition outside the timed region; and two launches on the converged state, which every workgroup leaves after staging and
copying its tile.
Events around the library call alone (buffers preallocated, no host sync inside), 3 warm-ups, median, minimum and maximum of --reps.
functions.warping_error as wall time of the whole Python call (read-backs and the labelling of the mismatch included).

    timeout -k 10 600 python tools/warp_time.py [--reps 50] [--json out.json]
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


def event_median_after(prepare, call, reps):
    """event_median with prepare() in front of every call, outside the events."""
    for _ in range(3):
        prepare(); call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        prepare(); a.record(); call(); b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0], ms[-1]


def time_case(dev, B, H, W, cells, reps, reach):
    L = _hip.lib()
    pairs = [instances_ref.cells_case(100 + b % 6, cells, H, W) for b in range(B)]
    gt = torch.from_numpy(np.stack([g > 0 for g, _ in pairs]).astype(np.uint8)).to(dev)
    pred = torch.from_numpy(np.stack([p > 0 for _, p in pairs]).astype(np.uint8)).to(dev)
    r = {"B": B, "H": H, "W": W, "cells": cells, "reach": reach}
    labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    nobj = torch.empty(B, dtype=torch.int32, device=dev)
    lscr = torch.empty(L.unet_label_components_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    mask64 = gt.long()
    r["label_ms"] = event_median(lambda: _hip.run("unet_label_components", dev, _hip.ptr(mask64), 0, B, H, W, _hip.ptr(labels), _hip.ptr(nobj),
                                                  _hip.ptr(lscr)), reps)
    warped, c = functions.warp_labels(gt, pred, reach=reach)
    r["sweeps"], r["flips"], r["mismatch_before"], r["mismatch"] = c.sweeps, int(c.flips.sum()), int(c.mismatch_before.sum()), int(c.mismatch.sum())
    state0 = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    state = torch.empty_like(state0)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(L.unet_warp_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    init = lambda: _hip.run("unet_warp_init", dev, _hip.ptr(gt), 3, _hip.ptr(pred), 3, None, 0, B, H, W,
                            -1 if reach is None else int(reach * reach), 4, _hip.ptr(state0), _hip.ptr(counts), _hip.ptr(scratch))
    r["init_ms"] = event_median(init, reps)
    for P in (4, 8, 16):
        n = -(-4 * c.sweeps // P)                             # launches that hold every sweep, the empty one included
        slots = torch.empty(n, 4, B, dtype=torch.int32, device=dev)
        sweeps = lambda k=n: _hip.run("unet_warp_sweeps", dev, _hip.ptr(state), B, H, W, P, k, _hip.ptr(slots), 0, _hip.ptr(scratch))
        r["converge_p%d_ms" % P] = event_median_after(lambda: state.copy_(state0), sweeps, reps)
        r["launches_p%d" % P] = n
        assert int(slots.sum()) == r["flips"] and not bool(slots[-1, P // 4 - 1].any())
        r["idle_launch_p%d_ms" % P] = event_median(lambda: sweeps(2), reps)          # the state is converged now: two no-op launches
        assert not bool(slots[0].any())
    r["warping_error_wall_ms"] = wall_median(lambda: functions.warping_error(pred, gt, reach=reach), max(3, reps // 5))
    r["warping_error_mean"] = float(functions.warping_error(pred, gt, reach=reach).warping_error_mean)
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
        for reach in (None, 5):
            r = time_case(dev, B, H, W, cells, a.reps, reach)
            res.append(r)
            print("B %d, %d x %d, reach %s: %d sweeps, %d flips, mismatch %d -> %d | label %.3f ms | init %.3f ms | to convergence: "
                  "P=4 %.3f ms (%d launches)  P=8 %.3f ms (%d)  P=16 %.3f ms (%d) | two idle launches: %.4f / %.4f / %.4f ms | "
                  "warping_error %.2f ms wall, mean %.5f"
                  % (B, H, W, reach, r["sweeps"], r["flips"], r["mismatch_before"], r["mismatch"], r["label_ms"][0], r["init_ms"][0],
                     r["converge_p4_ms"][0], r["launches_p4"], r["converge_p8_ms"][0], r["launches_p8"], r["converge_p16_ms"][0],
                     r["launches_p16"], r["idle_launch_p4_ms"][0], r["idle_launch_p8_ms"][0], r["idle_launch_p16_ms"][0],
                     r["warping_error_wall_ms"], r["warping_error_mean"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
