"""Time of the grid stage of data.augment - everything after reflect_rotate_crop with elastic='grid' - without and with the
grey-value variation, in one process, alternated, after warm-up, at the configs[3] shape (B = 2, S = 700, crop = 512) and at
B = 8, S = 572 (crop = 388):
  plain   unet_elastic_grid_sample, unet_normalise01                            (2 G^2 normal draws per sample on the host)
  grey    unet_elastic_grid_sample, unet_grey_vary with the min / max table    (+ 5 uniform draws per sample on the host):
          contrast, brightness, gamma and noise all active for every sample, i.e. both of its launches and every stage
Both start from the same rotated batch.  Events are recorded on the stream around the whole stage, so the host's share (draws,
the upload of the nodes, launch gaps) is inside the figure, as it is inside a training step; `*_device` is the same stage with
the nodes already on the device and the parameters given.  `normalise01` and `grey_vary` are the last call of each stage alone,
on the sampled image (restored before each call, outside the events), `grey_vary_no_mean` the same with contrast and brightness
the identity, i.e. without the sum pass.  Median (min .. max) of --reps.  The launches per batch
are counted with torch.profiler in a pass of their own after the timing.

    timeout -k 10 600 python tools/grey_time.py [--reps 30] [--json profiles/grey_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dl-unet_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import _hip  # noqa: E402
import data  # noqa: E402
from time_elastic import launches, rotated_batch, timed  # noqa: E402

RANGES = dict(gamma=(0.7, 1.5), contrast=(0.75, 1.25), brightness=(-0.1, 0.1), noise=(0.01, 0.05))


def stage(both, crop, sigma, levels, grid, random_state=None, disp=None, grey=None, step=0):
    """data.augment's statements after reflect_rotate_crop for elastic='grid' (main() checks it against augment itself)"""
    B = both.shape[0] // 2
    disp = data.grid_displacements(random_state, B, grid, sigma) if disp is None else disp
    if grey is not None:
        grey = (data.grey_parameters(random_state, B, **grey) if isinstance(grey, dict) else grey, 0, step)
    return data._grid_stage(both, crop, disp, -0.5, levels, grey)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--grid", type=int, default=3)
    ap.add_argument("--no-count", action="store_true", help="skip the torch.profiler pass that counts launches")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "grey_time.py measures on a HIP device; there is nothing to report without one"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    sigma, levels = 10, 255
    res = []
    for B, S, crop in ((2, 700, 512), (8, 572, 388)):
        img, tgt, angles, both = rotated_batch(dev, B, crop, S, levels, 7)
        # the stage restated above is augment's: same draws, same batch
        w = data.augment(img, tgt, [(0, 0)] * B, crop, angles, 3, sigma, random_state=np.random.RandomState(1), levels=levels, elastic="grid",
                         grid=a.grid, grey=RANGES, grey_step=5)
        g = stage(both, crop, sigma, levels, a.grid, random_state=np.random.RandomState(1), grey=RANGES, step=5)
        assert torch.equal(w[0][:, 0], g[0]) and torch.equal(w[1][:, 0], g[1])
        rs_p, rs_g = np.random.RandomState(2), np.random.RandomState(3)
        dev_disp = torch.from_numpy(data.grid_displacements(np.random.RandomState(4), B, a.grid, sigma)).to(dev)
        rows = data.grey_parameters(np.random.RandomState(5), B, **RANGES)
        # the last call of each stage alone, on the image unet_elastic_grid_sample leaves
        d = data._grid_tensor(dev_disp, B, dev, "grey_time")
        raw = torch.empty(B, S, S, device=dev)
        gt = torch.empty(B, crop, crop, dtype=torch.int64, device=dev)
        mm = torch.empty(B, 2, device=dev)
        _hip.run("unet_elastic_grid_sample", dev, _hip.ptr(both[:B]), _hip.ptr(both[B:]), B, S, _hip.ptr(d), a.grid, -0.5, levels,
                 int((S - crop) / 2), crop, _hip.ptr(raw), _hip.ptr(gt), _hip.ptr(mm))
        work = raw.clone()
        calls = {
            "plain": lambda: stage(both, crop, sigma, levels, a.grid, random_state=rs_p),
            "grey": lambda: stage(both, crop, sigma, levels, a.grid, random_state=rs_g, grey=RANGES),
            "plain_device": lambda: stage(both, crop, sigma, levels, a.grid, disp=dev_disp),
            "grey_device": lambda: stage(both, crop, sigma, levels, a.grid, disp=dev_disp, grey=rows),
        }
        ms = timed(calls, a.reps)
        # the two last calls alone: the copy that restores the image runs after the closing event of one repetition and before
        # the opening event of the next, so it is outside every figure
        flat = work.reshape(B, -1)
        no_mean = rows.copy()
        no_mean[:, 1:3] = (1.0, 0.0)                    # contrast and brightness the identity: no sum pass, one launch
        alone = {
            "normalise01": lambda: _hip.run("unet_normalise01", dev, _hip.ptr(work), B, S * S, _hip.ptr(mm)),
            "grey_vary": lambda: data._grey_run(flat, flat, rows, 0, 0, 0, True, mm),
            "grey_vary_no_mean": lambda: data._grey_run(flat, flat, no_mean, 0, 0, 0, True, mm),
        }
        ev = {n: [] for n in alone}
        for n, call in alone.items():
            for _ in range(3):
                call(); work.copy_(raw)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for n, call in alone.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record(); call(); e.record()
                work.copy_(raw)
                ev[n].append((s, e))
        torch.cuda.synchronize()
        ms.update({n: sorted(s.elapsed_time(e) for s, e in v) for n, v in ev.items()})
        row = {"B": B, "S": S, "crop": crop, "grid": a.grid, "reps": a.reps}
        for n, v in ms.items():
            row[n + "_ms"], row[n + "_min_ms"], row[n + "_max_ms"] = v[len(v) // 2], v[0], v[-1]
        row["ratio_grey_over_plain"] = row["grey_ms"] / row["plain_ms"]
        row["ratio_device_grey_over_plain"] = row["grey_device_ms"] / row["plain_device_ms"]
        row["ratio_grey_vary_over_normalise01"] = row["grey_vary_ms"] / row["normalise01_ms"]
        if not a.no_count:
            for n in ("plain_device", "grey_device"):
                row[n + "_kernels"], row[n + "_copies"] = launches(calls[n])
        res.append(row)
        print("B=%d S=%d crop=%d" % (B, S, crop))
        for n in ms:
            print("  %-13s %8.3f ms  (%.3f .. %.3f)" % (n, row[n + "_ms"], row[n + "_min_ms"], row[n + "_max_ms"]))
        print("  grey / plain: %.2fx with the host's share, %.2fx device only; unet_grey_vary / unet_normalise01 alone: %.2fx"
              % (row["ratio_grey_over_plain"], row["ratio_device_grey_over_plain"], row["ratio_grey_vary_over_normalise01"]))
        if not a.no_count:
            print("  launches per batch: plain %d kernels + %d copies, grey %d kernels + %d copies"
                  % (row["plain_device_kernels"], row["plain_device_copies"], row["grey_device_kernels"], row["grey_device_copies"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
