"""Time of the elastic stage of data.augment alone - everything after reflect_rotate_crop - for both deformations, in one
process, alternated, after warm-up, at the configs[3] shape (B = 2, S = 700, crop = 512) and at B = 8, S = 572 (crop = 388):
  field   elastic='field' in host-RandomState mode, as augment runs it: two S x S uniform fields per sample drawn on the host
          and uploaded, four 1-D Gaussian passes of radius 40, a bilinear warp per plane, then the ATen glue (floor / clamp,
          crop + threshold, amin / amax, normalisation)
  grid    elastic='grid': 2 G^2 normal draws per sample on the host, one small upload, unet_elastic_grid_sample,
          unet_normalise01
Both stages start from the same rotated batch.  Events are recorded on the stream around the whole stage, so the host's
share (draws, uploads, launch gaps during which the device idles) is inside the figure, as it is inside a training step;
`device` is the same stage with the random input already on the device (fields= / a device disp), i.e. the kernels and their
launch gaps only.  Median (min .. max) of --reps.  The launches per batch are counted with torch.profiler in a pass of their
own after the timing (device kernels and memory copies of one stage).

    timeout -k 10 600 python tools/time_elastic.py [--reps 30] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dl-unet_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import data  # noqa: E402


def field_stage(both, crop, alpha, sigma, levels, random_state=None, fields=None):
    """data.augment's statements after reflect_rotate_crop for elastic='field' (main() checks it against augment itself)"""
    B, S = both.shape[0] // 2, both.shape[-1]
    inp, gt = data.elastic_transform((both[:B], both[B:]), alpha, sigma, random_state=random_state, fields=fields)
    if levels:
        inp = torch.floor(inp + 0.5).clamp_(0, levels)
        gt = torch.floor(gt + 0.5).clamp_(0, levels)
    pad = int((S - crop) / 2)
    gt = (gt[:, pad:crop + pad, pad:crop + pad] > 127).long()
    lo, hi = inp.amin(dim=(1, 2), keepdim=True), inp.amax(dim=(1, 2), keepdim=True)
    return (inp - lo) / (hi - lo), gt


def grid_stage(both, crop, sigma, levels, grid, random_state=None, disp=None):
    B = both.shape[0] // 2
    return data._grid_stage(both, crop, data.grid_displacements(random_state, B, grid, sigma) if disp is None else disp, -0.5, levels)


def timed(calls, reps):
    """calls: name -> stage; alternated rep by rep.  name -> sorted event times in ms"""
    for call in calls.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    ev = {n: [] for n in calls}
    for _ in range(reps):
        for n, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); call(); b.record()
            ev[n].append((a, b))
    torch.cuda.synchronize()
    return {n: sorted(a.elapsed_time(b) for a, b in v) for n, v in ev.items()}


def launches(call):
    """(device kernels, memory copies) of one call"""
    from torch.profiler import ProfilerActivity, profile
    call()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
    copies = [e for e in dev if e.name.lower().startswith(("memcpy", "memset"))]
    return len(dev) - len(copies), len(copies)


def rotated_batch(dev, B, crop, S, levels, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:crop, :crop]
    img = np.floor(rs.rand(B, crop, crop) * 256).astype(np.float32)
    tgt = np.zeros((B, crop, crop), np.float32)
    for b in range(B):
        for _ in range(40):
            cy, cx, r = rs.uniform(0, crop), rs.uniform(0, crop), rs.uniform(8, crop / 12)
            tgt[b][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = 255
    angles = [float(a) for a in rs.choice(np.arange(0, 360, 30), B)]
    both = data.reflect_rotate_crop(torch.from_numpy(np.concatenate([img, tgt])).to(dev), angles + angles, S, levels=levels)
    return torch.from_numpy(img).to(dev), torch.from_numpy(tgt).to(dev), angles, both


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--grid", type=int, default=3)
    ap.add_argument("--no-count", action="store_true", help="skip the torch.profiler pass that counts launches")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_elastic.py measures on a HIP device; there is nothing to report without one"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    alpha, sigma, levels = 3, 10, 255
    res = []
    for B, S, crop in ((2, 700, 512), (8, 572, 388)):
        img, tgt, angles, both = rotated_batch(dev, B, crop, S, levels, 7)
        # the stage restated above is augment's: same draws, same batch
        w = data.augment(img, tgt, [(0, 0)] * B, crop, angles, alpha, sigma, random_state=np.random.RandomState(1), levels=levels)
        f = field_stage(both, crop, alpha, sigma, levels, random_state=np.random.RandomState(1))
        assert torch.equal(w[0][:, 0], f[0]) and torch.equal(w[1][:, 0], f[1])
        w = data.augment(img, tgt, [(0, 0)] * B, crop, angles, alpha, sigma, random_state=np.random.RandomState(1), levels=levels,
                         elastic="grid", grid=a.grid)
        g = grid_stage(both, crop, sigma, levels, a.grid, random_state=np.random.RandomState(1))
        assert torch.equal(w[0][:, 0], g[0]) and torch.equal(w[1][:, 0], g[1])
        rs_f, rs_g = np.random.RandomState(2), np.random.RandomState(3)
        dev_fields = (torch.rand(B, S, S, device=dev), torch.rand(B, S, S, device=dev))
        dev_disp = torch.from_numpy(data.grid_displacements(np.random.RandomState(4), B, a.grid, sigma)).to(dev)
        calls = {
            "field": lambda: field_stage(both, crop, alpha, sigma, levels, random_state=rs_f),
            "grid": lambda: grid_stage(both, crop, sigma, levels, a.grid, random_state=rs_g),
            "field_device": lambda: field_stage(both, crop, alpha, sigma, levels, fields=dev_fields),
            "grid_device": lambda: grid_stage(both, crop, sigma, levels, a.grid, disp=dev_disp),
        }
        ms = timed(calls, a.reps)
        row = {"B": B, "S": S, "crop": crop, "grid": a.grid, "reps": a.reps}
        for n, v in ms.items():
            row[n + "_ms"], row[n + "_min_ms"], row[n + "_max_ms"] = v[len(v) // 2], v[0], v[-1]
        row["ratio_field_over_grid"] = row["field_ms"] / row["grid_ms"]
        row["ratio_device_field_over_grid"] = row["field_device_ms"] / row["grid_device_ms"]
        if not a.no_count:
            for n in ("field", "grid"):
                row[n + "_kernels"], row[n + "_copies"] = launches(calls[n])
        res.append(row)
        print("B=%d S=%d crop=%d" % (B, S, crop))
        for n in calls:
            print("  %-13s %8.3f ms  (%.3f .. %.3f)" % (n, row[n + "_ms"], row[n + "_min_ms"], row[n + "_max_ms"]))
        print("  field / grid: %.1fx with the host's share, %.1fx device only" % (row["ratio_field_over_grid"], row["ratio_device_field_over_grid"]))
        if not a.no_count:
            print("  launches per batch: field %d kernels + %d copies, grid %d kernels + %d copies"
                  % (row["field_kernels"], row["field_copies"], row["grid_kernels"], row["grid_copies"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
