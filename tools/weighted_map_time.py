"""Device time of the border weight map (unet_weighted_map) after warm-up, on three label batches:
  cells   B = 2, 512^2 oracle.aux_ref.cells masks (BASELINE configs[3]'s label), int64
  speckle B = 1, 512^2, each pixel a cell with p = 0.35 (tens of thousands of components), int64
  big     B = 16, 1028^2 cells masks (configs[4]'s output size), int64
Events bracket the library call alone (buffers preallocated, no host sync inside); median of --reps.

    timeout -k 10 300 python tools/weighted_map_time.py [--reps 50] [--json out.json]
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
import _hip  # noqa: E402
from oracle import aux_ref  # noqa: E402


def time_op(lab, reps, w0=20.0, sig2=25.0):
    L = _hip.lib()
    B, H, W = lab.shape
    dev = lab.device
    w = torch.empty(B, H, W, device=dev)
    counts = torch.empty(B, dtype=torch.int64, device=dev)
    nobj = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(L.unet_weighted_map_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)

    def call():
        _hip.run("unet_weighted_map", dev, _hip.ptr(lab), 0, B, H, W, w0, sig2, _hip.ptr(w), _hip.ptr(counts),
                 _hip.ptr(nobj), _hip.ptr(scratch))

    for _ in range(5):
        call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); call(); b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"B": B, "H": H, "W": W, "median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1],
            "components": nobj.cpu().tolist()[:4], "count1": counts.cpu().tolist()[:4]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cells = torch.from_numpy(np.stack([aux_ref.cells(s, 512)[1] // 255 for s in (1, 2)]).astype(np.int64)).to(dev)
    speckle = torch.from_numpy((np.random.RandomState(0).rand(1, 512, 512) < 0.35).astype(np.int64)).to(dev)
    big = torch.from_numpy(np.stack([aux_ref.cells(s, 1028)[1] // 255 for s in range(16)]).astype(np.int64)).to(dev)
    res = {}
    for name, lab in (("cells_B2_512", cells), ("speckle_B1_512", speckle), ("cells_B16_1028", big)):
        res[name] = r = time_op(lab, a.reps)
        print("%-15s B=%-2d %4dx%-4d  median %.4f ms  (min %.4f, max %.4f)  components %s" %
              (name, r["B"], r["H"], r["W"], r["median_ms"], r["min_ms"], r["max_ms"], r["components"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
