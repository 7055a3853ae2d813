"""Device time of the mask clean-up: unet_clean_mask (defaults; with max_hole_area and min_area set; with the filling off) and
unet_label_components_conn at connectivity 4 and 8, next to unet_label_components at the same shapes in the same run: B = 30,
512 x 512 and B = 8, 388 x 388.  The masks are seeded cell images (tests/instances_ref.cells_case, the prediction's foreground,
as in tools/shape_time.py) with 1 % of the pixels flipped, so that there are holes to fill and speckle to drop.
Events around the library call alone (buffers preallocated, no host sync inside), 3 warm-ups, median, minimum and maximum of --reps.
The structural claim, that the cost does not depend on the number of holes or cells: at 8 x 388 x 388 a speckle mask against a
mask of discs, whose component counts differ more than tenfold, through the same calls.

    timeout -k 10 600 python tools/clean_time.py [--reps 50] [--json out.json]
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
from instances_time import event_median  # noqa: E402

CLEAN = (("clean_default_ms", dict(fill=1, hole=-1, small=0, border=0)),
         ("clean_limits_ms", dict(fill=1, hole=64, small=30, border=1)),
         ("clean_nofill_ms", dict(fill=0, hole=-1, small=30, border=1)))


def cells(B, H, W, n, flip=0.01):
    rs = np.random.RandomState(5)
    m = np.stack([instances_ref.cells_case(100 + b % 6, n, H, W)[1] > 0 for b in range(B)])
    return (m ^ (rs.rand(B, H, W) < flip)).astype(np.uint8)


def speckle(B, H, W, p=0.02):
    return (np.random.RandomState(6).rand(B, H, W) < p).astype(np.uint8)


def discs(B, H, W, n=40):
    rs = np.random.RandomState(7)
    return np.stack([instances_ref.discs(rs, H, W, n) for _ in range(B)]).astype(np.uint8)


def time_mask(dev, name, mask_np, reps):
    L = _hip.lib()
    B, H, W = mask_np.shape
    mask = torch.from_numpy(mask_np).to(dev)
    mask64 = mask.long()
    r = {"name": name, "B": B, "H": H, "W": W}
    labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    nobj = torch.empty(B, dtype=torch.int32, device=dev)
    lscr = torch.empty(L.unet_label_components_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    r["label_ms"] = event_median(lambda: _hip.run("unet_label_components", dev, _hip.ptr(mask64), 0, B, H, W, _hip.ptr(labels), _hip.ptr(nobj),
                                                  _hip.ptr(lscr)), reps)
    r["components"] = int(nobj.sum())
    old = labels.clone()
    cscr = torch.empty(L.unet_label_components_conn_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    for conn in (4, 8):
        r["label_conn%d_ms" % conn] = event_median(lambda: _hip.run("unet_label_components_conn", dev, _hip.ptr(mask64), 0, B, H, W, conn, 1,
                                                                    _hip.ptr(labels), _hip.ptr(nobj), _hip.ptr(cscr)), reps)
        r["components_conn%d" % conn] = int(nobj.sum())
        if conn == 4:
            assert torch.equal(labels, old)
    out = torch.empty_like(mask)
    action = torch.empty_like(mask)
    info = torch.empty(B, 7, dtype=torch.int64, device=dev)
    scr = torch.empty(L.unet_clean_mask_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    for key, kw in CLEAN:
        r[key] = event_median(lambda: _hip.run("unet_clean_mask", dev, _hip.ptr(mask), 3, B, H, W, 4, kw["fill"], kw["hole"], kw["small"], kw["border"],
                                               _hip.ptr(out), _hip.ptr(action), _hip.ptr(info), _hip.ptr(scr)), reps)
        r[key[:-3] + "_info"] = info.sum(dim=0).tolist()
    r["clean_default_conn8_ms"] = event_median(lambda: _hip.run("unet_clean_mask", dev, _hip.ptr(mask), 3, B, H, W, 8, 1, -1, 0, 0, _hip.ptr(out),
                                                                _hip.ptr(action), _hip.ptr(info), _hip.ptr(scr)), reps)
    assert torch.equal(functions.clean_mask(mask, connectivity=8), out)
    for k in [k for k in r if k.endswith("_ms") and k != "label_ms"]:
        r[k[:-3] + "_over_label"] = r[k][0] / r["label_ms"][0]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = []
    for name, m in (("cells 30x512x512", cells(30, 512, 512, 170)), ("cells 8x388x388", cells(8, 388, 388, 99)),
                    ("speckle 8x388x388", speckle(8, 388, 388)), ("discs 8x388x388", discs(8, 388, 388))):
        r = time_mask(dev, name, m, a.reps)
        res.append(r)
        print("%-18s %6d components (%d at 8) | label %.3f ms | label_conn 4: %.3f, 8: %.3f ms | clean default %.3f (conn 8: %.3f), "
              "limits %.3f, no fill %.3f ms | default info %s"
              % (name, r["components"], r["components_conn8"], r["label_ms"][0], r["label_conn4_ms"][0], r["label_conn8_ms"][0],
                 r["clean_default_ms"][0], r["clean_default_conn8_ms"][0], r["clean_limits_ms"][0], r["clean_nofill_ms"][0], r["clean_default_info"]),
              flush=True)
        print("   ratios to unet_label_components: " + ", ".join("%s %.2f" % (k[:-11], v) for k, v in r.items() if k.endswith("_over_label")), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
