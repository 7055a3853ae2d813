"""Cost of a K-class head (Unet(n_classes=K)) on one MI355X, in one process, the shapes alternated:

  step     the fp32 (math 3) and bf16 (math 2) training step at B = 8, 572^2 for K in {2, 3, 4, 8}: forward, centre crop,
           loss, backward, SGD; K = 2 once with the reference's BCE (optim.bce_argmax_step, unweighted: a [B,H,W] map
           meets the class axis at B = 8, quirk Q4) and every K with optim.softmax_ce_step (validate=False, unweighted).
           Median of --reps.
  kernels  head forward / backward (unet_head1xk_*; K = 2 runs head1x1), the softmax CE step and the K-class stitch at
           B = 8, 388^2, C = 64, and the HBM fraction of the algorithmic bytes against 8 TB/s:
             head fwd  npix (es C + 4 K)        head bwd  npix (2 es C + 4 K)        (es = 4 fp32, 2 bf16)
             CE step   npix (4 K + 8 + 4 K + 8) (logits, labels in; dlogits, mask out)
             stitch    npix (4 K + 8 + 4 K)     (logits in; mask, probabilities out)
           Kernel time comes from rocprofv3 in runs of their own: --profile K launches every case of one K --iters times
           (no timing of its own), and --from-stats DIR turns the kernel_stats.csv files under DIR into the table (head
           backward and CE step = main kernel + its reduce / finish kernel, averages per launch).  Without those options the
           same cases are also timed in process: --iters launches back to back between one event pair, queued behind a
           sleep kernel so the window holds device time only.
  segment  tester.segment of a 4096^2 image at K = 2 and K = 4 (fp32, automatic tile size), probabilities off.

    timeout -k 10 900 python tools/multiclass_time.py [--reps 5] [--iters 50] [--json out.json]
    for K in 2 3 4 8; do rocprofv3 --kernel-trace --stats -d prof/K$K -o run --output-format csv -- \
        python tools/multiclass_time.py --profile $K; done
    python tools/multiclass_time.py --from-stats prof
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dl-unet_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import _hip  # noqa: E402
import network  # noqa: E402
import optim  # noqa: E402
import tester  # noqa: E402

HBM = 8e12
KS = (2, 3, 4, 8)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(cases, reps, warm=2):
    """cases: {name: fn}; every rep runs every case once, in turn; returns {name: median ms}."""
    for _ in range(warm):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            ms[k].append(timed(fn))
    return {k: float(np.median(v)) for k, v in ms.items()}


def back_to_back(fn, iters, reps):
    """Median over reps of the device time per launch of `iters` launches of fn between one event pair.  A sleep kernel
    is queued first, so the host enqueues the whole window while the device is busy: the window holds no host time."""
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        torch.cuda._sleep(50_000_000)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return float(np.median(ms))


def step_case(K, math, loss, dev, B=8, S=572):
    L = _hip.lib()
    net = network.Unet(n_classes=K).to(dev)
    opt = optim.SGD(net.parameters(), lr=1e-4, momentum=0.99)
    g = torch.Generator(device="cpu").manual_seed(K)
    x = torch.rand(B, 1, S, S, generator=g).to(dev)
    lab = torch.randint(0, K, (B, 1, S - 184, S - 184), generator=g).to(dev)

    def fn():
        _hip.check(L.unet_set_math(math), "unet_set_math")
        opt.zero_grad()
        preds = net(x)
        if loss == "bce":
            l, _ = optim.bce_argmax_step(preds, lab, want_mask=False)
        else:
            l, _ = optim.softmax_ce_step(preds, lab, want_mask=False, validate=False)
        l.backward()
        opt.step()
    return fn


def kernel_bytes(K, math, B=8, So=388, C=64):
    """Algorithmic HBM bytes of each kernel case (see the module docstring)."""
    es = 2 if math == 2 else 4
    npix = B * So * So
    tag = "%s K=%d" % ("bf16" if es == 2 else "fp32", K)
    nbytes = {"head fwd " + tag: npix * (es * C + 4 * K), "head bwd " + tag: npix * (2 * es * C + 4 * K)}
    if es == 4:
        nbytes["CE step K=%d" % K] = npix * (8 * K + 16)
        nbytes["stitch K=%d" % K] = npix * (8 * K + 8)
    return nbytes


def kernel_cases(K, math, dev, B=8, So=388, C=64, shapes_only=False):
    if shapes_only:
        return None, kernel_bytes(K, math, B, So, C)
    L = _hip.lib()
    es = 2 if math == 2 else 4
    npix = B * So * So
    g = torch.Generator(device="cpu").manual_seed(100 + K)
    x = torch.randn(B, So, So, C, generator=g).to(dev).to(torch.bfloat16 if es == 2 else torch.float32)
    w = (torch.randn(K, C, generator=g) * 0.1).to(dev)
    b = torch.zeros(K, device=dev)
    y = torch.empty(B, K, So, So, device=dev)
    dl = (torch.randn(B, K, So, So, generator=g) * 1e-3).to(dev)
    dz = torch.empty_like(x)
    dw, db = torch.empty(K, C, device=dev), torch.empty(K, device=dev)
    sc = torch.empty(L.unet_head1xk_bwd_scratch_bytes(B, So, So, C, K), dtype=torch.uint8, device=dev)
    lab = torch.randint(0, K, (B, So, So), generator=g).to(dev)
    loss = torch.empty((), device=dev)
    inv = torch.empty((), dtype=torch.int64, device=dev)
    mask = torch.empty(B, So, So, dtype=torch.int64, device=dev)
    csc = torch.empty(L.unet_softmax_ce_scratch_bytes(npix), dtype=torch.uint8, device=dev)
    prob = torch.empty(B, K, So, So, device=dev)
    st = lambda: _hip.stream(dev)  # noqa: E731

    def setm():
        _hip.check(L.unet_set_math(math), "unet_set_math")

    def fwd():
        setm()
        _hip.check(L.unet_head1xk_fwd(_hip.ptr(x), B, So, So, C, K, _hip.ptr(w), _hip.ptr(b), _hip.ptr(y), st()), "fwd")

    def bwd():
        setm()
        _hip.check(L.unet_head1xk_bwd(_hip.ptr(x), B, So, So, C, K, _hip.ptr(w), _hip.ptr(dl), _hip.ptr(dz), _hip.ptr(dw), _hip.ptr(db),
                                      _hip.ptr(sc), st()), "bwd")

    def ce():
        _hip.check(L.unet_softmax_ce_step(_hip.ptr(y), y.stride(0), y.stride(1), y.stride(2), K, _hip.ptr(lab), None, 0, 0, 0, B, So, So,
                                          _hip.ptr(loss), _hip.ptr(dl), 1.0, _hip.ptr(mask), _hip.ptr(inv), _hip.ptr(csc), st()), "ce")

    def stitch():                              # B tiles of So^2 = a B x 1 grid of an So x (B So) image, every pixel in one tile
        _hip.check(L.unet_tile_stitch_k(_hip.ptr(y), So, K, 0, 0, 1, B, 0, B, 1, So, B * So, _hip.ptr(mask), _hip.ptr(prob), st()),
                   "stitch")
    tag = "%s K=%d" % ("bf16" if es == 2 else "fp32", K)
    cases = {"head fwd " + tag: fwd, "head bwd " + tag: bwd}
    if es == 4:
        cases["CE step K=%d" % K] = ce
        cases["stitch K=%d" % K] = stitch
    return cases, kernel_bytes(K, math, B, So, C)


# rocprofv3 kernel names of each case (C = 64): (substrings that must all occur, typed); typed kernels are told apart by their
# activation type (bf16 tensors are unsigned short); the first entry is the main kernel
def _case_kernels(case):
    if case.startswith("head fwd"):
        return [(("head", "_fwd_kernel<64, "), True)]
    if case.startswith("head bwd"):
        return [(("head", "_bwd_kernel<64, "), True), (("head", "bwd_reduce_kernel"), False)]
    if case.startswith("CE step"):
        return [(("softmax_ce_kernel<",), False), (("softmax_ce_final_kernel",), False)]
    return [(("tile_stitch_k_kernel<",), False)]


def _match(stats, need, typed, bf16):
    return [v for n, v in stats.items() if all(p in n for p in need) and (not typed or ("unsigned short" in n) == bf16)]


def read_stats(path):
    """{kernel name: average ns} of one rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            keys = {k.lower(): k for k in row}
            name = row[keys.get("name", keys.get("kernel_name", list(row)[0]))]
            avg = row.get(keys.get("averagens", ""), None)
            if avg is None:
                tot = float(row[keys["totaldurationns"]])
                avg = tot / float(row[keys["calls"]])
            out[name] = float(avg)
    return out


def from_stats(root, K_list=KS):
    """Table of kernel time (rocprofv3 averages) and HBM fraction per case, from <root>/K<k>/**/*kernel_stats.csv."""
    res = {}
    for K in K_list:
        files = glob.glob(os.path.join(root, "K%d" % K, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("no kernel_stats.csv under %s/K%d" % (root, K))
        stats = {}
        for f in files:
            stats.update(read_stats(f))
        for math in (3, 2):
            _, nbytes = kernel_cases(K, math, None, shapes_only=True)
            for case, nb in nbytes.items():
                ns = 0.0
                for need, typed in _case_kernels(case):
                    hit = _match(stats, need, typed, "bf16" in case)
                    if len(hit) != 1:
                        raise SystemExit("case %r: kernel %r matched %d names in %s" % (case, need, len(hit), sorted(stats)))
                    ns += hit[0]
                res[case] = {"ms": ns * 1e-6, "bytes": nb, "hbm_frac": nb / (ns * 1e-9) / HBM}
    print("kernels, B = 8, 388^2 (C = 64), rocprofv3 kernel time (average per launch)")
    for k, v in res.items():
        print("  %-22s %8.3f ms   %6.3f GB   %.2f of 8 TB/s" % (k, v["ms"], v["bytes"] / 1e9, v["hbm_frac"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window (kernels) / per profiled case")
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile", type=int, default=None, help="launch every kernel case of this K --iters times, no timing")
    ap.add_argument("--from-stats", default=None, help="directory of rocprofv3 runs (K<k>/...) to tabulate")
    args = ap.parse_args()
    if args.from_stats:
        res = from_stats(args.from_stats)
        if args.json:
            with open(args.json, "w") as f:
                json.dump({"kernels_rocprof": res}, f, indent=1)
        return
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    L = _hip.lib()
    if args.profile is not None:
        default_math = L.unet_get_math()
        for math in (3, 2):
            cases, _ = kernel_cases(args.profile, math, dev)
            for fn in cases.values():
                for _ in range(args.iters):
                    fn()
            torch.cuda.synchronize()
            del cases
        _hip.check(L.unet_set_math(default_math), "unet_set_math")
        return
    default_math = L.unet_get_math()
    out = {}

    steps = {}
    for math in (3, 2):
        mname = "fp32" if math == 3 else "bf16"
        steps["%s K=2 bce" % mname] = step_case(2, math, "bce", dev)
        for K in KS:
            steps["%s K=%d softmax_ce" % (mname, K)] = step_case(K, math, "softmax_ce", dev)
    res = alternate(steps, args.reps)
    print("training step, B = 8, 572^2 (median of %d, shapes alternated)" % args.reps)
    for k, v in res.items():
        base = res[k.split()[0] + " K=2 bce"]
        print("  %-26s %8.2f ms   %+6.2f %% vs the binary BCE step" % (k, v, 100.0 * (v / base - 1.0)))
    out["step_ms"] = res
    del steps
    torch.cuda.empty_cache()

    kc, nb = {}, {}
    for K in KS:
        for math in (3, 2):
            c, n = kernel_cases(K, math, dev)
            kc.update(c)
            nb.update(n)
    for fn in kc.values():                           # warm every case
        fn()
    res = {k: back_to_back(fn, args.iters, args.reps) for k, fn in kc.items()}
    print("kernels, B = 8, 388^2 (C = 64), %d launches back to back per event pair (median of %d)" % (args.iters, args.reps))
    out["kernels"] = {}
    for k, v in res.items():
        frac = nb[k] / (v * 1e-3) / HBM
        print("  %-22s %8.3f ms   %6.3f GB   %.2f of 8 TB/s" % (k, v, nb[k] / 1e9, frac))
        out["kernels"][k] = {"ms": v, "bytes": nb[k], "hbm_frac": frac}
    del kc
    torch.cuda.empty_cache()
    _hip.check(L.unet_set_math(3), "unet_set_math")

    seg = {}
    img = torch.rand(4096, 4096, generator=torch.Generator(device="cpu").manual_seed(0)).to(dev)
    for K in (2, 4):
        net = network.Unet(n_classes=K).to(dev)
        seg["segment 4096^2 K=%d" % K] = (lambda n: (lambda: tester.segment(n, img)))(net)
    res = alternate(seg, max(3, args.reps // 2), warm=1)
    print("segment, 4096^2, fp32")
    for k, v in res.items():
        print("  %-22s %8.1f ms   %+6.2f %% vs K=2" % (k, v, 100.0 * (v / res["segment 4096^2 K=2"] - 1.0)))
    out["segment_ms"] = res
    _hip.check(L.unet_set_math(default_math), "unet_set_math")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
