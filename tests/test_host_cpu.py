"""CPU-only checks: the C-ABI library loads and exports every declared symbol, host-side logic
(size contract, drop-in module surface, helper functions), and the data-parallel bucket reducer
over gloo with world_size 2."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_builds_loads_and_exports_every_declared_symbol():
    import _hip
    _hip.build()
    L = _hip.lib()
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr)))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(L, name), "libunet_hip.so does not export %s" % name
    assert sorted(_hip.EXPORTS) == declared          # the ctypes table covers the whole header
    assert L.unet_abi_version() == 4


def test_size_contract_no_gpu_needed():
    import _hip
    L = _hip.lib()
    out = C.c_int()
    for S, So in ((188, 4), (220, 36), (380, 196), (572, 388), (700, 516), (1212, 1028)):
        assert L.unet_output_size(S, C.byref(out)) == 0 and out.value == So
    for S in (570, 571, 204, 172, 60, 0, -4):
        assert L.unet_output_size(S, C.byref(out)) == -1
        assert b"16L+60" in L.unet_last_error()


def test_module_surface_matches_reference(golden_dir):
    import network
    ka = np.load(os.path.join(golden_dir, "known_answers.npz"))
    torch.manual_seed(0)
    m = network.Unet()
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in ka["init_keys"]]
    assert [repr(tuple(p.shape)) for p in m.parameters()] == [str(s) for s in ka["init_shapes"]]
    assert list(m.state_dict().keys()) == [str(k) for k in ka["init_keys"]]
    # same RNG consumption and init formulas as the reference: bit-identical parameters for a seed
    first = np.stack([p.detach().flatten()[:2].numpy() for p in m.parameters()])
    assert np.array_equal(first, ka["init_seed0_first"])
    # crop_and_concat stays a public method with the reference's pad / crop / odd-raises behaviour
    A = torch.arange(2 * 3 * 4 * 4, dtype=torch.float32).reshape(2, 3, 4, 4)
    B = torch.arange(2 * 2 * 8 * 8, dtype=torch.float32).reshape(2, 2, 8, 8)
    assert np.array_equal(m.crop_and_concat(A, B).numpy(), ka["cac_pad"])
    assert np.array_equal(m.crop_and_concat(B, A).numpy(), ka["cac_crop"])
    with pytest.raises(RuntimeError):
        m.crop_and_concat(A, torch.zeros(2, 2, 7, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 188, 188))


def test_functions_known_answers(golden_dir):
    import functions
    ka = np.load(os.path.join(golden_dir, "known_answers.npz"))
    for orig in (196, 388, 512, 1024, 100, 20):
        assert tuple(ka["isc_%d" % orig]) == functions.input_size_compute(torch.zeros(1, 1, orig, orig))
    p = torch.tensor([[1, 1, 0], [0, 1, 0], [0, 0, 0]]); l = torch.tensor([[1, 0, 0], [0, 1, 1], [0, 0, 0]])
    assert np.allclose(functions.evaluation_metrics(p, l), ka["evalm"])
    assert np.array_equal(functions.class_balance(l[None]).numpy(), ka["class_balance"])
    from oracle import prng
    lab = torch.from_numpy(prng.make_labels(3, 2, 36)[:, 0])
    assert np.array_equal(functions.class_balance(lab).numpy(), ka["class_balance_rand"])


def test_trainer_goal_identity_semantics(golden_dir):
    """trainer.py:18-27: `DATASET is '<literal>'`.  Pinned against the reference's own run (trainer_golden.json):
    only a caller's literal 'ISBI2012' arms the goal."""
    import json
    import trainer
    gold = json.load(open(os.path.join(golden_dir, "trainer_golden.json")))["cases"]
    assert trainer._goal_for("ISBI2012") == (1, 0.0611) and gold["literal_ISBI2012"]["goal_lines"]
    assert trainer._goal_for("".join(["ISBI", "2012"])) == (None, None) and not gold["runtime_ISBI2012"]["goal_lines"]
    assert trainer._goal_for("DIC-C2DH-HeLa") == (None, None) and not gold["literal_DIC-C2DH-HeLa"]["goal_lines"]
    assert "models/unet_weight_save_ISBI2012.pth" in gold["literal_ISBI2012"]["files"]
    assert "models/unet_weight_save_latest.pth" not in gold["literal_ISBI2012"]["files"]


def test_rccl_binds_without_a_gpu():
    import _hip
    assert _hip.lib().unet_dp_rccl_version() > 20000          # librccl found and its symbols bound (no communicator yet)
    assert _hip.lib().unet_dp_world(None) == 0


def test_grad_buckets_layout():
    import dp
    numels = [10, 3, 64, 7]
    b = dp.GradBuckets(numels, order=[3, 2, 0, 1], bounds=[0, 2, 4])
    flat, views = b.allocate([(10,), (3,), (8, 8), (7,)], "cpu")
    assert b.total == 64 * 4 and flat.numel() == b.total
    assert [v.numel() for v in views] == numels
    assert b.bucket_range(0) == (0, 128) and b.bucket_range(1) == (128, 256)
    for i, v in enumerate(views):
        v.fill_(i + 1)
    assert flat[0] == 4 and flat[64] == 3 and flat[128] == 1 and flat[192] == 2
    assert dp.shard_batch(8, 1, 2) == (4, 8)
    with pytest.raises(ValueError):
        dp.shard_batch(7, 0, 2)


_DP_WORKER = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.path.join(sys.argv[1], "dl-unet_amd")); sys.path.insert(0, sys.argv[1])
import dp
from oracle import prng, torch_ref
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.set_num_threads(2)
S, Bg = 188, 2
params = torch_ref.params_to_torch(prng.make_params(0), torch.float64, requires_grad=True)
names = list(params.keys())
x = torch.from_numpy(prng.make_input(1, Bg, S)).double()
dl = torch.from_numpy(prng.make_cotangent(2, (Bg, 2, 4, 4))).double()
lo, hi = dp.shard_batch(Bg, rank, world)
# per-rank backward on its shard with dlogits pre-scaled by 1/world (what network._UnetFunction does)
torch_ref.unet_forward(params, x[lo:hi]).backward(dl[lo:hi] * (1.0 / world))
numels = [params[k].numel() for k in names]
order = list(reversed(range(len(names))))            # completion order: reverse layer order
bounds = [0, 8, 14, 20, 26, 30, 46]
b = dp.GradBuckets(numels, order, bounds)
flat, views = b.allocate([params[k].shape for k in names], "cpu", torch.float64)
for v, k in zip(views, names):
    v.copy_(params[k].grad)
works = [b.reduce_stage(flat, s) for s in range(b.n_stages())]
for w in works:
    w.wait()
if rank == 0:
    ref = torch_ref.params_to_torch(prng.make_params(0), torch.float64, requires_grad=True)
    torch_ref.unet_forward(ref, x).backward(dl / world)        # the global-batch MEAN gradient
    worst = max(((v - ref[k].grad).abs().max() / ref[k].grad.abs().max()).item() for v, k in zip(views, names))
    print("WORST", worst)
    assert worst < 1e-12, worst
dist.destroy_process_group()
'''


def test_dp_bucket_allreduce_equals_global_batch_gradient_gloo(tmp_path):
    """N-rank (pre-scaled, SUM-reduced, bucketed) gradients == single-rank global-batch mean gradient.
    Runs 2 gloo ranks on CPU; gradients come from the torch restatement (test infrastructure)."""
    script = os.path.join(tmp_path, "dp_worker.py")
    with open(script, "w") as f:
        f.write(_DP_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29531", WORLD_SIZE="2", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, script, ROOT], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
    assert "WORST" in outs[0]


def test_bench_line_is_short_and_keeps_the_contract_fields():
    """The driver keeps an 8 KB tail of stdout: the result line must stay far below it whatever the tables hold.  Input:
    round 2's committed full result (27 KB, 75 layer rows) through bench.split_line."""
    import json
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r02_e_bench.json")))
    full["cpu_baseline"].update({"gflops": 790.0, "iters": 5, "s_per_iter": 1.1,
                                 "logits_parity": {"max_abs_err_over_max_abs_ref": 2.1e-6, "bound": 1e-3, "ok": True}})
    full["comm"] = {"gradient_allreduce": "rccl", "ranks": 8, "rccl_version": 22204, "message_mb": 124.1, "buckets": 6,
                    "self_launched": True, "allreduce_ms_per_step": 1.234567, "exposed_ms_per_step": 0.123456}
    full["roofline"]["traffic_source"] = bench.pmc_traffic(3, "wino", 8)[1] + " " * 0
    full["bf16"] = {"ms_per_step": 9.56123456, "tiles_per_s": 836.7123456, "steps": 10, "warmup": 3, "kernel": "igemmb3+igemmb+convb64", "frac": 0.3612345,
                    "peak": 2500.0, "logits_err": 0.0181234, "argmax_flips": 39, "px": 150544, "what": "x" * 400, "parity_note": "y" * 300}
    line, detail = bench.split_line(full, "gpurun_out/bench_detail.json")
    assert len(json.dumps(line["bf16"])) <= 300 and "what" not in line["bf16"]
    for k in ("ms_per_step", "tiles_per_s", "frac", "logits_err", "argmax_flips"):
        assert k in line["bf16"], k
    text = json.dumps(line)
    assert len(text) < bench.LINE_LIMIT <= 4096, len(text)
    back = json.loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "comm", "detail"):
        assert k in back, k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "launches_per_step", "alg_bytes_per_launch"):
        assert k in back["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample", "gflops", "logits_parity"):
        assert k in back["cpu_baseline"], k
    assert "workload" in back["config"] and "model" not in back["config"]
    assert "layers" not in back and "kernels" not in back and "table" not in back["cpu_baseline"]
    assert len(detail["layers"]) > 50                      # nothing is lost: the side file has the tables
    # free text cannot push the numbers out: an absurdly long kernel name is cut
    full["roofline"]["kernel"] = "k" * 5000
    assert len(json.dumps(bench.split_line(full, "x.json")[0])) < bench.LINE_LIMIT


def test_bench_gpus_n_starts_its_own_ranks_dry_launch():
    """`python3 bench.py --gpus N` without WORLD_SIZE must launch N child ranks itself (the driver's plain command);
    --dry-launch prints what it would start.  No torch import, no GPU."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "7", "--warmup", "2", "--math", "2", "--dry-launch"],
                         env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    spec = json.loads(out.stdout.strip().splitlines()[-1])["launch"]
    assert len(spec) == 4
    ports = set()
    for r, s in enumerate(spec):
        assert s["argv"][0] == sys.executable and s["argv"][1].endswith("bench.py")
        assert "--dry-launch" not in s["argv"] and s["argv"][2:] == ["--gpus", "4", "--steps", "7", "--warmup", "2", "--math", "2"]
        e = s["env"]
        assert e["RANK"] == str(r) and e["LOCAL_RANK"] == str(r) and e["WORLD_SIZE"] == "4"
        assert e["MASTER_ADDR"] == "127.0.0.1" and e["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
        ports.add(e["MASTER_PORT"])
    assert len(ports) == 1


def test_bench_launcher_relays_rank0_line_and_exit_codes(tmp_path):
    """The launcher itself (bench.launch) with stand-in children: rank 0's JSON line is relayed, a failing rank's exit code
    comes back and the other ranks are stopped."""
    import bench
    script = os.path.join(tmp_path, "child.py")
    with open(script, "w") as f:
        f.write("import os, sys, time, json\n"
                "r = int(os.environ['RANK']); mode = sys.argv[1]\n"
                "if mode == 'ok':\n"
                "    print('chatter from rank %d' % r)\n"
                "    if r == 0: print(json.dumps({'metric': 'm', 'value': 1.5, 'n_gpus': int(os.environ['WORLD_SIZE'])}))\n"
                "elif mode == 'fail':\n"
                "    if r == 1: sys.exit(7)\n"
                "    time.sleep(60)\n")
    runner = os.path.join(tmp_path, "run.py")
    with open(runner, "w") as f:
        f.write("import sys; sys.path.insert(0, %r)\nimport bench\n"
                "bench.child_specs = lambda args, argv, port=None: [([sys.executable, %r, argv[0]], {'RANK': str(r), 'WORLD_SIZE': str(args.gpus)}) for r in range(args.gpus)]\n"
                "args = bench.parse_args(['--gpus', '3'])\n"
                "sys.exit(bench.launch(args, [sys.argv[1]]))\n" % (ROOT, script))
    ok = subprocess.run([sys.executable, runner, "ok"], capture_output=True, text=True, timeout=60)
    assert ok.returncode == 0, ok.stderr
    import json
    assert json.loads(ok.stdout.strip()) == {"metric": "m", "value": 1.5, "n_gpus": 3}       # exactly one line on stdout
    assert "chatter from rank 1" in ok.stderr
    t0 = __import__("time").time()
    bad = subprocess.run([sys.executable, runner, "fail"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 7 and bad.stdout.strip() == "" and __import__("time").time() - t0 < 30


def test_bench_launcher_restarts_the_ranks_with_comm_torch_after_a_hung_rccl_bring_up(tmp_path):
    """First contact with N GPUs cannot be rehearsed, so its failure mode is: a rank whose unet_dp_init does not return within
    BENCH_DP_INIT_TIMEOUT ends itself with exit code 3 (bench._call_with_watchdog, here with a stand-in that sleeps for ever);
    the launcher - a parent that never touched a GPU - stops the other ranks and starts all of them ONCE more, as fresh
    processes, with `--comm torch`; a second failure is final."""
    import json
    import bench
    # (a) the watchdog itself, in a process of its own (it ends the process)
    probe = os.path.join(tmp_path, "probe.py")
    with open(probe, "w") as f:
        f.write("import sys, time; sys.path.insert(0, %r)\nimport bench\n"
                "print(bench._call_with_watchdog(lambda: 41 + 1, 5, 'quick call'))\n"
                "try:\n    bench._call_with_watchdog(lambda: 1 / 0, 5, 'raising call')\nexcept ZeroDivisionError:\n    print('raised')\n"
                "sys.stdout.flush()\n"
                "bench._call_with_watchdog(lambda: time.sleep(600), 0.5, 'unet_dp_init stand-in')\nprint('not reached')\n" % ROOT)
    t0 = __import__("time").time()
    r = subprocess.run([sys.executable, probe], capture_output=True, text=True, timeout=60)
    assert r.returncode == bench.EXIT_DP_INIT_TIMEOUT and r.stdout.split() == ["42", "raised"], (r.returncode, r.stdout, r.stderr)
    assert "unet_dp_init stand-in has not returned" in r.stderr and __import__("time").time() - t0 < 30
    # (b) the launcher: children hang in "rccl" mode (rank 1 reports it with code 3), succeed once relaunched with --comm torch
    child = os.path.join(tmp_path, "child.py")
    with open(child, "w") as f:
        f.write("import os, sys, time, json\n"
                "r = int(os.environ['RANK']); args = sys.argv[1:]\n"
                "open(os.path.join(%r, 'seen_%%d_%%s' %% (r, 'torch' if 'torch' in args else 'rccl')), 'w').write(os.environ['MASTER_PORT'])\n"
                "if 'torch' not in args:\n"
                "    if r == 1: time.sleep(0.3); sys.exit(3)\n"
                "    time.sleep(600)\n"
                "if 'always-hang' in args:\n"
                "    sys.exit(3)\n"
                "if r == 0: print(json.dumps({'metric': 'm', 'value': 2.5, 'comm': args}))\n" % str(tmp_path))
    runner = os.path.join(tmp_path, "run.py")
    with open(runner, "w") as f:
        f.write("import sys; sys.path.insert(0, %r)\nimport bench\n"
                "real = bench.child_specs\n"
                "def specs(args, argv, port=None):\n"
                "    return [([sys.executable, %r] + argv[len(argv) - argv[::-1].index('--') if '--' in argv else 0:], e) for _, e in real(args, argv, port)]\n"
                "bench.child_specs = specs\n"
                "argv = ['--gpus', '3'] + sys.argv[1:]\n"
                "sys.exit(bench.launch(bench.parse_args(['--gpus', '3']), argv))\n" % (ROOT, child))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    ok = subprocess.run([sys.executable, runner, "--", "x"], capture_output=True, text=True, timeout=60, env=env)
    assert ok.returncode == 0, ok.stderr
    got = json.loads(ok.stdout.strip())
    assert got["value"] == 2.5 and got["comm"][-2:] == ["--comm", "torch"]
    assert "starting the ranks again with --comm torch" in ok.stderr
    seen = sorted(n for n in os.listdir(tmp_path) if n.startswith("seen_"))
    assert seen == ["seen_%d_%s" % (r, m) for r in range(3) for m in ("rccl", "torch")]
    ports = {m: {open(os.path.join(tmp_path, "seen_%d_%s" % (r, m))).read() for r in range(3)} for m in ("rccl", "torch")}
    assert len(ports["rccl"]) == 1 and len(ports["torch"]) == 1 and ports["rccl"] != ports["torch"]      # one free port per attempt
    bad = subprocess.run([sys.executable, runner, "--", "always-hang"], capture_output=True, text=True, timeout=60, env=env)
    assert bad.returncode == 3 and bad.stdout.strip() == ""                                               # only ONE relaunch
    assert bench._with_comm_torch(["--gpus", "8", "--comm", "rccl", "--steps", "5"]) == ["--gpus", "8", "--steps", "5", "--comm", "torch"]
    assert bench._with_comm_torch(["--comm=rccl", "--gpus", "2"]) == ["--gpus", "2", "--comm", "torch"]


def test_bench_quotes_pmc_traffic_only_for_the_kernels_it_was_measured_on(tmp_path, monkeypatch):
    """profiles/pmc_traffic.json carries the fingerprint of dl-unet_amd/csrc it was measured on (tools/summarize_profiles.py);
    bench.py gives `traffic: null` (and says why) when the tree's kernels differ, when the batch is not the profiled one, or
    when no pass exists for the family."""
    import json
    import bench
    sha = bench.csrc_sha()
    assert len(sha) == 16 and sha == bench.csrc_sha()
    root = os.path.join(tmp_path, "repo")
    os.makedirs(os.path.join(root, "profiles"))
    os.makedirs(os.path.join(root, "dl-unet_amd", "csrc"))
    open(os.path.join(root, "dl-unet_amd", "csrc", "k.hip"), "w").write("// kernel v1\n")
    monkeypatch.setattr(bench, "ROOT", root)
    sha1 = bench.csrc_sha()
    json.dump({"math3": {"source": "profiles/rXX_pmc_summary.md", "csrc_sha": sha1, "wino_hbm_mb_per_launch": 500.0}},
              open(os.path.join(root, "profiles", "pmc_traffic.json"), "w"))
    v, why = bench.pmc_traffic(3, "wino", 8)
    assert v == 500.0e6 and sha1 in why
    assert bench.pmc_traffic(3, "wino", 2)[0] is None and bench.pmc_traffic(3, "igemm", 8)[0] is None and bench.pmc_traffic(2, "igemm", 8)[0] is None
    open(os.path.join(root, "dl-unet_amd", "csrc", "k.hip"), "w").write("// kernel v2\n")
    v, why = bench.pmc_traffic(3, "wino", 8)
    assert v is None and "stale" in why


def test_bench_tables_from_a_synthetic_launch_dump():
    """bench.layer_table / comm_table on a hand-made per-launch dump: row aggregation, the two roofs, which one binds, SURVEY
    row mapping, per-bucket all-reduce time and the exposed wait."""
    import bench
    rows = [
        {"kind": "3", "ms": "0.5", "gflop": "180.0", "exec_gflop": "80.0", "mbytes": "400.0", "row": "conv22c.fwd", "tag": "wino32<1> M=1 N=128 Kd=1152 nsrc=1 tiles=9"},
        {"kind": "3", "ms": "0.5", "gflop": "180.0", "exec_gflop": "80.0", "mbytes": "400.0", "row": "conv22c.fwd", "tag": "wino32<1> M=1 N=128 Kd=1152 nsrc=1 tiles=9"},
        {"kind": "5", "ms": "0.25", "gflop": "0.0", "exec_gflop": "0.0", "mbytes": "1200.0", "row": "pool1.bwd", "tag": "maxpool2_bwd"},
        {"kind": "6", "ms": "0.4", "gflop": "0.0", "exec_gflop": "0.0", "mbytes": "100.0", "row": "allreduce", "tag": "allreduce n=1000 world=8"},
        {"kind": "6", "ms": "0.6", "gflop": "0.0", "exec_gflop": "0.0", "mbytes": "100.0", "row": "allreduce", "tag": "allreduce n=1000 world=8"},
        {"kind": "6", "ms": "0.3", "gflop": "0.0", "exec_gflop": "0.0", "mbytes": "0.0", "row": "allreduce", "tag": "join (exposed wait of the compute stream)"},
    ]
    t = {r["row"]: r for r in bench.layer_table([r for r in rows if r["kind"] != "6"], 2, 3)}
    c = t["conv22c.fwd"]
    assert c["survey"] == "A5" and c["kernels"] == ["wino32"] and abs(c["ms_per_step"] - 0.5) < 1e-12 and c["launches_per_step"] == 1.0
    assert abs(c["mfma_frac"] - (160e9 / 157.3e12) / 1e-3) < 1e-9 and c["bound"] == "mfma" and abs(c["hbm_frac"] - 0.1) < 1e-9
    pl = t["pool1.bwd"]
    assert pl["survey"] == "A3" and pl["bound"] == "hbm" and abs(pl["hbm_frac"] - (1200e6 / 8e12) / 0.25e-3) < 1e-9
    cm = bench.comm_table(rows, 2)
    assert abs(cm["allreduce_ms_per_step"] - 0.5) < 1e-12 and abs(cm["exposed_ms_per_step"] - 0.15) < 1e-12
    assert len(cm["buckets"]) == 1 and abs(cm["buckets"][0]["gb_per_s"] - 0.1 / 0.5e-3) < 1e-6
    # a row above what a streaming copy gets from HBM (0.79 of 8 TB/s) is labelled as partly Infinity-Cache-served
    fast = dict(rows[2], ms="0.17")
    assert bench.layer_table([fast], 1, 3)[0]["bound"] == "hbm+mall" and bench.layer_table([rows[2]], 1, 3)[0]["bound"] == "hbm"
    w = bench.weakest_rows(bench.layer_table([r for r in rows if r["kind"] != "6"], 2, 3), 1)
    assert w[0]["row"] == "pool1.bwd" and abs(w[0]["frac"] - 0.6) < 1e-9


def test_bench_plain_run_options():
    """A plain run is lean: --full (the instrumented pass, bf16 block, CPU baseline, side file) is off by default; --steps
    sets the timed steps and must be >= 1; --dump-launches comes from the instrumented pass and so needs --full."""
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "out", "--dump-launches", "l.csv"])
    assert a.full and a.dump_outputs == "out" and a.dump_launches == "l.csv"
    for bad in (["--steps", "0"], ["--dump-launches", "l.csv"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_bench_dump_outputs_are_fixed_samples_within_the_limit(tmp_path):
    """bench.output_arrays / dump_outputs: small outputs whole, large ones a seeded sample that is the same in every run,
    float64 kept, everything else float32, integers exact; parameters and gradients sampled at the same positions; the
    64 MB limit is enforced."""
    import bench
    g = torch.Generator().manual_seed(0)
    big = torch.rand(bench.DUMP_ELEMS + 1000, generator=g)
    res = {"logits": torch.rand(2, 2, 8, 8, generator=g), "masks": torch.randint(0, 2, (2, 8, 8), generator=g),
           "loss": torch.tensor(0.25), "metrics": np.array([[0.5], [0.125]]), "big": big, "none": None}
    p = torch.nn.Parameter(torch.rand(bench.PARAM_SAMPLE * 3, generator=g))
    p.grad = -2 * p.detach()
    out = bench.output_arrays(res, [p])
    assert set(out) == {"logits", "masks", "loss", "metrics", "big", "params", "grads"}
    assert out["logits"].dtype == np.float32 and np.array_equal(out["logits"], res["logits"].numpy())
    assert out["masks"].dtype == np.float32 and np.array_equal(out["masks"], res["masks"].numpy())
    assert out["loss"].shape == () and out["loss"] == np.float32(0.25)
    assert out["metrics"].dtype == np.float64 and np.array_equal(out["metrics"], res["metrics"])
    idx = bench.sample_index(big.numel(), bench.DUMP_ELEMS, "big")
    assert np.array_equal(idx, bench.sample_index(big.numel(), bench.DUMP_ELEMS, "big")) and np.all(np.diff(idx) > 0)
    assert idx.size == bench.DUMP_ELEMS and np.array_equal(out["big"], big.numpy()[idx])
    assert out["params"].size == bench.PARAM_SAMPLE and np.array_equal(out["grads"], -2 * out["params"])
    assert np.array_equal(bench.output_arrays(res, [p])["big"], out["big"])
    bench.dump_outputs(str(tmp_path / "d"), out)
    for name, a in out.items():
        assert np.array_equal(np.load(tmp_path / "d" / (name + ".npy")), a)
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "e"), {"x": np.zeros(bench.DUMP_BYTES // 4 + 1, np.float32)})
    assert not os.path.exists(tmp_path / "e")
