"""Depth Anything 3's ray-based cameras at the scorer's size: 10 views, ray maps of 160 x 288 (a 504 x 280 input) and 192 x 288, synthetic rays of a
known camera (Gaussian noise, a fifth of the rays outliers), so nearly every view has more than 8000 inliers and the refit draws its subset.

    python tools/da3_ray_pose_bench.py --json profiles/da3_ray_pose.json                          the measurement
    python tools/da3_ray_pose_bench.py --calls N                                                   N calls per size and nothing else, for a kernel trace
    python tools/da3_ray_pose_bench.py --merge --json PATH --kernel-stats DIR --traced-calls N     add the trace's statistics to PATH (no device needed)

Per size (ms over device events around a synchronised loop, warmed up): ops.da3_ray_pose per clip with a drawn sample table, as the network calls it;
its three C-ABI calls through ops.KernelTimer (weights; ransac = fit + score + select + mask; refit); the plain-torch restatement of
tests/da3_raypose_ref.py in float64 on the same device and inputs.  Then DepthAnything3("da3-large", random weights).inference on 10 frames of
504 x 280 with and without use_ray_pose (the option adds the head's auxiliary branch).  --kernel-stats: the output directory of
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/da3_ray_pose_bench.py --calls N` (a run of its own; its inputs are copied in, so every
dispatch of the trace belongs to the calls): per-kernel time and the launches per call are taken from there."""
import csv
import glob
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((160, 288), (192, 288))
VIEWS = 10


def synthetic(views, ph, pw, seed=0):
    """host tensors: ray fp32 [1,views,ph,pw,6], conf fp32 [1,views,ph,pw]"""
    import da3_raypose_ref as R
    g = torch.Generator().manual_seed(seed)
    gx, gy = R.plane_grid(ph, pw)
    N = ph * pw
    p = torch.stack([gx.double().view(1, pw).expand(ph, pw), gy.double().view(ph, 1).expand(ph, pw), torch.ones(ph, pw, dtype=torch.float64)], -1).reshape(N, 3)
    rays, confs = [], []
    for _ in range(views):
        r = torch.rand(6, generator=g, dtype=torch.float64)
        axis = (r[:3] - 0.5) / (r[:3] - 0.5).norm()
        K = torch.tensor([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=torch.float64)
        ang = 0.1 + 0.4 * float(r[3])
        rot = torch.eye(3, dtype=torch.float64) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
        L = torch.diag(torch.tensor([1 / (0.9 + float(r[4])), 1 / (0.9 + float(r[5])), 1.0], dtype=torch.float64))
        d = p @ (rot @ L).T
        d = d / d.norm(dim=1, keepdim=True) + 0.01 * torch.randn(N, 3, generator=g, dtype=torch.float64)
        conf = 1 + torch.exp(0.5 * torch.randn(N, generator=g, dtype=torch.float64))
        out = torch.randperm(N, generator=g)[:N // 5]
        d[out] = torch.randn(out.numel(), 3, generator=g, dtype=torch.float64)
        conf[out] = 1 + 0.1 * torch.rand(out.numel(), generator=g, dtype=torch.float64)
        t = 0.05 * torch.randn(N, 3, generator=g, dtype=torch.float64)
        rays.append(torch.cat([d, t], -1).float().reshape(ph, pw, 6))
        confs.append(conf.float().reshape(ph, pw))
    return torch.stack(rays)[None].contiguous(), torch.stack(confs)[None].contiguous()


def _timeit(f, n):
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def calls_only(n):
    from videogpa_amd import ops
    for ph, pw in SIZES:
        ray, conf = (t.cuda() for t in synthetic(VIEWS, ph, pw))
        for _ in range(n):
            ops.da3_ray_pose(ray, conf, (14 * ph // 8, 14 * pw // 8))
        torch.cuda.synchronize()


def kernel_stats(directory, calls):
    """A rocprofv3 kernel trace (its *_results.db, or *kernel_stats.csv with --output-format csv) -> per-kernel launches per da3_ray_pose call and
    mean time for this file's kernels, all dispatches per call, and the summed kernel time per call"""
    rows = []                                                   # (name, calls, total ns)
    dbs = glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True)
    csvs = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if dbs:
        import sqlite3
        rows = list(sqlite3.connect(dbs[0]).execute("select name, count(*), sum(end - start) from kernels group by name"))
    elif csvs:
        with open(csvs[0]) as f:
            rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(f)]
    else:
        raise FileNotFoundError(f"no kernel trace under {directory}")
    ours = {name.split("(")[0].split(" ")[-1]: {"launches_per_call": n / calls, "avg_us": ns / n / 1e3} for name, n, ns in rows if "da3_ray_" in name}
    return {"source": "rocprofv3 --kernel-trace, a run of its own, both sizes together", "calls_traced": calls,
            "launches_per_call_all_kernels": sum(r[1] for r in rows) / calls, "kernel_time_per_call_ms": sum(r[2] for r in rows) / calls / 1e6,
            "own_kernels_per_call_ms": sum(v["launches_per_call"] * v["avg_us"] for v in ours.values()) / 1e3, "kernels": ours}


def run(quick=False):
    import da3_raypose_ref as R
    from videogpa_amd import ops
    from videogpa_amd.da3 import DepthAnything3
    n = 3 if quick else 20
    rows = {"device": torch.cuda.get_device_name(0), "views": VIEWS, "sizes": {}}
    for ph, pw in SIZES:
        hw = (14 * ph // 8, 14 * pw // 8)
        ray, conf = (t.cuda() for t in synthetic(VIEWS, ph, pw))
        _, _, info = ops.da3_ray_pose(ray, conf, hw)
        row = {"points_per_view": ph * pw, "image_hw": list(hw), "n_inliers": info["n_inliers"].flatten().tolist(), "n_used": info["n_used"].flatten().tolist()}
        row["da3_ray_pose_ms"] = _timeit(lambda: ops.da3_ray_pose(ray, conf, hw), n)
        row["da3_ray_pose_given_table_ms"] = _timeit(lambda: ops.da3_ray_pose(ray, conf, hw, sample_idx=info["sample_idx"]), n)
        ops.TIMER = ops.KernelTimer()
        for _ in range(n):
            ops.da3_ray_pose(ray, conf, hw)
        torch.cuda.synchronize()
        row["c_abi_calls_ms"] = {k: v["avg_ms"] for k, v in ops.TIMER.summary().items()}
        ops.TIMER = None
        gen = torch.Generator(device="cuda").manual_seed(0)
        row["torch_restatement_fp64_ms"] = _timeit(lambda: R.ray_pose(ray, conf, hw, info["sample_idx"], 0.2, torch.float64, gen), 3)
        rows["sizes"][f"{ph}x{pw}"] = row
        print(f"{VIEWS} views {ph} x {pw}: da3_ray_pose {row['da3_ray_pose_ms']:.3f} ms (given table {row['da3_ray_pose_given_table_ms']:.3f}), "
              f"calls {row['c_abi_calls_ms']}, torch restatement {row['torch_restatement_fp64_ms']:.1f} ms")
    torch.manual_seed(0)
    with torch.device("cuda"):
        api = DepthAnything3("da3-large").eval()
    frames = (torch.rand(VIEWS, 280, 504, 3, generator=torch.Generator().manual_seed(1)) * 255).to(torch.uint8).cuda()
    inf = {"frames": [VIEWS, 280, 504], "weights": "random (da3-large preset)"}
    inf["inference_ms"] = _timeit(lambda: api.inference(frames), max(2, n // 4))
    try:
        inf["inference_use_ray_pose_ms"] = _timeit(lambda: api.inference(frames, use_ray_pose=True), max(2, n // 4))
    except ValueError as e:                                   # random weights can leave a view without 4 inliers: the network alone, and the op from above
        x = api.input_processor(api._get_model_device()).process(frames, None, None, 504, "upper_bound_resize")[0]
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            inf["network_aux_true_ms"] = _timeit(lambda: api.model(x, aux=True), max(2, n // 4))
            inf["network_aux_false_ms"] = _timeit(lambda: api.model(x, aux=False), max(2, n // 4))
        inf["inference_use_ray_pose_ms"] = None
        inf["note"] = f"inference(use_ray_pose=True) raised on random weights ({e}); the auxiliary branch is network_aux_true_ms - network_aux_false_ms"
    rows["inference"] = inf
    print(inf)
    return rows


if __name__ == "__main__":
    if "--calls" in sys.argv:
        calls_only(int(sys.argv[sys.argv.index("--calls") + 1]))
        sys.exit(0)
    if "--merge" in sys.argv:                                  # no device needed: add a trace's statistics to a measurement written earlier
        with open(sys.argv[sys.argv.index("--json") + 1]) as f:
            rows = json.load(f)
    else:
        rows = run(quick="--quick" in sys.argv)
    if "--kernel-stats" in sys.argv:
        calls = int(sys.argv[sys.argv.index("--traced-calls") + 1]) if "--traced-calls" in sys.argv else 10
        rows["kernel_trace"] = kernel_stats(sys.argv[sys.argv.index("--kernel-stats") + 1], calls * len(SIZES))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)
