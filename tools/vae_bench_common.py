"""What tools/vae_bench.py, tools/vae_encode_bench.py and tools/vae_decode_bench.py share: the seeded 5B module, the HIP-event median, the wall-clock
timing of one clip with its peak memory, the per-entry-point table of ops.KernelTimer, and the `--quick / --json` command line."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def seeded_vae(dev, with_decoder=False):
    """the 5B AutoencoderKLCogVideoX as a bfloat16 module with seeded random weights that keep activations O(1): He-scaled convolutions, norms near
    identity, the decoder's conv_y around 1 and conv_b small.  Returns (vae, generator): the inputs are drawn from the same generator after the weights."""
    from videogpa_amd.vae import AutoencoderKLCogVideoX
    g = torch.Generator().manual_seed(0)
    vae = AutoencoderKLCogVideoX(with_decoder=with_decoder)
    with torch.no_grad():
        for name, p in vae.named_parameters():
            if ".conv_y." in name or ".conv_b." in name:
                p.copy_((1.0 if name.endswith("conv_y.conv.bias") else 0.0) + 0.1 * torch.randn(p.shape, generator=g) / (4.0 if p.dim() > 1 else 1.0))
            elif p.dim() >= 4:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p[0].numel()) ** 0.5)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return vae.to(device=dev, dtype=torch.bfloat16).requires_grad_(False).eval(), g


def median_ms(f, warmup, runs):
    """(median, min, max) HIP-event milliseconds of f() over `runs` runs behind `warmup` untimed ones"""
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def clip_seconds(f, dev, warmup, runs):
    """wall seconds of f() (host clock around a synchronised call): the keys seconds_per_clip (median), seconds_min_max and peak_allocated_gb"""
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    secs = []
    for _ in range(runs):
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    return {"seconds_per_clip": statistics.median(secs), "seconds_min_max": [min(secs), max(secs)],
            "peak_allocated_gb": torch.cuda.max_memory_allocated(dev) / 1e9}


def kernel_entries(f):
    """one f() under ops.KernelTimer: the keys entries (per ops entry point: launches, total ms, TFLOP/s or GB/s) and conv_tflop_per_clip"""
    from videogpa_amd import ops
    ops.TIMER = ops.KernelTimer()
    try:
        f()
        torch.cuda.synchronize()
        summary = ops.TIMER.summary()
    finally:
        ops.TIMER = None
    entries = {}
    for name, s in summary.items():
        rate = s["work_per_launch"] * s["launches"] / (s["total_ms"] * 1e-3)
        entries[name] = {"launches": s["launches"], "total_ms": s["total_ms"],
                         ("tflops" if s["unit"] == "flop" else "gbytes_per_s"): rate / (1e12 if s["unit"] == "flop" else 1e9)}
    return {"entries": entries,
            "conv_tflop_per_clip": sum(s["work_per_launch"] * s["launches"] for s in summary.values() if s["unit"] == "flop") / 1e12}


def main(tool, run, print_json=True):
    """`python tools/<tool> [--quick] [--json PATH]`: run(device, quick) on cuda:0, its result as one JSON line and, with --json, as a file"""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool} measures on the GPU: no device found")
    res = run(torch.device("cuda", 0), a.quick)
    if print_json:
        print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
