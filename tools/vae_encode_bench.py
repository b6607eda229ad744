"""The offline video encode of 02_encode.py (videogpa_amd.vae.AutoencoderKLCogVideoX on a clip) at its own size: ONE 49 x 480 x 720 clip through the
5B encoder (128,256,256,512 x 3 layers, seeded random weights, bfloat16 module), slicing and tiling on as 02_encode.py sets them,
`vae.encode(v.to(vae.dtype)).latent_dist.sample()`.  Prints ONE JSON line:
    seconds_per_clip      wall seconds (host clock around a synchronised call), the median of the timed runs
    entries               per ops entry point over one encode under ops.KernelTimer: launches, total ms, TFLOP/s (GB/s for the byte-bound ones)
    shapes                in the same process, for the convolution shapes that carry most of the clip's FLOPs: ops.conv3d_causal_f32 at (N,T,H,W,Cin,Cout)
                          as the encode calls it, and ops.conv3x3_pad_f32 (the 2-D chunked kernel) at the same (Cin,Cout,H,W) over N * T frames, so the same
                          M; median HIP-event ms, TFLOP/s of each, and their ratio (expected >= 0.9: the same core with a longer K loop)
    python tools/vae_encode_bench.py [--quick] [--json PATH]"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(f, warmup, runs):
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
    return statistics.median(ms)


def _seeded_vae(dev):
    from videogpa_amd.vae import AutoencoderKLCogVideoX
    g = torch.Generator().manual_seed(0)
    vae = AutoencoderKLCogVideoX()
    with torch.no_grad():
        for name, p in vae.named_parameters():          # O(1) activations: He-scaled convolutions, GroupNorm near identity
            if p.dim() >= 4:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p[0].numel()) ** 0.5)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    vae = vae.to(device=dev, dtype=torch.bfloat16).requires_grad_(False).eval()
    vae.enable_slicing()
    vae.enable_tiling()
    return vae, g


def run(dev, quick=False, frames=49, height=480, width=720, top=8):
    from videogpa_amd import ops
    vae, g = _seeded_vae(dev)
    warmup, runs, shape_runs = (1, 1, 3) if quick else (1, 3, 7)
    v = (torch.rand(1, 3, frames, height, width, generator=g) * 2 - 1).to(dev)
    encode = lambda: vae.encode(v.to(vae.dtype)).latent_dist.sample()
    out = {"frames": frames, "height": height, "width": width, "warmup": warmup, "runs": runs, "frame_batches": vae.frame_batches(frames)}
    with torch.no_grad():
        # the shapes the causal convolution is called at, counted over one encode (which is also the warm-up)
        calls, real = {}, ops.conv3d_causal_f32

        def counting(x, w_packed, *a, **kw):
            key = tuple(x.shape) + (w_packed.shape[-1],)
            calls[key] = calls.get(key, 0) + 1
            return real(x, w_packed, *a, **kw)
        ops.conv3d_causal_f32 = counting
        try:
            z = encode()
        finally:
            ops.conv3d_causal_f32 = real
        out["latent_shape"] = list(z.shape)
        for _ in range(warmup - 1):
            encode()
        torch.cuda.synchronize()
        secs = []
        for _ in range(runs):
            torch.cuda.reset_peak_memory_stats(dev)
            t0 = time.perf_counter()
            encode()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        out["seconds_per_clip"] = statistics.median(secs)
        out["seconds_min_max"] = [min(secs), max(secs)]
        out["peak_allocated_gb"] = torch.cuda.max_memory_allocated(dev) / 1e9
        ops.TIMER = ops.KernelTimer()
        try:
            encode()
            torch.cuda.synchronize()
            summary = ops.TIMER.summary()
        finally:
            ops.TIMER = None
        out["entries"] = {}
        for name, s in summary.items():
            rate = s["work_per_launch"] * s["launches"] / (s["total_ms"] * 1e-3)
            out["entries"][name] = {"launches": s["launches"], "total_ms": s["total_ms"],
                                    ("tflops" if s["unit"] == "flop" else "gbytes_per_s"): rate / (1e12 if s["unit"] == "flop" else 1e9)}
        out["conv_tflop_per_clip"] = sum(s["work_per_launch"] * s["launches"] for s in summary.values() if s["unit"] == "flop") / 1e12
        # the 3-D kernel against the 2-D chunked one at the same widths and the same M, heaviest shapes first
        flop = lambda k: 2.0 * k[0] * k[1] * k[2] * k[3] * k[5] * 27 * k[4]
        out["shapes"] = []
        for key in sorted(calls, key=lambda k: -flop(k) * calls[k])[:top]:
            N, T, H, W, Cin, Cout = key
            x = torch.randn(N, T, H, W, Cin, device=dev)
            w3, w2, b = torch.randn(3, 3, 3, Cin, Cout, device=dev) * 0.02, torch.randn(3, 3, Cin, Cout, device=dev) * 0.02, torch.zeros(Cout, device=dev)
            ms3 = _median_ms(lambda: ops.conv3d_causal_f32(x, w3, b), 2, shape_runs)
            x2 = x.view(N * T, H, W, Cin)
            ms2 = _median_ms(lambda: ops.conv3x3_pad_f32(x2, w2, b), 2, shape_runs)
            tf3, tf2 = flop(key) / ms3 / 1e9, flop(key) / 3 / ms2 / 1e9
            out["shapes"].append({"N": N, "T": T, "H": H, "W": W, "Cin": Cin, "Cout": Cout, "calls_per_clip": calls[key],
                                  "share_of_conv3d_flop": flop(key) * calls[key] / sum(flop(k) * c for k, c in calls.items()),
                                  "conv3d_ms": ms3, "conv3d_tflops": tf3, "conv2d_ms": ms2, "conv2d_tflops": tf2, "ratio_3d_over_2d": tf3 / tf2})
            del x, x2, w3, w2
    return out


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vae_encode_bench.py measures on the GPU: no device found")
    res = run(torch.device("cuda", 0), a.quick)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
