"""Depth Anything 3's backbone and cameras at the replication path's scale: DA3-Large (ViT-L/14, alt_start = qknorm_start = rope_start = 8, out layers
11 / 15 / 19 / 23) on 10 frames of 504 x 504 -- N = 1297 tokens per view, global attention over 12 970 tokens, C = 1024, 16 heads.  One row per kernel of
csrc/da3.hip (ms, GB/s over its algorithmic bytes) and one for the whole DA3Cameras forward, random weights, bf16 autocast.
    python tools/da3_bench.py [--quick] [--json PATH]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def run(dev, quick=False):
    from videogpa_amd import ops
    from videogpa_amd.da3 import CameraDec, DA3Cameras, DinoV2
    n = 2 if quick else 20
    B, S, H, W, C = 1, 10, 504, 504, 1024
    N = 1 + (H // 14) * (W // 14)
    rows = {"shape": {"B": B, "S": S, "H": H, "W": W, "N": N, "C": C}}
    torch.manual_seed(0)
    with torch.no_grad():
        x, local = torch.randn(B, S, N, C, device=dev), torch.randn(B, S, N, C, device=dev)
        w, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        cam, pose = torch.randn(1, 2, C, device=dev), torch.randn(B, S, 9, device=dev)
        ref_idx = ops.da3_ref_view(x)
        slab = 4.0 * x.numel()
        for name, f, nbytes in (("da3_ref_view", lambda: ops.da3_ref_view(x), 4.0 * B * S * C),
                                ("da3_view_gather", lambda: ops.da3_view_gather(x, ref_idx), 2 * slab),
                                ("da3_cam_token", lambda: ops.da3_cam_token(x, cam, per_view=False), 8.0 * B * S * C),
                                ("da3_tap", lambda: ops.da3_tap(local, x, w, b, 1e-5, ref_idx), 4 * slab),
                                ("da3_pose_decode", lambda: ops.da3_pose_decode(pose, (H, W)), 4.0 * B * S * 30)):
            ms = _timeit(f, n)
            rows[name] = {"ms": ms, "gbs": nbytes / ms / 1e6}
            print(f"{name:16s} {ms:.4f} ms = {nbytes / ms / 1e6:.0f} GB/s over its algorithmic bytes")
        del x, local
        with torch.device(dev):
            net = DA3Cameras(DinoV2("vitl", [11, 15, 19, 23], alt_start=8, qknorm_start=8, rope_start=8, cat_token=True), CameraDec(2048)).eval()
        images = torch.randn(B, S, 3, H, W, device=dev)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ms = _timeit(lambda: net(images), max(2, n // 4))
        rows["DA3Cameras_forward"] = {"ms": ms}
        print(f"DA3Cameras forward (backbone + camera decoder), {S} x {H} x {W}: {ms:.2f} ms")
    return rows


if __name__ == "__main__":
    rows = run("cuda", quick="--quick" in sys.argv)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)
