"""Depth Anything 3's DualDPT head and the whole network at the replication path's scale: DA3-Large (dim_in 2048, features 256, channels 256 / 512 /
1024 / 1024) on 10 frames of 504 x 504 -- a 36 x 36 patch grid, fusion maps up to 288 x 288 x 256, outputs at 504 x 504 -- with chunk_size = 8 and random
weights.  One row each (ms over device events, peak allocated memory above what was resident before the call) for the auxiliary tail kernel of
csrc/dualdpt.hip at the head's own shape (also TFLOP/s over its algorithmic operations), the head with aux=True, the head with aux=False, and the whole
DepthAnything3Net forward under bf16 autocast with aux=False, as the scorer calls it.
    python tools/da3_head_bench.py [--quick] [--json PATH]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timeit(f, n):
    """-> (ms per call, peak bytes allocated during the calls above the resident set)"""
    f()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, torch.cuda.max_memory_allocated() - base


def run(dev, quick=False):
    from videogpa_amd import ops
    from videogpa_amd.da3 import DepthAnything3Net
    n = 2 if quick else 10
    B, S, H, W, chunk = 1, 10, 504, 504, 8
    ph, pw = H // 14, W // 14
    rows = {"shape": {"B": B, "S": S, "H": H, "W": W, "patch_grid": [ph, pw], "chunk_size": chunk}}
    torch.manual_seed(0)
    with torch.no_grad():
        with torch.device(dev):
            net = DepthAnything3Net.from_preset("da3-large").eval()
        head = net.head
        C = head.scratch.output_conv1.out_channels
        sc = head.scratch.output_conv2_aux[3]
        a = torch.randn(chunk, 8 * ph, 8 * pw, C, device=dev)
        w1 = ops.pack_conv_weight(sc[0].weight)
        args = (w1, sc[0].bias.float(), sc[2].weight.float(), sc[2].bias.float(), sc[2].eps, sc[5].weight.float().reshape(7, 32).contiguous(), sc[5].bias.float())
        tabs = ops.uv_embed_tables(8 * pw, 8 * ph, C, W / H, dev, f32_angles=True)
        ms, peak = _timeit(lambda: ops.dualdpt_aux_tail_f32(a, *args, tabs=tabs), 2 * n)
        flop = 2.0 * a.shape[0] * a.shape[1] * a.shape[2] * (9 * C * 32 + 32 * 7)
        rows["dualdpt_aux_tail_f32"] = {"ms": ms, "tflops": flop / ms / 1e9, "peak_mb": peak / 2 ** 20, "shape": list(a.shape)}
        print(f"dualdpt_aux_tail_f32 {list(a.shape)}: {ms:.3f} ms = {flop / ms / 1e9:.1f} TFLOP/s (exact fp32), peak +{peak / 2 ** 20:.0f} MB")
        del a
        feats = [(torch.randn(B, S, ph * pw, 2048, device=dev), None) for _ in range(4)]
        for name, aux in (("DualDPT_aux", True), ("DualDPT_main_only", False)):
            ms, peak = _timeit(lambda: head(feats, H, W, patch_start_idx=0, chunk_size=chunk, aux=aux), n)
            rows[name] = {"ms": ms, "peak_mb": peak / 2 ** 20}
            print(f"DualDPT head aux={aux}, {S} x {H} x {W}, chunk_size {chunk}: {ms:.2f} ms, peak +{peak / 2 ** 20:.0f} MB")
        del feats
        images = torch.randn(B, S, 3, H, W, device=dev)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ms, peak = _timeit(lambda: net(images, aux=False), max(2, n // 2))
        rows["DepthAnything3Net_forward"] = {"ms": ms, "peak_mb": peak / 2 ** 20}
        print(f"DepthAnything3Net forward (backbone + head aux=False + cameras), bf16 autocast, {S} x {H} x {W}: {ms:.2f} ms, peak +{peak / 2 ** 20:.0f} MB")
    return rows


if __name__ == "__main__":
    rows = run("cuda", quick="--quick" in sys.argv)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)
