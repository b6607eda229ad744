"""The DINOv2 patch embedding at the scorer's scale: 10 frames of 518 x 518 (the square grid of the position table) and of 294 x 518 (the scorer's crop
mode: interpolated table), ViT-L/14-reg widths.  Three rows per size -- the fused token-embed kernel alone (ms, GB/s over the bytes in + out, TFLOP/s), the
whole DinoVisionTransformer forward, VGGT end to end -- the first two next to the same computation composed from torch ops (tests/dinov2_ref.py under bf16
autocast) in the same process.  tools/scorer_bench.py calls run() for its `vggt_dinov2` block; standalone:
    python tools/dinov2_bench.py [--quick] [--no-end-to-end] [--json PATH]      # --json: also write the rows to PATH"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def run(dev, quick=False, end_to_end=True):
    import dinov2_ref
    from videogpa_amd import ops
    from videogpa_amd.vggt import VGGT, vit_large
    n = 2 if quick else 20
    rows = {}
    torch.manual_seed(0)
    with torch.no_grad():
        with torch.device(dev):
            vit = vit_large(img_size=518, patch_size=14, num_register_tokens=4, interpolate_antialias=True, interpolate_offset=0.0, block_chunks=0,
                            init_values=1.0).eval()
        sd = {k: v.detach() for k, v in vit.state_dict().items()}
        wp, bias, cls, reg = vit._embed_params()
        for H, W in ((518, 518), (294, 518)):
            tag, row = f"10x{H}x{W}", {}
            x = torch.randn(10, 3, H, W, device=dev)
            pos = vit.pos_table(H, W).detach().float().contiguous()
            P, C = (H // 14) * (W // 14), 1024
            flop = 2.0 * 10 * P * C * 588
            for name, xin, odt in (("f32_to_bf16", x, torch.bfloat16), ("bf16_to_bf16", x.to(torch.bfloat16), torch.bfloat16), ("f32_to_f32", x, torch.float32)):
                ms = _timeit(lambda: ops.dino_embed(xin, wp, bias, cls, reg, pos[0], odt), n)
                nbytes = xin.numel() * xin.element_size() + 10 * (5 + P) * C * (2 if odt == torch.bfloat16 else 4)
                row["dino_embed_" + name] = {"ms": ms, "gbs_in_plus_out": nbytes / ms / 1e6, "tflops": flop / ms / 1e9}
                print(f"dino_embed [{tag} {name:12s}] {ms:.4f} ms = {nbytes / ms / 1e6:.0f} GB/s over bytes in + out, {flop / ms / 1e9:.1f} TFLOP/s")
            with torch.autocast("cuda", dtype=torch.bfloat16):
                ms_t = _timeit(lambda: dinov2_ref.prepare_tokens(sd, x, 14, pos), n)
            ms_t32 = _timeit(lambda: dinov2_ref.prepare_tokens(sd, x, 14, pos), n)
            row["torch_ops_embed_ms_bf16_autocast"], row["torch_ops_embed_ms_fp32"] = ms_t, ms_t32
            print(f"torch ops (conv2d, transpose, cat, add, cat) [{tag}] bf16 autocast {ms_t:.4f} ms ({ms_t / row['dino_embed_f32_to_bf16']['ms']:.2f}x the kernel), "
                  f"fp32 {ms_t32:.4f} ms ({ms_t32 / row['dino_embed_f32_to_f32']['ms']:.2f}x)")
            with torch.autocast("cuda", dtype=torch.bfloat16):
                ms_k = _timeit(lambda: vit(x), max(2, n // 4))
                ms_r = _timeit(lambda: dinov2_ref.forward(sd, x, 14, 16, table=pos), max(2, n // 4))
            row["dinov2_forward_ms"], row["torch_ops_forward_ms_bf16_autocast"] = ms_k, ms_r
            print(f"DinoVisionTransformer ViT-L/14-reg [{tag}] {ms_k:.2f} ms; torch ops under bf16 autocast {ms_r:.2f} ms ({ms_r / ms_k:.2f}x)")
            rows[tag] = row
            del x
        del vit, sd
        if end_to_end:
            with torch.device(dev):
                model = VGGT().eval()
            for H, W in ((518, 518), (294, 518)):
                images = torch.rand(1, 10, 3, H, W, device=dev)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    ms = _timeit(lambda: model(images), 2 if quick else 3)
                rows[f"10x{H}x{W}"]["vggt_end_to_end_ms"] = ms
                print(f"VGGT (DINOv2 front + aggregator + camera, depth and point heads) [10x{H}x{W}] {ms:.1f} ms end to end (no torch-op twin of the whole model is built)")
    return rows


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-end-to-end", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = run(torch.device("cuda", 0), a.quick, not a.no_end_to_end)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
