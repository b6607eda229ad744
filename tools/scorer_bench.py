"""The geometry scorer at the reference's scale (10 views x 518 x 518, a cloud of 10 * 518 * 518 points: train/01_preference_pair.py:33-34, utils/projection_utils.py):
the SAME measurement bench.py attaches as its `scorer` block (bench.scorer_report: ms per video, point-views / s, algorithmic GB/s against the 8 TB/s peak, atomics / s,
the reference's argsort + scatter formulation on this GPU, the CPU oracle), plus the kernels that block does not touch (confidence cut, MVCS, 8-point + Sampson, SSIM, the VGGT heads, the DINOv2 patch embedding, LPIPS-VGG) so that
a rocprofv3 pass over this script (tools/profile_round.sh) sees every scorer kernel.
    python tools/scorer_bench.py [--quick] [--json gpurun_out/scorer_bench.json]      # --quick: two launches of everything, no timing loops (PMC passes)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from videogpa_amd import scorer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true")
ap.add_argument("--json", default=os.path.join(ROOT, "gpurun_out", "scorer_bench.json"))
a = ap.parse_args()
dev = torch.device("cuda", 0)


def timeit(f, n=10):
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        r = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, r


out = {}
if a.quick:
    for pm in (True, False):
        T, H, W, N, pc, colors, K, E, gt = bench.scorer_inputs(dev, pm)
        for _ in range(2):
            rep = scorer.batch_reproject(pc, colors, K, E, H, W)
        scorer.MSEMetric().compute_device(gt=gt, rep=rep)
else:
    out = bench.scorer_report(dev, with_cpu=True)
    for kind in ("pointmap", "random_cloud"):
        r = out[kind]
        print(f"batch_reproject [{kind:12s}] {r['ms_per_video']:.3f} ms per video  {r['gpoint_views_per_s']:.1f} Gpoint-views/s  {r['algorithmic_gbs']:.0f} GB/s algorithmic "
              f"= {r['frac_of_hbm_peak']:.3f} of 8 TB/s  {r['atomics_per_s'] / 1e9:.1f} G atomics/s  ({100 * r['pixels_covered']:.0f} % of the pixels hit)")
    r = out["pointmap"]
    print(f"frame MSE {r['mse_ms']:.3f} ms = {r['mse_gbs']:.0f} GB/s; motion score {r['motion_score_us']:.1f} us; reference formulation (torch argsort + scatter) "
          f"{r['torch_argsort_ms_same_gpu']:.1f} ms per video; CPU oracle {r.get('cpu_oracle_ms', float('nan')):.0f} ms per video")
# the kernels the bench block does not touch: confidence cut (radix select), MVCS, 8-point + Sampson
T, H, W, N, pc, colors, K, E, gt = bench.scorer_inputs(dev, True)
g = torch.Generator(device=dev).manual_seed(1)
conf = torch.rand(N, generator=g, device=dev) * 10
depth = 3.0 + 0.2 * torch.rand(T, H, W, generator=g, device=dev)
rng = np.random.default_rng(0)
p1 = [rng.random((2048, 2)).astype(np.float32) * 500 for _ in range(9)]
p2 = [p + rng.normal(size=p.shape).astype(np.float32) for p in p1]
n = 2 if a.quick else 10
ms_c, _ = timeit(lambda: scorer.confidence_threshold(conf, 50.0), n)
ms_p, _ = timeit(lambda: scorer.reproject_predictions(pc.view(T, H, W, 3), conf.view(T, H, W), colors.view(T, H, W, 3) / 255, K, E, H, W, conf_thres=50.0), n)
ms_m, _ = timeit(lambda: scorer.MVCSMetric().compute_device(depths=depth, intrinsics=K, extrinsics=E[:, :3]), n)
ms_e, _ = timeit(lambda: scorer.epipolar_errors(p1, p2), max(2, n // 2))
out["other_kernels"] = {"conf_threshold_ms": ms_c, "conf_threshold_gbs": N * 4 * 2 / ms_c / 1e6, "reproject_predictions_conf50_ms": ms_p, "mvcs_ms": ms_m,
                        "mvcs_gbs": (T - 1) * H * W * 8 / ms_m / 1e6, "epipolar_9x2048_ms_incl_host_packing": ms_e}
print(f"confidence cut (radix select over {N} values): {ms_c:.3f} ms; fused filter + reproject at conf_thres 50: {ms_p:.3f} ms; MVCS: {ms_m:.3f} ms; "
      f"8-point + Sampson, 9 pairs x 2048 matches: {ms_e:.3f} ms")

# SSIM (csrc/scorer_ssim.hip) on the reference's scorer workload, 10 frames of 518 x 518 x 3, next to the same computation composed from torch ops on this GPU in
# fp32 (piq.ssim's own formulation: avg_pool2d + five grouped 11 x 11 convolutions + elementwise); GB/s = the bytes of both inputs once over the time.
def torch_ssim(gt, rep):
    x, y = [(t.float().permute(0, 3, 1, 2) if t.shape[-1] == 3 else t.float()) for t in (gt, rep)]
    x, y = [((t + 1) / 2 if t.min() < 0 else (t / 255 if t.max() > 1 else t)) for t in (x, y)]
    f = max(1, round(min(x.shape[-2:]) / 256))
    if f > 1:
        x, y = torch.nn.functional.avg_pool2d(x, f), torch.nn.functional.avg_pool2d(y, f)
    c = torch.arange(11, dtype=torch.float32, device=x.device) - 5
    g = torch.exp(-(c[:, None] ** 2 + c[None, :] ** 2) / (2 * 1.5 ** 2))
    g = (g / g.sum()).expand(x.shape[1], 1, 11, 11).contiguous()
    conv = lambda t: torch.nn.functional.conv2d(t, g, groups=t.shape[1])
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    ss = (2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4) * (2 * sxy + 9e-4) / (sxx + syy + 9e-4)
    return ss.mean(dim=(1, 2, 3)).mean()


gs = torch.Generator(device=dev).manual_seed(2)
f_gt = torch.rand(T, 3, H, W, generator=gs, device=dev)
f_rep = (f_gt + 0.05 * torch.randn(T, 3, H, W, generator=gs, device=dev)).clamp(0, 1)
ssim_rows = {}
for form, x_gt, x_rep in (("f32_nchw", f_gt, f_rep),
                          ("u8_nhwc", (f_gt * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous(), (f_rep * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous())):
    n_s = 2 if a.quick else 200
    ms_k, v_k = timeit(lambda: scorer.ssim(x_gt, x_rep), n_s)
    ms_t, v_t = timeit(lambda: torch_ssim(x_gt, x_rep), n_s)
    nbytes = 2 * x_gt.numel() * x_gt.element_size()
    ssim_rows[form] = {"ssim_ms": ms_k, "ssim_gbs": nbytes / ms_k / 1e6, "frac_of_hbm_peak": nbytes / ms_k / 1e6 / 8000.0, "torch_ops_ms_same_gpu": ms_t,
                       "speedup_vs_torch_ops": ms_t / ms_k, "value": float(v_k), "torch_ops_value": float(v_t)}
    print(f"frame SSIM [{form:8s}] {ms_k:.4f} ms = {nbytes / ms_k / 1e6:.0f} GB/s ({nbytes / ms_k / 1e6 / 8000.0:.3f} of 8 TB/s); torch-op composition on this GPU {ms_t:.4f} ms "
          f"({ms_t / ms_k:.1f}x); values {float(v_k):.6f} / {float(v_t):.6f}")
out["ssim"] = ssim_rows

# The VGGT heads (csrc/vggt_heads.hip) at the scorer's scale, 10 frames of 518 x 518 (37 x 37 patches), VGGT-1B widths: one DPT head and the camera head, next to the
# same computation from torch ops (fp32, TF32 off) in the same process, and the convolution kernel per shape against the 157.3 TFLOP/s fp32-matrix peak.
from videogpa_amd import ops  # noqa: E402
from videogpa_amd.vggt import CameraHead, DPTHead  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vggt_heads_ref as heads_ref  # noqa: E402

torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
F32_MATRIX_PEAK = 157.3e12
n_h = 2 if a.quick else 5
heads = {"conv3x3": {}}
with torch.no_grad():
    for tag, (nf, hw_, ci, co) in {"refinenet1 256->256 @148": (10, 148, 256, 256), "output_conv1 256->128 @296": (10, 296, 256, 128), "refinenet2 256->256 @74": (10, 74, 256, 256),
                                    "layer2_rn 512->256 @74": (10, 74, 512, 256), "layer4_rn 1024->256 @19": (10, 19, 1024, 256)}.items():
        x = torch.randn(nf, hw_, hw_, ci, device=dev)
        w = torch.randn(co, ci, 3, 3, device=dev) / (9 * ci) ** 0.5
        b = torch.randn(co, device=dev)
        wp = ops.pack_conv_weight(w)
        xc = x.permute(0, 3, 1, 2)                                             # the same memory as a channels_last NCHW tensor
        ms_k, _ = timeit(lambda: ops.conv3x3_f32(x, wp, b, relu_in=True), n_h)
        ms_t, _ = timeit(lambda: torch.nn.functional.conv2d(torch.relu(xc), w, b, padding=1), n_h)
        fl = 2.0 * nf * hw_ * hw_ * 9 * ci * co
        heads["conv3x3"][tag] = {"ms": ms_k, "tflops": fl / ms_k / 1e9, "frac_of_f32_matrix_peak": fl / ms_k / 1e-3 / F32_MATRIX_PEAK, "torch_conv2d_ms_same_gpu": ms_t}
        print(f"conv3x3_f32 [{tag:28s}] {ms_k:.3f} ms = {fl / ms_k / 1e9:.1f} TFLOP/s ({fl / ms_k / 1e-3 / F32_MATRIX_PEAK:.3f} of the fp32-matrix peak); torch conv2d {ms_t:.3f} ms")
        del x, w, xc
    x = torch.randn(8, 296, 296, 128, device=dev)
    w1, b1 = torch.randn(32, 128, 3, 3, device=dev) / 34, torch.randn(32, device=dev)
    w2, b2 = torch.randn(2, 32, device=dev) * 0.2, torch.randn(2, device=dev)
    tabs, w1p = ops.uv_embed_tables(518, 518, 128, 1.0, dev), ops.pack_conv_weight(w1)
    sd_t = {"scratch.output_conv2.0.weight": w1, "scratch.output_conv2.0.bias": b1, "scratch.output_conv2.2.weight": w2.reshape(2, 32, 1, 1), "scratch.output_conv2.2.bias": b2}
    ms_k, _ = timeit(lambda: ops.dpt_tail_f32(x, 518, 518, w1p, b1, w2, b2, activation="exp", tabs=tabs), n_h)
    xc = x.permute(0, 3, 1, 2).contiguous()
    ms_t, _ = timeit(lambda: heads_ref.dpt_tail(sd_t, xc, (518, 518)), n_h)
    fl = 2.0 * 8 * 518 * 518 * 9 * 128 * 32
    heads["dpt_tail_8_frames"] = {"ms": ms_k, "tflops": fl / ms_k / 1e9, "frac_of_f32_matrix_peak": fl / ms_k / 1e-3 / F32_MATRIX_PEAK, "torch_ops_ms_same_gpu": ms_t}
    print(f"dpt_tail_f32 [8 frames, 128 -> 32 -> 2 @518] {ms_k:.3f} ms = {fl / ms_k / 1e9:.1f} TFLOP/s; torch ops (interpolate + embed + conv + conv + exp) {ms_t:.3f} ms")
    del x, xc
    torch.manual_seed(0)
    head = DPTHead(dim_in=2048, output_dim=2, activation="exp").to(dev).eval()
    toks = [torch.randn(1, 10, 5 + 37 * 37, 2048, device=dev) if i in (4, 11, 17, 23) else None for i in range(24)]
    images = torch.zeros(1, 10, 3, 518, 518, device=dev)
    sd_h = {k: v.detach() for k, v in head.state_dict().items()}
    ms_k, _ = timeit(lambda: head(toks, images, 5), n_h)
    ms_t, _ = timeit(lambda: [heads_ref.dpt_head(sd_h, [t[:, s0:s0 + 8] if t is not None else None for t in toks], (518, 518), 5, layer_idx=(4, 11, 17, 23))
                              for s0 in (0, 8)], n_h)
    heads["dpt_head_10_frames"] = {"ms": ms_k, "torch_ops_ms_same_gpu": ms_t, "speedup_vs_torch_ops": ms_t / ms_k}
    print(f"DPTHead [10 x 518 x 518, dim_in 2048, features 256, chunks of 8] {ms_k:.2f} ms; torch ops on this GPU {ms_t:.2f} ms ({ms_t / ms_k:.2f}x)")
    cam = CameraHead(dim_in=2048).to(dev).eval()
    sd_c = {k: v.detach() for k, v in cam.state_dict().items()}
    ctoks = [torch.randn(1, 10, 1, 2048, device=dev)]
    ms_k, _ = timeit(lambda: cam(ctoks), n_h)
    ms_t, _ = timeit(lambda: heads_ref.camera_head(sd_c, ctoks, 16, 4), n_h)
    heads["camera_head_10_frames"] = {"ms": ms_k, "torch_ops_ms_same_gpu": ms_t}
    print(f"CameraHead [10 frames, dim 2048, 4 blocks, 4 iterations] {ms_k:.3f} ms; torch ops on this GPU {ms_t:.3f} ms")
out["vggt_heads"] = heads

# The DINOv2 patch embedding (csrc/dino_embed.hip, vggt.DinoVisionTransformer) and VGGT end to end at the same scale: tools/dinov2_bench.py
import dinov2_bench  # noqa: E402
out["vggt_dinov2"] = dinov2_bench.run(dev, a.quick)

# LPIPS-VGG (csrc/lpips.hip, videogpa_amd.lpips.LPIPS) at 10 + 10 frames of 518 x 518, per convolution shape and per layer kernel: tools/lpips_bench.py
import lpips_bench  # noqa: E402
out["lpips"] = lpips_bench.run(dev, a.quick)
if not a.quick:
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
