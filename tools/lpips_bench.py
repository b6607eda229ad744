"""LPIPS-VGG (videogpa_amd.lpips.LPIPS, csrc/lpips.hip) at the scorer's scale: one video = 10 gt + 10 rep frames of 518 x 518, seeded random weights.
Rows: the whole call (ms per video, TFLOP/s on algorithmic FLOPs -- true Cin = 3 for conv1_1 -- against the 157.3 TFLOP/s fp32-matrix peak), each of the
13 convolution shapes at 20 frames, the five layer-kernel calls and the four pools (GB/s on algorithmic bytes against 8 TB/s), each next to the same
computation from F.conv2d / F.max_pool2d / elementwise torch ops in fp32 with TF32 off in the same process (tests/lpips_ref.py on the GPU).
tools/scorer_bench.py calls run() for its `lpips` block; standalone:
    python tools/lpips_bench.py [--quick] [--json PATH]"""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32_MATRIX_PEAK = 157.3e12
HBM_PEAK_GBS = 8000.0


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


def run(dev, quick=False, frames=10, size=518):
    import lpips_ref
    from videogpa_amd import ops
    from videogpa_amd.lpips import CHNS, LPIPS, SLICES
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    n = 2 if quick else 5
    rows = {"convs": {}, "layers": {}, "pools": {}}
    net = LPIPS(net="vgg", pretrained=False, pnet_rand=True).to(dev)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    g = torch.Generator(device=dev).manual_seed(3)
    gt = torch.rand(frames, 3, size, size, generator=g, device=dev) * 2 - 1
    rep = (gt + 0.3 * torch.randn(frames, 3, size, size, generator=g, device=dev)).clamp(-1, 1)
    with torch.no_grad():
        # the 13 convolution shapes, 2 * frames frames each, and the FLOP count of the call
        shapes, hw, cin, flops = [], size, 3, 0.0
        for k, (idx, cout) in enumerate(zip(SLICES, CHNS)):
            for j, i in enumerate(idx):
                shapes.append((f"conv{k + 1}_{j + 1}", hw, cin, cout, j > 0))
                flops += 2.0 * 2 * frames * hw * hw * 9 * cin * cout
                cin = cout
            hw //= 2
        ms_k = _timeit(lambda: net(gt, rep), n)
        ms_t = _timeit(lambda: lpips_ref.lpips(sd, gt, rep, torch.float32), n)
        v_k, v_t = net(gt, rep).reshape(-1), lpips_ref.lpips(sd, gt, rep, torch.float32)[0]
        rows["video"] = {"frames": 2 * frames, "size": size, "ms_per_video": ms_k, "gflop_per_video": flops / 1e9, "tflops": flops / ms_k / 1e9,
                         "frac_of_f32_matrix_peak": flops / ms_k / 1e-3 / F32_MATRIX_PEAK, "torch_ops_ms_same_gpu": ms_t, "speedup_vs_torch_ops": ms_t / ms_k,
                         "mean_value": float(v_k.mean()), "torch_ops_mean_value": float(v_t.mean())}
        print(f"LPIPS-VGG [{frames} + {frames} frames of {size} x {size}] {ms_k:.2f} ms per video = {flops / ms_k / 1e9:.1f} TFLOP/s "
              f"({flops / ms_k / 1e-3 / F32_MATRIX_PEAK:.3f} of the fp32-matrix peak, {flops / 1e12:.2f} TFLOP); torch ops on this GPU {ms_t:.2f} ms ({ms_t / ms_k:.2f}x); "
              f"mean values {float(v_k.mean()):.6f} / {float(v_t.mean()):.6f}")
        for tag, hw, cin, cout, relu_in in shapes:
            cpad = max(cin, 16)
            x = torch.randn(2 * frames, hw, hw, cpad, device=dev)
            x[..., cin:] = 0
            w = torch.randn(cout, cin, 3, 3, device=dev) * (2.0 / (9 * cin)) ** 0.5
            b = torch.randn(cout, device=dev)
            wp = ops.pack_conv_weight(w)
            if cin < cpad:
                wp = torch.cat([wp, wp.new_zeros(3, 3, cpad - cin, cout)], dim=2).contiguous()
            xc = x[..., :cin].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
            ms_k = _timeit(lambda: ops.conv3x3_f32(x, wp, b, relu_in=relu_in), n)
            ms_t = _timeit(lambda: F.conv2d(torch.relu(xc) if relu_in else xc, w, b, padding=1), n)
            fl = 2.0 * 2 * frames * hw * hw * 9 * cin * cout
            rows["convs"][tag] = {"hw": hw, "cin": cin, "cout": cout, "ms": ms_k, "tflops": fl / ms_k / 1e9, "frac_of_f32_matrix_peak": fl / ms_k / 1e-3 / F32_MATRIX_PEAK,
                                  "torch_conv2d_ms_same_gpu": ms_t, "slower_than_torch": bool(ms_k > ms_t)}
            print(f"conv3x3_f32 [{tag:8s} {cin:3d} -> {cout:3d} @{hw:3d}] {ms_k:.3f} ms = {fl / ms_k / 1e9:6.1f} TFLOP/s ({fl / ms_k / 1e-3 / F32_MATRIX_PEAK:.3f} of peak); "
                  f"torch conv2d {ms_t:.3f} ms{'   <- slower than torch' if ms_k > ms_t else ''}")
            del x, xc, w, wp
        hw = size
        for k, c in enumerate(CHNS):
            f0, f1 = torch.randn(frames, hw, hw, c, device=dev), torch.randn(frames, hw, hw, c, device=dev)
            w = 0.01 * torch.rand(c, device=dev)
            c0, c1, w4 = f0.permute(0, 3, 1, 2), f1.permute(0, 3, 1, 2), w.view(1, c, 1, 1)
            ms_k = _timeit(lambda: ops.lpips_layer_f32(f0, f1, w, relu=True), n)
            ms_t = _timeit(lambda: lpips_ref.layer(F.relu(c0), F.relu(c1), w4), n)
            nbytes = 2.0 * f0.numel() * 4
            rows["layers"][f"layer{k + 1}"] = {"hw": hw, "c": c, "ms": ms_k, "gbs": nbytes / ms_k / 1e6, "frac_of_hbm_peak": nbytes / ms_k / 1e6 / HBM_PEAK_GBS,
                                               "torch_ops_ms_same_gpu": ms_t}
            print(f"lpips_layer_f32 [layer{k + 1} C {c:3d} @{hw:3d}] {ms_k:.3f} ms = {nbytes / ms_k / 1e6:.0f} GB/s ({nbytes / ms_k / 1e6 / HBM_PEAK_GBS:.3f} of 8 TB/s); "
                  f"torch ops {ms_t:.3f} ms")
            if k + 1 < len(CHNS):
                x = torch.cat([f0, f1])
                xc = x.permute(0, 3, 1, 2)
                ms_k = _timeit(lambda: ops.maxpool2x2_f32(x, relu=True), n)
                ms_t = _timeit(lambda: F.max_pool2d(F.relu(xc), 2, 2), n)
                nbytes = 4.0 * (2 * (hw // 2)) ** 2 * 2 * frames * c * 1.25
                rows["pools"][f"pool{k + 1}"] = {"hw": hw, "c": c, "ms": ms_k, "gbs": nbytes / ms_k / 1e6, "frac_of_hbm_peak": nbytes / ms_k / 1e6 / HBM_PEAK_GBS,
                                                 "torch_ops_ms_same_gpu": ms_t}
                print(f"maxpool2x2_f32  [pool{k + 1}  C {c:3d} @{hw:3d}] {ms_k:.3f} ms = {nbytes / ms_k / 1e6:.0f} GB/s ({nbytes / ms_k / 1e6 / HBM_PEAK_GBS:.3f} of 8 TB/s); "
                      f"torch ops {ms_t:.3f} ms")
                del x, xc
            del f0, f1, c0, c1
            hw //= 2
    return rows


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = run(torch.device("cuda", 0), a.quick)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
