"""The I2V conditioning encode (videogpa_amd.vae.AutoencoderKLCogVideoX, csrc/vae.hip) at the trainer's size: one 480 x 720 frame per sample through
the 5B-I2V encoder (128,256,256,512 x 3 layers, seeded random weights, bfloat16 module as the reference builds it), `encode(x).latent_dist.sample()`.
Rows: untiled and tiled (diffusers' 3 x 3 tiled_encode grid) at B = 1 and 2 with slicing off; HIP-event milliseconds per encode, 5 warm-up runs, the
median of 20 timed runs.  Each row is split with ops.KernelTimer (event pairs around every launch, in runs of their own) into the convolutions, the
GroupNorm passes (statistics + apply) and the rest = the untimed median minus those two: the layout and sampling kernels, torch's tile crops, blends
and concatenations, and the gaps between launches.  TFLOP/s is over the algorithmic FLOPs of the convolutions (true Cin = 3 for the stem).
    python tools/vae_bench.py [--quick] [--json PATH]"""
import torch

from vae_bench_common import main, median_ms, seeded_vae

F32_MATRIX_PEAK = 157.3e12
CFG3_STEP_S = 4.39          # BASELINE configs[2], the I2V training step this encode is part of


def conv_flops(vae, B, H, W):
    """algorithmic FLOPs of one untiled encode: 2 * outputs * taps * Cin per convolution"""
    cfg = vae.config
    chans, fl, c, h, w = cfg.block_out_channels, 0.0, cfg.block_out_channels[0], H, W
    fl += 2.0 * h * w * 9 * 3 * c
    for i, co in enumerate(chans):
        for j in range(cfg.layers_per_block):
            ci = c if j == 0 else co
            fl += 2.0 * h * w * 9 * (ci * co + co * co) + (2.0 * h * w * ci * co if ci != co else 0.0)
        c = co
        if i < len(chans) - 1:
            h, w = (h - 2) // 2 + 1, (w - 2) // 2 + 1
            fl += 2.0 * h * w * 9 * c * c
    fl += 2 * 2 * 2.0 * h * w * 9 * c * c + 2.0 * h * w * 9 * c * 2 * cfg.latent_channels
    return B * fl


def run(dev, quick=False, height=480, width=720):
    from videogpa_amd import ops
    warmup, runs, split_runs = (2, 5, 2) if quick else (5, 20, 3)
    vae, g = seeded_vae(dev)
    rows = {"height": height, "width": width, "warmup": warmup, "runs": runs, "cfg3_step_s": CFG3_STEP_S, "cases": {}}
    with torch.no_grad():
        for tiled in (False, True):
            (vae.enable_tiling if tiled else vae.disable_tiling)()
            for B in (1, 2):
                x = (torch.rand(B, 3, 1, height, width, generator=g) * 2 - 1).to(device=dev, dtype=torch.bfloat16)
                f = lambda: vae.encode(x).latent_dist.sample()
                torch.cuda.reset_peak_memory_stats(dev)
                med, lo, hi = median_ms(f, warmup, runs)
                peak_gb = torch.cuda.max_memory_allocated(dev) / 1e9
                ops.TIMER = ops.KernelTimer()
                try:
                    for _ in range(split_runs):
                        f()
                    torch.cuda.synchronize()
                    per = {k: v["total_ms"] / split_runs for k, v in ops.TIMER.summary().items()}
                    launches = sum(v["launches"] for v in ops.TIMER.summary().values()) // split_runs
                finally:
                    ops.TIMER = None
                conv = sum(v for k, v in per.items() if k.startswith("conv"))
                norm = sum(v for k, v in per.items() if k.startswith("groupnorm"))
                fl = conv_flops(vae, B, height, width)             # the tiled encode computes its overlaps on top of this
                tag = f"{'tiled' if tiled else 'untiled'}_b{B}"
                rows["cases"][tag] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "conv_ms": conv, "norm_ms": norm, "rest_ms": med - conv - norm,
                                      "kernel_launches": launches, "peak_allocated_gb": peak_gb, "per_kernel_ms": per, "untiled_conv_gflop": fl / 1e9,
                                      "conv_tflops": fl / conv / 1e9 if not tiled else None,
                                      "share_of_cfg3_step": med / 1e3 / CFG3_STEP_S}
                print(f"vae encode [{tag:10s} {height} x {width}] {med:8.2f} ms (min {lo:.2f}, max {hi:.2f}) = convolutions {conv:.2f} + norm passes {norm:.2f} "
                      f"+ rest {med - conv - norm:.2f}; {launches} kernel launches; peak {peak_gb:.2f} GB allocated; "
                      + (f"convolutions at {fl / conv / 1e9:.1f} TFLOP/s ({fl / conv / 1e-3 / F32_MATRIX_PEAK:.3f} of the fp32-matrix peak); " if not tiled else "")
                      + f"{100 * med / 1e3 / CFG3_STEP_S:.2f} % of cfg3's {CFG3_STEP_S} s step")
                del x
    return rows


if __name__ == "__main__":
    main("vae_bench.py", run, print_json=False)             # the rows are printed as they are measured
