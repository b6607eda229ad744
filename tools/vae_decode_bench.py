"""The decode at the end of the reference's generate scripts (videogpa_amd.vae.AutoencoderKLCogVideoX with_decoder=True) at its own size: ONE
[1,16,13,60,90] latent -> 49 x 480 x 720 frames through the 5B decoder (512,256,256,128 x 4 resnets, seeded random weights, bfloat16 module), slicing
and tiling on as generate/CogVideoX-5B.py sets them, through generate.decode_latents.  Prints ONE JSON line:
    seconds_per_clip      wall seconds (host clock around a synchronised call), the median of the timed runs
    entries               per ops entry point over one decode under ops.KernelTimer: launches, total ms, TFLOP/s (GB/s for the byte-bound ones)
    upsamplers            in the same process, for the three up-sampler shapes of a full tile batch: ops.vae_upsample_f32 at (N,T,H,W,C,compress_time)
                          as the decode calls it, and ops.conv3x3_pad_f32 on an already up-sampled [N * T',2H,2W,C] map, so the same output M; median
                          HIP-event ms, TFLOP/s of each, and their ratio (the loader reads a quarter of the rows the plain convolution reads)
    python tools/vae_decode_bench.py [--quick] [--json PATH]"""
import torch

from vae_bench_common import clip_seconds, kernel_entries, main, median_ms, seeded_vae


def run(dev, quick=False, latent_frames=13, height=60, width=90):
    from videogpa_amd import generate, ops
    vae, g = seeded_vae(dev, with_decoder=True)
    vae.enable_slicing()
    vae.enable_tiling()
    warmup, runs, shape_runs = (1, 1, 3) if quick else (1, 3, 7)
    latents = (0.7 * torch.randn(1, latent_frames, 16, height, width, generator=g)).to(device=dev, dtype=vae.dtype)
    decode = lambda: generate.decode_latents(vae, latents)
    out = {"latent_frames": latent_frames, "latent_height": height, "latent_width": width, "warmup": warmup, "runs": runs,
           "device": torch.cuda.get_device_name(dev), "latent_frame_batches": vae.latent_frame_batches(latent_frames),
           "tile_plan": vae.decode_tile_plan(height, width)}
    with torch.no_grad():
        # the shapes the up-sampler is called at, counted over one decode (which is also the warm-up)
        calls, real = {}, ops.vae_upsample_f32

        def counting(x, w_packed, bias=None, compress_time=True):
            key = tuple(x.shape) + (bool(compress_time),)
            calls[key] = calls.get(key, 0) + 1
            return real(x, w_packed, bias, compress_time=compress_time)
        ops.vae_upsample_f32 = counting
        try:
            frames = decode()
        finally:
            ops.vae_upsample_f32 = real
        out["frames_shape"] = list(frames.shape)
        out["frames_finite"] = bool(torch.isfinite(frames.float()).all())
        del frames
        out.update(clip_seconds(decode, dev, warmup - 1, runs))
        out.update(kernel_entries(decode))
        # the up-sampler against the plain chunked convolution at the same output M: the largest call of each of the three up-sampling blocks
        out["upsamplers"] = []
        by_width = {}
        for key in calls:
            k = (key[4], key[5])
            if k not in by_width or key[0] * key[1] * key[2] * key[3] > by_width[k][0] * by_width[k][1] * by_width[k][2] * by_width[k][3]:
                by_width[k] = key
        for key in sorted(by_width.values(), key=lambda k: k[2]):
            N, T, H, W, C, ct = key
            To = ops.vae_upsample_frames(T, ct)
            x, w, b = torch.randn(N, T, H, W, C, device=dev), torch.randn(3, 3, C, C, device=dev) * 0.02, torch.zeros(C, device=dev)
            ms_up = median_ms(lambda: ops.vae_upsample_f32(x, w, b, compress_time=ct), 2, shape_runs)[0]
            x2 = torch.randn(N * To, 2 * H, 2 * W, C, device=dev)
            ms_2d = median_ms(lambda: ops.conv3x3_pad_f32(x2, w, b), 2, shape_runs)[0]
            flop = 2.0 * N * To * 4 * H * W * 9 * C * C
            out["upsamplers"].append({"N": N, "T": T, "T_out": To, "H": H, "W": W, "C": C, "compress_time": ct,
                                      "calls_per_clip": sum(c for k, c in calls.items() if (k[4], k[5]) == (C, ct)),
                                      "upsample_ms": ms_up, "upsample_tflops": flop / ms_up / 1e9, "conv2d_ms": ms_2d, "conv2d_tflops": flop / ms_2d / 1e9,
                                      "ratio_upsample_over_conv2d": ms_2d / ms_up})
            del x, x2, w
    return out


if __name__ == "__main__":
    main("vae_decode_bench.py", run)
