"""The offline video encode of 02_encode.py (videogpa_amd.vae.AutoencoderKLCogVideoX on a clip) at its own size: ONE 49 x 480 x 720 clip through the
5B encoder (128,256,256,512 x 3 layers, seeded random weights, bfloat16 module), slicing and tiling on as 02_encode.py sets them,
`vae.encode(v.to(vae.dtype)).latent_dist.sample()`.  Prints ONE JSON line:
    seconds_per_clip      wall seconds (host clock around a synchronised call), the median of the timed runs
    entries               per ops entry point over one encode under ops.KernelTimer: launches, total ms, TFLOP/s (GB/s for the byte-bound ones)
    shapes                in the same process, for the convolution shapes that carry most of the clip's FLOPs: ops.conv3d_causal_f32 at (N,T,H,W,Cin,Cout)
                          as the encode calls it, and ops.conv3x3_pad_f32 (the 2-D chunked kernel) at the same (Cin,Cout,H,W) over N * T frames, so the same
                          M; median HIP-event ms, TFLOP/s of each, and their ratio (expected >= 0.9: the same core with a longer K loop)
    python tools/vae_encode_bench.py [--quick] [--json PATH]"""
import torch

from vae_bench_common import clip_seconds, kernel_entries, main, median_ms, seeded_vae


def run(dev, quick=False, frames=49, height=480, width=720, top=8):
    from videogpa_amd import ops
    vae, g = seeded_vae(dev)
    vae.enable_slicing()
    vae.enable_tiling()
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
        out.update(clip_seconds(encode, dev, warmup - 1, runs))
        out.update(kernel_entries(encode))
        # the 3-D kernel against the 2-D chunked one at the same widths and the same M, heaviest shapes first
        flop = lambda k: 2.0 * k[0] * k[1] * k[2] * k[3] * k[5] * 27 * k[4]
        out["shapes"] = []
        for key in sorted(calls, key=lambda k: -flop(k) * calls[k])[:top]:
            N, T, H, W, Cin, Cout = key
            x = torch.randn(N, T, H, W, Cin, device=dev)
            w3, w2, b = torch.randn(3, 3, 3, Cin, Cout, device=dev) * 0.02, torch.randn(3, 3, Cin, Cout, device=dev) * 0.02, torch.zeros(Cout, device=dev)
            ms3 = median_ms(lambda: ops.conv3d_causal_f32(x, w3, b), 2, shape_runs)[0]
            x2 = x.view(N * T, H, W, Cin)
            ms2 = median_ms(lambda: ops.conv3x3_pad_f32(x2, w2, b), 2, shape_runs)[0]
            tf3, tf2 = flop(key) / ms3 / 1e9, flop(key) / 3 / ms2 / 1e9
            out["shapes"].append({"N": N, "T": T, "H": H, "W": W, "Cin": Cin, "Cout": Cout, "calls_per_clip": calls[key],
                                  "share_of_conv3d_flop": flop(key) * calls[key] / sum(flop(k) * c for k, c in calls.items()),
                                  "conv3d_ms": ms3, "conv3d_tflops": tf3, "conv2d_ms": ms2, "conv2d_tflops": tf2, "ratio_3d_over_2d": tf3 / tf2})
            del x, x2, w3, w2
    return out


if __name__ == "__main__":
    main("vae_encode_bench.py", run)
