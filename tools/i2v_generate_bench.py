"""One image-to-video generation of the reference's replication run (replicate.py:160-240, generate/CogVideoX-5B-I2V.py) at its own size on seeded random
weights: CogVideoX-5B-I2V transformer (42 layers, 32 channels in), T5-XXL encoder, the 5B VAE with slicing and tiling, DDIM, 50 steps, guidance 6, a
720 x 1080 uint8 image -> 49 frames of 480 x 720 through videogpa_amd.generate.  Prints ONE JSON line (and writes it with --json):
    stages_seconds        wall seconds (host clock around a synchronised call) of preprocess / prompt / image encode / loop / decode of ONE generation
    loop_ab               the denoising loop alone at --ab-steps steps, fused sampler step (A) against the same loop on torch ops (B), alternated A B A B ...
                          in this one process: seconds per run of each, ms per step, and the spread of each side over the rounds
    glue_ab               what the two loops differ in, without the transformer: one ops.sampler_step against the torch ops it replaces (float(), chunk,
                          guidance, fp64 scheduler.step, the cast, the two cats of the next input), HIP-event ms per step at the full latent size, alternated.
                          The torch side includes the host synchronisation of `int(timestep)` on a device tensor, as the loop has it
    bytes_per_step        HBM bytes of the fused pass and of the unfused sequence, counted from the shapes
    python tools/i2v_generate_bench.py [--quick] [--json PATH] [--steps N] [--ab-steps N] [--ab-rounds N]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from vae_bench_common import median_ms, seeded_vae  # noqa: E402


def _timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def step_bytes(B, F, C, C_img, h, w, guided, latent_bytes=2):
    """HBM bytes per step behind the transformer, from the shapes.  fused: one pass of csrc/sampler.hip.  unfused: every torch op of the loop body reads its
    operands and writes its result (float(), v_c - v_u, g * (), v_u + (), the fp64 scheduler.step on upcast copies, two casts, and the two cats)."""
    n, ni, G = B * F * C * h * w, B * F * C_img * h * w, 2 if guided else 1
    e = latent_bytes
    fused = G * n * e + n * e + ni * e + n * e + 4 * n + G * (n + ni) * e            # read v, x, image; write x_next, x0 (fp32), packed
    un = G * n * (e + 4)                                                             # v.float()
    if guided:
        un += 3 * 12 * n                                                             # sub, mul, add in fp32: two reads and a write each
    un += (e + 8) * n + (4 + 8) * n                                                  # x and v to fp64
    un += 4 * 24 * n + 2 * 24 * n                                                    # x0 = sa x - sb v (3 ops, the scalar products included: 4), prev = a x + b x0
    un += 2 * (8 + e) * n                                                            # prev and x0 back to the latent dtype
    un += G * n * 2 * e + G * ni * 2 * e + G * (n + ni) * 2 * e                      # cat([latents] * G), cat([image] * G), cat(dim=2)
    return {"fused": fused, "unfused": un, "ratio": un / fused}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2 layers, 4 steps: a rehearsal of the tool, not a measurement")
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--ab-steps", type=int, default=10)
    ap.add_argument("--ab-rounds", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("i2v_generate_bench.py measures on the GPU: no device found")
    import bench
    import t5_ref
    from videogpa_amd import generate, ops, t5
    from videogpa_amd import transformer as vtr
    from videogpa_amd.scheduler import CogVideoXDDIMScheduler
    dev = torch.device("cuda", 0)
    steps, ab_steps = (4, 2) if a.quick else (a.steps, a.ab_steps)
    cfg_kw = dict(vtr.COGVIDEOX_5B_I2V, num_layers=2) if a.quick else dict(vtr.COGVIDEOX_5B_I2V)
    model = bench.build_model(cfg_kw, dev, seed=0).requires_grad_(False).eval()
    tcfg = t5_ref.make_cfg(vocab_size=32128, d_model=4096, d_ff=10240, num_layers=2 if a.quick else 24, num_heads=64)
    with torch.device("meta"):
        enc = t5.T5EncoderModel(tcfg)
    enc.load_state_dict(dict(t5_ref.seeded_state_dict(tcfg, seed=0, device="cuda")), strict=True, assign=True)
    enc.encoder.embed_tokens.weight = enc.shared.weight
    vae, g = seeded_vae(dev, with_decoder=True)
    vae.enable_slicing()
    vae.enable_tiling()
    image = torch.randint(0, 256, (720, 1080, 3), generator=g, dtype=torch.uint8).to(dev)
    ids = torch.randint(0, tcfg["vocab_size"], (2, 226), generator=g).to(dev)
    sch = CogVideoXDDIMScheduler()
    gen = lambda: torch.Generator(device=dev).manual_seed(42)
    cfg = model.config
    out = {"device": torch.cuda.get_device_name(dev), "quick": a.quick, "steps": steps, "guidance_scale": 6.0, "num_frames": 49,
           "transformer_layers": cfg.num_layers, "scheduler": "CogVideoXDDIMScheduler"}
    with torch.no_grad():
        # ---- one generation, stage by stage (the same calls generate.image_to_video makes), behind one short warm-up of every stage's kernels
        generate.image_to_video(model, vae, sch, enc, image, ids[:1], ids[1:], num_frames=49, num_inference_steps=1, generator=gen())
        torch.cuda.reset_peak_memory_stats(dev)
        st, rng = {}, gen()
        img, st["preprocess"] = _timed(lambda: generate.preprocess_image(image, 480, 720, dtype=torch.bfloat16, pre_resize=(1080, 720)))
        (pos, neg), st["prompt"] = _timed(lambda: generate.encode_prompt(enc, ids[:1], ids[1:]))
        il, st["image_encode"] = _timed(lambda: generate.prepare_image_latents(vae, img, 13, rng).to(pos.dtype))
        lat0 = torch.randn((1, 13, 16, 60, 90), generator=rng, device=dev, dtype=pos.dtype)
        loop = lambda fused, n: generate.denoise(model, sch, pos, neg, num_inference_steps=n, guidance_scale=6.0, latents=lat0, image_latents=il, fused=fused)
        lat, st["loop"] = _timed(lambda: loop(True, steps))
        frames, st["decode"] = _timed(lambda: generate.decode_latents(vae, lat, uint8=True))
        out["stages_seconds"] = st
        out["generation_seconds"] = sum(st.values())
        out["loop_ms_per_step"] = 1e3 * st["loop"] / steps
        out["frames_shape"] = list(frames.shape)
        out["latents_finite"] = bool(torch.isfinite(lat.float()).all())
        out["peak_allocated_gb"] = torch.cuda.max_memory_allocated(dev) / 1e9
        del frames
        # ---- the loop A/B, alternated in this process
        ta, tb = [], []
        la = lb = None
        for _ in range(a.ab_rounds):
            la, s = _timed(lambda: loop(True, ab_steps))
            ta.append(s)
            lb, s = _timed(lambda: loop(False, ab_steps))
            tb.append(s)
        diff = (la.float() - lb.float()).abs().max().item()
        out["loop_ab"] = {"steps": ab_steps, "rounds": a.ab_rounds, "fused_seconds": ta, "torch_ops_seconds": tb,
                          "fused_ms_per_step": 1e3 * statistics.median(ta) / ab_steps, "torch_ops_ms_per_step": 1e3 * statistics.median(tb) / ab_steps,
                          "fused_spread_ms_per_step": 1e3 * (max(ta) - min(ta)) / ab_steps, "torch_ops_spread_ms_per_step": 1e3 * (max(tb) - min(tb)) / ab_steps,
                          "max_abs_difference_of_latents": diff, "max_abs_latent": lb.float().abs().max().item()}
        # ---- the glue alone
        sch.set_timesteps(steps, device=dev)
        v = torch.randn(2, 13, 16, 60, 90, device=dev, dtype=torch.bfloat16)
        bufs = (torch.empty_like(lat0), torch.empty(lat0.shape, dtype=torch.float32, device=dev), torch.empty(2, 13, 32, 60, 90, device=dev, dtype=torch.bfloat16))
        coef, t_dev = sch.step_coefficients(steps // 2), sch.timesteps[steps // 2]

        def glue_fused():
            ops.sampler_step(v, lat0, coef, guidance_scale=6.0, image_latents=il, out=bufs)

        def glue_torch():
            vf = v.float()
            v_u, v_c = vf.chunk(2)
            x = sch.step(v_u + 6.0 * (v_c - v_u), t_dev, lat0)[0].to(torch.bfloat16)
            return torch.cat([torch.cat([x] * 2), torch.cat([il] * 2)], dim=2)

        fa, fb = [], []
        for _ in range(3):
            fa.append(median_ms(glue_fused, 3, 20)[0])
            fb.append(median_ms(glue_torch, 3, 20)[0])
        out["glue_ab"] = {"fused_ms": fa, "torch_ops_ms": fb, "fused_ms_median": statistics.median(fa), "torch_ops_ms_median": statistics.median(fb)}
    out["bytes_per_step"] = step_bytes(1, 13, 16, 16, 60, 90, True)
    out["glue_share_of_step"] = {"fused": out["glue_ab"]["fused_ms_median"] / out["loop_ms_per_step"],
                                 "torch_ops": out["glue_ab"]["torch_ops_ms_median"] / out["loop_ms_per_step"]}
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
