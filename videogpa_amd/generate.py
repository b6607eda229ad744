"""Denoising loop of the reference's generate path (generate/CogVideoX-5B.py:17-31,70-77 -> diffusers
CogVideoXPipeline.__call__): classifier-free guidance over a [uncond, cond] batch, 3D RoPE tables, the DPM scheduler,
with the MI355X transformer (RoPE kernel live) and a merged LoRA adapter, and the pipeline's decode_latents on the device VAE
decoder (videogpa_amd.vae with with_decoder=True): `denoise` returns latents, `decode_latents` turns them into `output.frames`.
Text encoding runs on the device too (videogpa_amd.t5.T5EncoderModel): `encode_prompt` turns token ids into the prompt embeddings `denoise` takes, so
the whole path prompt ids -> embeddings -> denoise -> VAE decode -> frames stays on the GPU.  Tokenisation is the caller's: the sentencepiece
tokenizer is string work on the host (`tokenizer(prompt, padding="max_length", max_length=226, truncation=True, add_special_tokens=True,
return_tensors="pt").input_ids`, as the pipeline calls it).
PARITY UNPINNED (diffusers not vendored): restated from pipeline_cogvideox.py / embeddings.get_3d_rotary_pos_embed."""
import torch


@torch.no_grad()
def decode_latents(vae, latents, uint8=False):
    """CogVideoXPipeline.decode_latents: latents [B,F,C,h,w] (what `denoise` returns) -> `vae.decode(latents.permute(0,2,1,3,4) /
    vae.config.scaling_factor).sample`, the frames [B,3,F',8h,8w] in the VAE's dtype, values in about [-1,1].  uint8=True: the pipeline's
    postprocess_video on top, [B,F',8h,8w,3] uint8, the layout the scorer takes frames in.  `vae` is an AutoencoderKLCogVideoX built with
    with_decoder=True; its slicing and tiling switches apply."""
    z = (1 / vae.config.scaling_factor) * latents.permute(0, 2, 1, 3, 4)
    return vae.decode_uint8(z) if uint8 else vae.decode(z).sample


@torch.no_grad()
def encode_prompt(text_encoder, input_ids, negative_input_ids=None, num_videos_per_prompt=1, dtype=None):
    """CogVideoXPipeline.encode_prompt / _get_t5_prompt_embeds behind the tokenizer: `text_encoder(input_ids)[0]` with NO attention mask (the
    pipeline passes none), cast to `dtype` (default: the encoder's), each prompt's embeddings repeated num_videos_per_prompt times in a row ->
    (prompt_embeds, negative_prompt_embeds), each [B * num_videos_per_prompt, S, d_model], ready for `denoise`.  input_ids / negative_input_ids are
    int [B,S] as the tokenizer pads them (max_length 226).  The pipeline encodes the negative prompt "" when guidance is on and none is given: pass
    the ids of "" for that; with negative_input_ids=None the second result is None (and `denoise` falls back to zeros, which the pipeline never does)."""
    def one(ids):
        e = text_encoder(ids)[0]
        e = e.to(dtype=dtype or e.dtype)
        b, s, _ = e.shape
        return e.repeat(1, num_videos_per_prompt, 1).view(b * num_videos_per_prompt, s, -1)

    if negative_input_ids is not None and tuple(negative_input_ids.shape) != tuple(input_ids.shape):
        raise ValueError(f"encode_prompt: negative_input_ids {tuple(negative_input_ids.shape)} and input_ids {tuple(input_ids.shape)} differ in shape")
    return one(input_ids), None if negative_input_ids is None else one(negative_input_ids)


def rope_3d_tables(num_frames, grid_h, grid_w, head_dim=64, theta=10000.0, device="cuda"):
    """(cos, sin) fp32 [F*h*w, head_dim], pair-repeated, t/h/w split = d/4, 3d/8, 3d/8 (native-resolution grid)."""
    dim_t, dim_h, dim_w = head_dim // 4, head_dim // 8 * 3, head_dim // 8 * 3

    def axis(dim, n):
        freqs = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float32)[: dim // 2] / dim))
        ang = torch.outer(torch.arange(n, dtype=torch.float32), freqs)
        return ang.cos().repeat_interleave(2, dim=1), ang.sin().repeat_interleave(2, dim=1)

    (ct, st), (ch, sh), (cw, sw) = axis(dim_t, num_frames), axis(dim_h, grid_h), axis(dim_w, grid_w)

    def combine(t, h, w):
        t = t[:, None, None, :].expand(-1, grid_h, grid_w, -1)
        h = h[None, :, None, :].expand(num_frames, -1, grid_w, -1)
        w = w[None, None, :, :].expand(num_frames, grid_h, -1, -1)
        return torch.cat([t, h, w], dim=-1).reshape(num_frames * grid_h * grid_w, head_dim)

    return combine(ct, ch, cw).to(device), combine(st, sh, sw).to(device)


def dynamic_guidance_scale(guidance_scale, num_inference_steps, t):
    """`use_dynamic_cfg=True` of the pipeline (generate/CogVideoX1.5-5B.py:85): the scale grows with a cosine ramp in the timestep
    VALUE t (as upstream writes it): 1 + g * (1 - cos(pi * ((n - t) / n) ** 5)) / 2."""
    import math
    return 1 + guidance_scale * ((1 - math.cos(math.pi * ((num_inference_steps - float(t)) / num_inference_steps) ** 5.0)) / 2)


@torch.no_grad()
def denoise(transformer, scheduler, prompt_embeds, negative_prompt_embeds=None, latent_frames=13, height=60, width=90,
            num_inference_steps=50, guidance_scale=6.0, generator=None, latents=None, step_noise=None, use_dynamic_cfg=False):
    """-> latents [B, F, C, H, W].  `latents` / `step_noise` ([steps, 2, B, F, C, H, W]) may be injected for parity tests.
    With patch_size_t (CogVideoX1.5) and a latent frame count that is not a multiple of it, the pipeline denoises with extra
    leading frames and drops them at the end; the same is done here."""
    cfg = transformer.config
    dev, dt = prompt_embeds.device, prompt_embeds.dtype
    B = prompt_embeds.shape[0]
    do_cfg = guidance_scale > 1.0
    if do_cfg:
        if negative_prompt_embeds is None:
            negative_prompt_embeds = torch.zeros_like(prompt_embeds)
        embeds = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)
    else:
        embeds = prompt_embeds
    pt_ = cfg.patch_size_t or 1
    extra = (pt_ - latent_frames % pt_) % pt_
    latent_frames = latent_frames + extra
    shape = (B, latent_frames, cfg.in_channels, height, width)
    if latents is None:
        latents = torch.randn(shape, generator=generator, device=dev, dtype=dt)
    latents = latents * scheduler.init_noise_sigma
    rope = None
    if cfg.use_rotary_positional_embeddings:
        p, pt = cfg.patch_size, (cfg.patch_size_t or 1)
        rope = rope_3d_tables((latent_frames + pt - 1) // pt, height // p, width // p, cfg.attention_head_dim, device=dev)
    scheduler.set_timesteps(num_inference_steps, device=dev)
    ts = scheduler.timesteps
    old_x0 = None
    for i, t in enumerate(ts):
        inp = torch.cat([latents] * 2) if do_cfg else latents
        inp = scheduler.scale_model_input(inp, t)
        v = transformer(hidden_states=inp, encoder_hidden_states=embeds, timestep=t.expand(inp.shape[0]), image_rotary_emb=rope,
                        return_dict=False)[0].float()
        if do_cfg:
            g_now = dynamic_guidance_scale(guidance_scale, num_inference_steps, t.item()) if use_dynamic_cfg else guidance_scale
            v_u, v_c = v.chunk(2)
            v = v_u + g_now * (v_c - v_u)
        latents, old_x0 = scheduler.step(v, old_x0, t, ts[i - 1] if i > 0 else None, latents, generator=generator,
                                         noise=None if step_noise is None else step_noise[i])
        latents = latents.to(dt)
    return latents[:, extra:] if extra else latents
