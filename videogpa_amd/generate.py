"""Denoising loop of the reference's generate path (generate/CogVideoX-5B.py:17-31,70-77 -> diffusers
CogVideoXPipeline.__call__): classifier-free guidance over a [uncond, cond] batch, 3D RoPE tables, the DPM scheduler,
with the MI355X transformer (RoPE kernel live) and a merged LoRA adapter, and the pipeline's decode_latents on the device VAE
decoder (videogpa_amd.vae with with_decoder=True): `denoise` returns latents, `decode_latents` turns them into `output.frames`.
Text encoding runs on the device too (videogpa_amd.t5.T5EncoderModel): `encode_prompt` turns token ids into the prompt embeddings `denoise` takes, so
the whole path prompt ids -> embeddings -> denoise -> VAE decode -> frames stays on the GPU.  Tokenisation is the caller's: the sentencepiece
tokenizer is string work on the host (`tokenizer(prompt, padding="max_length", max_length=226, truncation=True, add_special_tokens=True,
return_tensors="pt").input_ids`, as the pipeline calls it).
Image to video (generate/CogVideoX-5B-I2V.py, replicate.py) is the second half of this file: `preprocess_image` (PIL-exact Lanczos resize on the device),
`prepare_image_latents`, `denoise(image_latents=...)` on the fused sampler step (csrc/sampler.hip) and `image_to_video` for the whole call.
PARITY UNPINNED (diffusers not vendored): restated from pipeline_cogvideox.py / pipeline_cogvideox_image2video.py / embeddings.get_3d_rotary_pos_embed."""
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
            num_inference_steps=50, guidance_scale=6.0, generator=None, latents=None, step_noise=None, use_dynamic_cfg=False,
            image_latents=None, ofs=None, fused=None):
    """-> latents [B, F, C, H, W].  `latents` / `step_noise` ([steps, 2, B, F, C, H, W]) may be injected for parity tests.
    With patch_size_t (CogVideoX1.5) and a latent frame count that is not a multiple of it, the pipeline denoises with extra
    leading frames and drops them at the end; the same is done here.
    image_latents [B, F, C_img, H, W] (prepare_image_latents) selects the image-to-video loop (`_denoise_i2v`: the channel concat at every step, `ofs`,
    and the fused sampler step); without it the loop below is the text-to-video one, unchanged."""
    if image_latents is not None:
        return _denoise_i2v(transformer, scheduler, prompt_embeds, negative_prompt_embeds, image_latents, num_inference_steps, guidance_scale,
                            generator, latents, step_noise, use_dynamic_cfg, ofs, fused)
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


# ---------------------------------------------------------------------------------------------------------------- image to video
# generate/CogVideoX-5B-I2V.py:18-89 and replicate.py:160-240 -> diffusers CogVideoXImageToVideoPipeline.__call__.
# PARITY UNPINNED (diffusers not vendored): restated from pipeline_cogvideox_image2video.py (prepare_latents, the denoising loop), image_processor.py
# (VaeImageProcessor.preprocess: PIL Lanczos resize, / 255, 2 x - 1) and scheduling_ddim_cogvideox.py; the order of the random draws, the released
# checkpoint's scheduler_config.json and the resize filter are as those files are remembered, not as a run of the real packages shows them.
@torch.no_grad()
def preprocess_image(image_u8, height=480, width=720, dtype=torch.bfloat16, pre_resize=None):
    """The pipeline's `video_processor.preprocess(image, height, width)` behind the PNG decoder: uint8 [H,W,3] or [B,H,W,3] on the device ->
    [B,3,height,width] in `dtype`, values in [-1,1]: PIL Lanczos resize to (width, height), skipped when the size already matches (PIL returns a copy),
    then x / 255 * 2 - 1 in fp32, rounded once.  pre_resize=(w, h), PIL's order, applies `image.resize((w, h))` first: PIL's default bicubic, as
    replicate.py:201 does with (1080, 720)."""
    from . import ops
    x = image_u8[None] if image_u8.dim() == 3 else image_u8
    if x.dim() != 4 or x.shape[-1] != 3 or x.dtype != torch.uint8:
        raise ValueError(f"preprocess_image: expected uint8 [H,W,3] or [B,H,W,3], got {image_u8.dtype} {tuple(image_u8.shape)}")
    x = x.contiguous()
    if pre_resize is not None and (x.shape[2], x.shape[1]) != tuple(pre_resize):
        x = ops.image_resize(x, pre_resize[1], pre_resize[0], "bicubic")
    if (x.shape[1], x.shape[2]) != (height, width):
        x = ops.image_resize(x, height, width, "lanczos")
    return ops.image_to_pm1(x, dtype)


@torch.no_grad()
def prepare_image_latents(vae, image, latent_frames, generator=None):
    """The image half of the pipeline's prepare_latents: image [B,3,H,W] in [-1,1] -> [B, latent_frames, C, H/8, W/8] in the VAE's dtype: per sample
    `vae.encode(img[None, :, None]).latent_dist.sample(generator)`, as [B,1,C,h,w], times scaling_factor (its reciprocal under
    config.invert_scale_latents, CogVideoX1.5), zero frames behind it.  Call it BEFORE the initial noise is drawn from the same generator: upstream
    draws the image latents first."""
    if image.dim() != 4 or image.shape[1] != 3:
        raise ValueError(f"prepare_image_latents: expected [B,3,H,W], got {tuple(image.shape)}")
    img = image.to(vae.dtype)
    lat = torch.cat([vae.encode(img[b][None, :, None]).latent_dist.sample(generator) for b in range(img.shape[0])], dim=0).permute(0, 2, 1, 3, 4)
    sf = vae.config.scaling_factor
    lat = (1 / sf) * lat if vae.config.get("invert_scale_latents", False) else sf * lat
    B, _, C, h, w = lat.shape
    return torch.cat([lat, lat.new_zeros(B, latent_frames - 1, C, h, w)], dim=1)


def _denoise_i2v(transformer, scheduler, prompt_embeds, negative_prompt_embeds, image_latents, num_inference_steps, guidance_scale, generator,
                 latents, step_noise, use_dynamic_cfg, ofs, fused):
    """`denoise` with image_latents.  fused=None takes the fused step (ops.sampler_step: guidance, scheduler update, cast and the next input's two
    concatenations in one pass, every scalar from the host copy of the timesteps, so nothing in the loop waits for the device) whenever the scheduler
    offers step_coefficients; fused=False runs the same loop on torch ops as the pipeline writes it (what tools/i2v_generate_bench.py compares)."""
    from . import ops
    from .scheduler import CogVideoXDPMScheduler
    cfg = transformer.config
    dev, dt = prompt_embeds.device, prompt_embeds.dtype
    B, Fr, C_img, height, width = image_latents.shape
    C = cfg.in_channels - C_img
    if cfg.patch_size_t is not None:
        raise NotImplementedError("denoise(image_latents=...): patch_size_t (CogVideoX1.5 I2V pads the first frame's latents) is not implemented")
    if C <= 0 or B != prompt_embeds.shape[0]:
        raise ValueError(f"denoise: image_latents {tuple(image_latents.shape)} do not fit in_channels {cfg.in_channels} and {prompt_embeds.shape[0]} prompts")
    if cfg.use_learned_positional_embeddings and (height, width) != (cfg.sample_height, cfg.sample_width):
        raise ValueError(f"denoise: learned positional embeddings hold {cfg.sample_height} x {cfg.sample_width} latents only, got {height} x {width}")
    if fused is None:
        fused = hasattr(scheduler, "step_coefficients")
    do_cfg = guidance_scale > 1.0
    if do_cfg:
        if negative_prompt_embeds is None:
            negative_prompt_embeds = torch.zeros_like(prompt_embeds)
        embeds = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)
    else:
        embeds = prompt_embeds
    G = 2 if do_cfg else 1
    image_latents = image_latents.to(dt).contiguous()
    if latents is None:
        latents = torch.randn((B, Fr, C, height, width), generator=generator, device=dev, dtype=dt)
    latents = (latents * scheduler.init_noise_sigma).contiguous()
    rope = None
    if cfg.use_rotary_positional_embeddings:
        rope = rope_3d_tables(Fr, height // cfg.patch_size, width // cfg.patch_size, cfg.attention_head_dim, device=dev)
    if ofs is None and cfg.ofs_embed_dim is not None:
        ofs = latents.new_full((1,), 2.0)
    scheduler.set_timesteps(num_inference_steps, device=dev)
    ts = scheduler.timesteps
    ts_host = getattr(scheduler, "timesteps_host", None)
    g_at = lambda i: (dynamic_guidance_scale(guidance_scale, num_inference_steps, ts_host[i] if ts_host is not None else ts[i].item())
                      if use_dynamic_cfg else guidance_scale)
    model = lambda inp, t: transformer(hidden_states=inp, encoder_hidden_states=embeds, timestep=t.expand(inp.shape[0]), ofs=ofs,
                                       image_rotary_emb=rope, return_dict=False)[0]
    if not fused:
        old_x0 = None
        img_in = torch.cat([image_latents] * G)
        for i, t in enumerate(ts):
            inp = torch.cat([latents] * G) if do_cfg else latents
            inp = scheduler.scale_model_input(inp, t)
            v = model(torch.cat([inp, img_in], dim=2), t).float()
            if do_cfg:
                v_u, v_c = v.chunk(2)
                v = v_u + g_at(i) * (v_c - v_u)
            if isinstance(scheduler, CogVideoXDPMScheduler):
                latents, old_x0 = scheduler.step(v, old_x0, t, ts[i - 1] if i > 0 else None, latents, generator=generator,
                                                 noise=None if step_noise is None else step_noise[i])
            else:
                latents, old_x0 = scheduler.step(v, t, latents, generator=generator)
            latents = latents.to(dt)
        return latents
    # the fused loop: two (x_next, x0, packed) triples written in turn; the first input is packed once by torch
    bufs = [(torch.empty_like(latents), torch.empty(latents.shape, dtype=torch.float32, device=dev),
             torch.empty(G * B, Fr, C + C_img, height, width, dtype=dt, device=dev)) for _ in range(2)]
    inp = torch.cat([torch.cat([latents] * G), torch.cat([image_latents] * G)], dim=2)
    old_x0 = None
    for i in range(len(ts)):
        coef = scheduler.step_coefficients(i)
        v = model(inp, ts[i])
        noise = None
        if coef["k_n"] is not None:
            # CogVideoXDPMScheduler.step draws once, and once more where it uses the history: the same draws in the same order
            draws = 2 if coef["k_old"] is not None else 1
            if step_noise is not None:
                noise = step_noise[i][draws - 1].to(dt).contiguous()
            else:
                for _ in range(draws):
                    noise = torch.randn(latents.shape, generator=generator, device=dev, dtype=dt)
        latents, old_x0, inp = ops.sampler_step(v.contiguous(), latents, coef, guidance_scale=g_at(i) if do_cfg else None, x0_old=old_x0, noise=noise,
                                                image_latents=image_latents, out=bufs[i % 2])
    return latents


@torch.no_grad()
def image_to_video(transformer, vae, scheduler, text_encoder, image_u8, input_ids, negative_input_ids, num_frames=49, num_inference_steps=50,
                   guidance_scale=6.0, generator=None, uint8=True, pre_resize=None):
    """The whole call of replicate.py:234-240 / generate/CogVideoX-5B-I2V.py:82-88 behind the tokenizer and in front of the mp4 writer:
    preprocess_image -> encode_prompt -> prepare_image_latents -> initial noise -> denoise -> decode_latents.  image_u8: uint8 [H,W,3] | [B,H,W,3] on the
    device; input_ids / negative_input_ids: the tokenizer's padded ids of the prompt and of "" ([B,226]).  The frame size is the transformer's:
    8 * sample_height x 8 * sample_width (480 x 720).  -> `output.frames` as the scorer takes them: uint8 [B, num_frames, H, W, 3] (uint8=False: the
    decoder's [B,3,num_frames,H,W] in about [-1,1])."""
    cfg = transformer.config
    sp = 2 ** (len(vae.config.block_out_channels) - 1)
    height, width = cfg.sample_height * sp, cfg.sample_width * sp
    latent_frames = (num_frames - 1) // cfg.temporal_compression_ratio + 1
    prompt, negative = encode_prompt(text_encoder, input_ids, negative_input_ids if guidance_scale > 1.0 else None)
    image = preprocess_image(image_u8, height, width, dtype=prompt.dtype, pre_resize=pre_resize)
    image_latents = prepare_image_latents(vae, image, latent_frames, generator).to(prompt.dtype)      # drawn before the initial noise, as upstream
    latents = torch.randn((image.shape[0], latent_frames, cfg.in_channels - image_latents.shape[2], cfg.sample_height, cfg.sample_width),
                          generator=generator, device=prompt.device, dtype=prompt.dtype)
    latents = denoise(transformer, scheduler, prompt, negative, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                      generator=generator, latents=latents, image_latents=image_latents)
    return decode_latents(vae, latents, uint8=uint8)
