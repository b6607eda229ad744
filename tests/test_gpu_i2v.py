"""Image-to-video generation on the device (videogpa_amd.generate: preprocess_image, prepare_image_latents, denoise(image_latents=...), image_to_video)
and its kernels: the fused sampler step (csrc/sampler.hip) against the fp64 restatement of tests/i2v_ref.py inside its per-element bound, the PIL-exact
resize to any size (csrc/preprocess.hip) against tests/resize_ref.py byte for byte.  -m gpu only."""
import functools

import numpy as np
import pytest
import torch

import i2v_ref
import resize_ref
import row_tol
import t5_ref
import vae_decoder_oracle as vd
import vae_oracle as vo
from oracle import cogvideox as ocv
from oracle import scheduler as osch
from videogpa_amd import ops
from videogpa_amd.generate import denoise, image_to_video, prepare_image_latents, preprocess_image
from videogpa_amd.scheduler import CogVideoXDDIMScheduler, CogVideoXDPMScheduler

pytestmark = pytest.mark.gpu

NARROW = dict(block_out_channels=(32, 64, 64, 64), layers_per_block=2)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------------------------------------------------------- 1. the fused sampler step
def _coef(kind):
    """real coefficients of a 6-step schedule: DDIM (no history, no noise), DPM first order (noise only), DPM second order (history and noise)"""
    sch = CogVideoXDDIMScheduler() if kind == "ddim" else CogVideoXDPMScheduler()
    sch.set_timesteps(6)
    return sch.step_coefficients({"ddim": 2, "dpm1": 0, "dpm2": 3}[kind])


def _sampler_case(B, F, h, w, dtype, v_dtype, guided, kind, image, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * B + 11 * F + 13 * h + w)
    G = 2 if guided else 1
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(B, F, 16, h, w).to(dtype).cuda()
    v = (0.8 * r(G * B, F, 16, h, w)).to(v_dtype).cuda()
    old = (0.9 * r(B, F, 16, h, w)).cuda()
    noise = r(B, F, 16, h, w).to(dtype).cuda()
    img = (0.7 * r(B, F, 16, h, w)).to(dtype).cuda() if image else None
    return x, v, old, noise, img


def _check_sampler(x, v, old, noise, img, coef, guided):
    gs = 6.0 if guided else None
    G = 2 if guided else 1
    x_next, x0, packed = ops.sampler_step(v, x, coef, guidance_scale=gs, x0_old=old, noise=noise, image_latents=img)
    ref, ref0, tol, tol0 = i2v_ref.sampler_step_ref(v, x, coef, gs, old, noise)
    assert x_next.dtype == x.dtype and x0.dtype == torch.float32 and x_next.shape == x.shape == x0.shape
    if x.dtype == torch.bfloat16:
        tol = tol + row_tol.half_ulp_bf16(ref.abs() + tol)
    print("x_next worst err / bound, err, bound:", row_tol.worst(x_next, ref, tol), " x0:", row_tol.worst(x0, ref0, tol0))
    bad = row_tol.judge("x_next", x_next, ref, tol) + row_tol.judge("x0", x0, ref0, tol0)
    assert not bad, "\n".join(bad)
    if img is None:
        assert packed is None
    else:
        assert packed.dtype == x.dtype and torch.equal(packed, i2v_ref.packed_ref(x_next, img, G))
    return x_next, x0, packed


@pytest.mark.parametrize("image", [False, True])
@pytest.mark.parametrize("kind", ["ddim", "dpm1", "dpm2"])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("dtype,v_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16)])
@pytest.mark.parametrize("shape", [(1, 3, 4, 4), (2, 3, 5, 7)])
def test_sampler_step_against_fp64(shape, dtype, v_dtype, guided, kind, image):
    """(2,3,5,7): 35 pixels, C h w = 560 = 70 chunks of 8 per frame, so frames do not start on a block boundary and the second sample and the second guidance
    half have their own offsets"""
    x, v, old, noise, img = _sampler_case(*shape, dtype, v_dtype, guided, kind, image)
    coef = _coef(kind)
    assert (coef["k_old"] is not None) == (kind == "dpm2") and (coef["k_n"] is not None) == (kind != "ddim")
    _check_sampler(x, v, old if kind == "dpm2" else None, noise if kind != "ddim" else None, img, coef, guided)


def test_sampler_step_grid_stride_and_output_reuse():
    """(1,17,128,128) with the image half: 2 x 557 056 chunks of 8 over a grid capped at 2048 blocks of 256 threads, so every thread strides; the second call
    writes into the first call's outputs (the loop's two triples) and gives the same bits"""
    x, v, old, noise, img = _sampler_case(1, 17, 128, 128, torch.bfloat16, torch.bfloat16, True, "dpm2", True)
    coef = _coef("dpm2")
    assert 17 * 32 * 128 * 128 // 8 > 2048 * 256
    first = _check_sampler(x, v, old, noise, img, coef, True)
    keep = [t.clone() for t in first]
    again = ops.sampler_step(v, x, coef, guidance_scale=6.0, x0_old=old, noise=noise, image_latents=img, out=first)
    assert all(a is b for a, b in zip(again, first)) and all(torch.equal(a, k) for a, k in zip(again, keep))


def test_sampler_step_refuses_what_it_cannot_vectorise():
    """C h w = 16 * 3 * 3 = 144 is a multiple of 8, 12 * 3 * 3 = 108 is not (latents), nor is 4 * 3 * 3 = 36 (image half): VGPA_ERR_INVALID, and nothing is launched --
    the outputs keep their fill"""
    coef = _coef("ddim")
    for C, C_img in ((12, 16), (16, 4)):
        x = torch.zeros(1, 2, C, 3, 3, device="cuda")
        v = torch.ones(1, 2, C, 3, 3, device="cuda")
        img = torch.ones(1, 2, C_img, 3, 3, device="cuda")
        out = (torch.full_like(x, 7.0), torch.full_like(x, 7.0), torch.full((1, 2, C + C_img, 3, 3), 7.0, device="cuda"))
        with pytest.raises(RuntimeError, match="vgpa_sampler_step failed: invalid argument"):
            ops.sampler_step(v, x, coef, image_latents=img, out=out)
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in out)
    with pytest.raises(RuntimeError, match="history"):
        ops.sampler_step(torch.ones(1, 2, 16, 4, 4, device="cuda"), torch.ones(1, 2, 16, 4, 4, device="cuda"), _coef("dpm2"),
                         noise=torch.ones(1, 2, 16, 4, 4, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- 2. resize and the [-1, 1] tensor
@functools.lru_cache(maxsize=None)
def _resize_case(src, dst, filter):
    """three different frames of one size and their references (computed once)"""
    frames = np.stack([resize_ref.test_image(*src, seed=s) for s in range(3)])
    return frames, np.stack([resize_ref.resize(f, dst[0], dst[1], filter) for f in frames])


@pytest.mark.parametrize("filter", ["bicubic", "lanczos"])
@pytest.mark.parametrize("src,dst", resize_ref.SIZES)
def test_image_resize_equals_the_restatement_byte_for_byte(src, dst, filter):
    frames, want = _resize_case(src, dst, filter)
    for T in (1, 3):
        got = ops.image_resize(torch.from_numpy(frames[:T]).cuda(), dst[0], dst[1], filter)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (T, dst[0], dst[1], 3)
        diff = (got.cpu().numpy().astype(int) - want[:T]).__abs__()
        assert diff.max() == 0, (src, dst, filter, T, int(diff.max()), int((diff > 0).sum()))


def test_image_to_pm1_is_exact_and_preprocess_image_chains_the_resizes():
    every = torch.arange(256, dtype=torch.uint8).repeat(3)[: 2 * 4 * 32 * 3].reshape(2, 4, 32, 3).contiguous()
    want32 = (every.float() / 255 * 2 - 1).permute(0, 3, 1, 2)          # CPU torch: a true fp32 division, then 2 x - 1
    assert set(every.flatten().tolist()) == set(range(256))
    for dtype in (torch.float32, torch.bfloat16):
        got = ops.image_to_pm1(every.cuda(), dtype)
        assert got.dtype == dtype and torch.equal(got.cpu(), want32.to(dtype))
    # replicate.py:201 + the pipeline: bicubic to 1080 x 720, Lanczos to 720 x 480, [-1, 1]; here a quarter of that in each direction
    img = resize_ref.test_image(100, 150)
    chain = resize_ref.resize(resize_ref.resize(img, 180, 270, "bicubic"), 120, 180, "lanczos")
    got = preprocess_image(torch.from_numpy(img).cuda(), 120, 180, dtype=torch.float32, pre_resize=(270, 180))
    want = (torch.from_numpy(chain).float() / 255 * 2 - 1).permute(2, 0, 1)[None]
    assert tuple(got.shape) == (1, 3, 120, 180) and torch.equal(got.cpu(), want)
    # an image of the right size is not resampled, as PIL returns a copy
    same = preprocess_image(torch.from_numpy(chain).cuda()[None], 120, 180, dtype=torch.bfloat16)
    assert same.dtype == torch.bfloat16 and torch.equal(same.cpu(), want.to(torch.bfloat16))
    with pytest.raises(ValueError):
        preprocess_image(torch.zeros(4, 4, 3, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- 3. the image latents
@functools.lru_cache(maxsize=None)
def _small_vae():
    from videogpa_amd.vae import AutoencoderKLCogVideoX
    vae = AutoencoderKLCogVideoX(with_decoder=True, sample_height=64, sample_width=96, **NARROW)
    vae.load_state_dict({**vo.seeded_state_dict(**NARROW, seed=21), **vd.seeded_decoder_state_dict(**NARROW, seed=23)})
    return vae.to(device="cuda", dtype=torch.bfloat16).requires_grad_(False).eval()


def test_prepare_image_latents_is_the_hand_written_sequence_and_draws_first():
    vae = _small_vae()
    img = (2 * torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(3)) - 1).to(torch.bfloat16).cuda()
    gen = lambda: torch.Generator(device="cuda").manual_seed(1234)
    g = gen()
    lat = prepare_image_latents(vae, img, 3, g)
    noise_after = torch.randn(2, 3, 16, 8, 12, generator=g, device="cuda", dtype=torch.bfloat16)
    assert lat.dtype == torch.bfloat16 and tuple(lat.shape) == (2, 3, 16, 8, 12)
    g = gen()
    with torch.no_grad():
        hand = [vae.encode(img[b][None, :, None]).latent_dist.sample(g) for b in range(2)]
    hand = torch.cat(hand).permute(0, 2, 1, 3, 4) * vae.config.scaling_factor
    assert torch.equal(lat[:, :1], hand) and float(lat[:, 1:].abs().max()) == 0.0 and float(lat[:, 0].float().abs().max()) > 0.05
    # the other order of the two draws gives other latents (and other noise)
    g = gen()
    noise_first = torch.randn(2, 3, 16, 8, 12, generator=g, device="cuda", dtype=torch.bfloat16)
    lat_second = prepare_image_latents(vae, img, 3, g)
    assert not torch.equal(lat_second, lat) and not torch.equal(noise_first, noise_after)
    # CogVideoX1.5 divides by the scaling factor instead
    vae.config["invert_scale_latents"] = True
    try:
        inv = prepare_image_latents(vae, img, 3, gen())
    finally:
        vae.config["invert_scale_latents"] = False
    sf = vae.config.scaling_factor
    assert torch.allclose(inv[:, 0].float() * sf * sf, lat[:, 0].float(), rtol=2 ** -6, atol=1e-3)


# ---------------------------------------------------------------------------------------------------------------- 4. the loop, end to end
I2V_KW = dict(num_attention_heads=2, attention_head_dim=64, num_layers=2, time_embed_dim=32, text_embed_dim=48, sample_width=8, sample_height=8,
              sample_frames=9, max_text_seq_length=6, in_channels=32, use_learned_positional_embeddings=True)


@functools.lru_cache(maxsize=None)
def _i2v_setup():
    """the small I2V model of tests/test_gpu_cfg34.py / test_gpu_model.py (32 channels in, learned positions and RoPE) with a seeded adapter, its inputs, and
    the fp64 CPU reference of the MERGED model's 6-step DDIM loop (computed once)"""
    from videogpa_amd.lora import LoraConfig, get_peft_model
    from videogpa_amd.transformer import CogVideoXTransformer3DModel
    cfg = ocv.CogVideoXConfig(**I2V_KW)
    sd = {k: v.to(torch.bfloat16) for k, v in ocv.init_state_dict(cfg, seed=4, std=0.05, mod_std=0.2).items()}

    def wrapped():
        model = CogVideoXTransformer3DModel(use_rotary_positional_embeddings=True, **I2V_KW)
        model.load_state_dict(sd, strict=True)
        pm = get_peft_model(model.to(device="cuda", dtype=torch.bfloat16), LoraConfig(r=4, lora_alpha=8, target_modules=["to_q", "to_k", "to_v", "to_out.0"]))
        own = pm.state_dict()
        for k, v in ocv.init_lora(cfg, r=4, seed=5, b_std=0.05).items():
            own[k[:-len(".weight")] + ".default.weight"].copy_(v)
        return pm.eval()

    g = torch.Generator().manual_seed(77)
    pos = (0.5 * torch.randn(1, 6, cfg.text_embed_dim, generator=g)).to(torch.bfloat16)
    neg = (0.5 * torch.randn(1, 6, cfg.text_embed_dim, generator=g)).to(torch.bfloat16)
    lat0 = torch.randn(1, 3, 16, 8, 8, generator=g).to(torch.bfloat16)
    img = torch.cat([0.7 * torch.randn(1, 1, 16, 8, 8, generator=g), torch.zeros(1, 2, 16, 8, 8)], dim=1).to(torch.bfloat16)
    return cfg, wrapped, pos, neg, lat0, img


def _reference(cfg, model, pos, neg, lat0, img, steps=6):
    sdm = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    cos, sin = ocv.rope_3d_tables(3, 4, 4, 64)
    emb = torch.cat([neg, pos]).double()
    fwd = lambda inp, t: ocv.forward(sdm, cfg, inp, emb, t.expand(2), image_rotary_emb=(cos.double(), sin.double()))
    return i2v_ref.i2v_loop_ref(fwd, osch.alphas_cumprod(), osch.trailing_timesteps(steps), lat0, img, 6.0)


def _run(model, pos, neg, lat0, img, fused, sch=None, **kw):
    return denoise(model, sch or CogVideoXDDIMScheduler(), pos.cuda(), neg.cuda(), num_inference_steps=6, guidance_scale=6.0, latents=lat0.cuda(),
                   image_latents=img.cuda(), fused=fused, **kw)


def test_i2v_denoise_matches_the_fp64_loop_fused_and_unfused_and_through_an_unmerged_adapter():
    cfg, wrapped, pos, neg, lat0, img = _i2v_setup()
    pm = wrapped()
    layers = [m for m in pm.modules() if hasattr(m, "scaling") and "default" in getattr(m, "scaling", {})]
    assert len(layers) == 8
    w = 0.5
    # replicate.py:206-216: scaling[adapter] = w * alpha / r on the UNMERGED adapter, between generations, no re-wrapping
    for m in layers:
        m.scaling["default"] = w * m.lora_alpha["default"] / m.r["default"]
    unmerged = _run(pm, pos, neg, lat0, img, None)
    for m in layers:
        m.scaling["default"] = 0.0
    zero = _run(pm, pos, neg, lat0, img, None)
    with pm.disable_adapter():
        base = _run(pm, pos, neg, lat0, img, None)
    assert torch.equal(zero, base) and not torch.equal(zero, unmerged)
    for m in layers:
        m.scaling["default"] = w * m.lora_alpha["default"] / m.r["default"]
    assert torch.equal(_run(pm, pos, neg, lat0, img, None), unmerged)          # and back: the sweep holds no stale operand
    merged = pm.merge_and_unload()
    ref = _reference(cfg, merged, pos, neg, lat0, img)
    scale = ref.abs().max().item()
    fused, plain = _run(merged, pos, neg, lat0, img, None), _run(merged, pos, neg, lat0, img, False)
    assert fused.dtype == torch.bfloat16 and tuple(fused.shape) == (1, 3, 16, 8, 8)
    errs = {k: (v.double().cpu() - ref).abs().max().item() for k, v in (("fused", fused), ("torch ops", plain), ("unmerged adapter", unmerged))}
    print("I2V 6-step DDIM loop: max |err| against fp64", errs, "bound", 0.06 * scale)
    assert all(e < 0.06 * scale for e in errs.values()), (errs, scale)
    # the two loops see the same transformer and differ by the rounding of one step's update: fp32 against fp64 arithmetic before the one bf16 store.
    # One bf16 ulp per step at the magnitude of the result, carried through the six steps
    ulp = 2.0 * row_tol.half_ulp_bf16(ref.abs().clamp_min(scale / 256))
    between = (fused.double().cpu() - plain.double().cpu()).abs()
    print("fused against torch ops: max", between.max().item(), "in ulps", (between / ulp).max().item())
    assert bool((between <= 6 * ulp).all()), (between / ulp).max().item()


def test_i2v_denoise_with_the_dpm_sampler_and_its_refusals():
    cfg, wrapped, pos, neg, lat0, img = _i2v_setup()
    merged = wrapped().merge_and_unload()
    noise = torch.randn(6, 2, 1, 3, 16, 8, 8, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).cuda()
    fused = _run(merged, pos, neg, lat0, img, True, sch=CogVideoXDPMScheduler(), step_noise=noise)
    plain = _run(merged, pos, neg, lat0, img, False, sch=CogVideoXDPMScheduler(), step_noise=noise)
    scale = plain.float().abs().max().item()
    err = (fused.float() - plain.float()).abs().max().item()
    print("DPM fused against torch ops:", err, "of", scale)
    assert torch.isfinite(fused.float()).all() and err < 0.06 * scale
    # the generator path draws what scheduler.step draws: the same stream, so the same seed gives the same latents twice
    g = lambda: torch.Generator(device="cuda").manual_seed(9)
    a = _run(merged, pos, neg, lat0, img, True, sch=CogVideoXDPMScheduler(), generator=g())
    b = _run(merged, pos, neg, lat0, img, True, sch=CogVideoXDPMScheduler(), generator=g())
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="learned positional"):
        denoise(merged, CogVideoXDDIMScheduler(), pos.cuda(), neg.cuda(), num_inference_steps=2, image_latents=torch.zeros(1, 3, 16, 8, 10, device="cuda"))
    merged.config.patch_size_t = 2
    try:
        with pytest.raises(NotImplementedError, match="patch_size_t"):
            denoise(merged, CogVideoXDDIMScheduler(), pos.cuda(), neg.cuda(), num_inference_steps=2, image_latents=img.cuda())
    finally:
        merged.config.patch_size_t = None


def test_image_to_video_smoke():
    from videogpa_amd import t5
    from videogpa_amd.transformer import CogVideoXTransformer3DModel
    kw = dict(I2V_KW, text_embed_dim=64, sample_width=12)
    cfg = ocv.CogVideoXConfig(**kw)
    model = CogVideoXTransformer3DModel(use_rotary_positional_embeddings=True, **kw)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in ocv.init_state_dict(cfg, seed=4, std=0.05, mod_std=0.2).items()}, strict=True)
    model = model.to(device="cuda", dtype=torch.bfloat16).eval()
    tcfg = t5_ref.make_cfg()
    with torch.device("meta"):
        enc = t5.T5EncoderModel(tcfg)
    enc.load_state_dict({k: v.cuda() for k, v in t5_ref.seeded_state_dict(tcfg, seed=3).items()}, strict=True, assign=True)
    enc.encoder.embed_tokens.weight = enc.shared.weight
    ids = torch.randint(0, tcfg["vocab_size"], (2, 6), generator=torch.Generator().manual_seed(1)).cuda()
    image = torch.from_numpy(resize_ref.test_image(40, 50)).cuda()
    run = lambda seed: image_to_video(model, _small_vae(), CogVideoXDDIMScheduler(), enc, image, ids[:1], ids[1:], num_frames=9, num_inference_steps=2,
                                      guidance_scale=6.0, generator=torch.Generator(device="cuda").manual_seed(seed))
    a, b, c = run(42), run(42), run(43)
    assert a.dtype == torch.uint8 and tuple(a.shape) == (1, 9, 64, 96, 3)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.float().std().item() > 1.0
