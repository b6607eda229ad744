"""videogpa_amd.vae (the CogVideoX VAE encoder on one frame) and its kernels against tests/vae_oracle.py, the plain-torch restatement in the general 3-D
form, run on the CPU in fp64.  -m gpu only.

Accuracy convention (tests/test_gpu_vggt_heads.py's): error = max |device - o64| / max |o64| per output tensor.  The bound is not guessed: it is
4 x the SAME quantity of the oracle run in fp32 on the CPU (floor 1e-6), computed in the test next to the device's figure.  The device works in fp32
with another summation order (up to 9 * 512 products per output and the group reductions, which the kernels carry in fp64), so it has to sit within
a small multiple of what fp32 itself costs.  Modules are float32 here and hold bf16-representable weights (a bf16 checkpoint's values): in a bfloat16
module only the final rounding of the outputs differs.

Measured on an MI355X, device error / oracle-fp32 error (every test prints its own figures and its bound):
    GroupNorm + SiLU alone            N(0,1): 1.3e-7 ... 2.0e-7 / 1.3e-7 ... 2.0e-7;  N(100,1): 9.2e-7 ... 1.1e-6 / 2.3e-6 ... 3.6e-6
                                      one pixel: 2.5e-8 ... 6.7e-6 / 7.9e-8 ... 1.1e-2 (torch's fp32 group_norm is off by 1 % on one element per group at mean 100)
    one-sided stride-2 convolution    1.8e-7 ... 2.4e-7 / 2.4e-7 ... 3.4e-7;  other paddings 1.0e-7 ... 1.2e-7 / 1.6e-7 ... 1.8e-7;  stem 1.5e-7, 1.6e-7 / 3.3e-7, 2.3e-7
    resnet 128 -> 256 at 24 x 40      3.7e-7 / 3.9e-7
    narrow encoder                    mean 8.1e-7 / 1.6e-6, logvar 7.0e-7 / 9.3e-7, std 5.0e-7 / 6.9e-7, sample 3.9e-7 / 6.2e-7 (the worse of the two sizes)
    real-width encoder at 64 x 96     mean 7.8e-7 / 1.3e-6, logvar 8.0e-7 / 1.1e-6, std 6.1e-7 / 6.7e-7, sample 4.5e-7 / 5.9e-7
    tiled narrow encoder              3 x 3 grid: mean 8.5e-7 / 1.6e-6, logvar 6.0e-7 / 1.1e-6;  3 x 4 at half overlap: mean 5.1e-7 / 8.0e-7, logvar 8.0e-7 / 8.6e-7
With the convolution's K sum as ONE fp32 chain (ops.conv3x3_f32, what the VGGT heads and LPIPS use) the 128-channel downsampler measured 1.35e-6 against a
bound of 1.19e-6 and the real-width encoder's std 2.64e-6 against 2.67e-6; that is why the encoder's convolutions sum in runs of 64 products
(ops.conv3x3_pad_f32, csrc/conv_mfma.h CV_CONV_CHUNKED).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import vae_oracle as vo

pytestmark = pytest.mark.gpu

NARROW = dict(block_out_channels=(32, 64, 64, 64), layers_per_block=2)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _check(name, dev, o64, o32):
    """device error against 4 x the fp32 oracle's (floor 1e-6), both printed"""
    e_dev, e_32 = vo.norm_err(dev.detach().cpu(), o64), vo.norm_err(o32, o64)
    bound = max(4.0 * e_32, 1e-6)
    print(f"{name}: device {e_dev:.2e}, oracle fp32 {e_32:.2e}, bound {bound:.2e}")
    assert tuple(dev.shape) == tuple(o64.shape), (name, tuple(dev.shape), tuple(o64.shape))
    assert e_dev <= bound, (name, e_dev, e_32, bound)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _bf16_values(t):
    return t.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def _vae(kind, **cfg):
    """a float32 module on the device holding the oracle's seeded, bf16-representable state dict (shared by the tests, never changed)"""
    from videogpa_amd.vae import AutoencoderKLCogVideoX
    arch = NARROW if kind == "narrow" else {}
    sd = vo.seeded_state_dict(**arch, seed=11 if kind == "narrow" else 12)
    vae = AutoencoderKLCogVideoX(**arch, **cfg)
    vae.load_state_dict(sd)
    return vae.cuda().requires_grad_(False).eval(), sd


def _image(shape, seed):
    return _bf16_values(torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1)


# ---------------------------------------------------------------------------------------------------------------- 1. GroupNorm + SiLU alone
@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("C", [32, 128, 512])
@pytest.mark.parametrize("hw", [(1, 1), (37, 53), (120, 181)])
def test_groupnorm_silu_elementwise(hw, C, offset):
    """N(0,1) and N(100,1) data: the second loses every digit of the variance in an E[x^2] - E[x]^2 implementation.  1, 4 and 16 channels per group;
    one pixel, one workgroup with a tail (37 x 53), and many workgroups with idle tail threads (120 x 181)."""
    from videogpa_amd import ops
    g = torch.Generator().manual_seed(C + hw[0])
    x = torch.randn(2, C, *hw, generator=g) + offset
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    eps = 1e-6
    o64 = F.silu(F.group_norm(x.double(), 32, gamma.double(), beta.double(), eps))
    o32 = F.silu(F.group_norm(x, 32, gamma, beta, eps))
    xd = _nhwc(x).cuda()
    with torch.no_grad():
        stats = ops.groupnorm_stats_f32(xd, 32, eps)
        out = ops.groupnorm_silu_f32(xd, gamma.cuda(), beta.cuda(), 32, eps, stats=stats)
        again = ops.groupnorm_stats_f32(xd[1:], 32, eps)
    _check(f"groupnorm+silu {hw} C={C} mean={offset:g}", _nchw(out), o64, o32)
    # the statistics themselves: formed in fp64 on the device and rounded once, so within 4 ulp of fp32 of the fp64 answer
    xg = x.double().reshape(2, 32, -1)
    mean64, var64 = xg.mean(dim=2), xg.var(dim=2, unbiased=False)
    rstd64 = (var64 + eps).rsqrt()
    st = stats.cpu().double()
    assert ((st[..., 0] - mean64).abs() <= 4 * 2.0 ** -24 * torch.maximum(mean64.abs(), var64.sqrt())).all()
    assert ((st[..., 1] - rstd64).abs() <= 4 * 2.0 ** -24 * rstd64).all()
    assert torch.equal(again[0], stats[1])                       # a sample's statistics do not depend on the batch


# ---------------------------------------------------------------------------------------------------------------- 2. one-sided stride-2 conv, stem
@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("hw", [(36, 52), (9, 13)])
def test_downsampler_convolution_pads_right_and_bottom_only(hw, C):
    """CogVideoXDownsample3D on even and odd sizes against the oracle's general form (temporal pooling branch, F.pad (0,1,0,1), Conv2d stride 2)"""
    from videogpa_amd import ops
    g = torch.Generator().manual_seed(C + hw[0])
    x = torch.randn(2, C, 1, *hw, generator=g)
    sd = {"d.conv.weight": torch.randn(C, C, 3, 3, generator=g) * (1.0 / (9 * C)) ** 0.5, "d.conv.bias": 0.1 * torch.randn(C, generator=g)}
    o64 = vo.downsample(vo.cast(sd, torch.float64), "d", x.double(), compress_time=True)[:, :, 0]
    o32 = vo.downsample(sd, "d", x, compress_time=True)[:, :, 0]
    assert tuple(o64.shape[2:]) == ((hw[0] - 2) // 2 + 1, (hw[1] - 2) // 2 + 1)
    with torch.no_grad():
        out = ops.conv3x3_pad_f32(_nhwc(x[:, :, 0]).cuda(), ops.pack_conv_weight(sd["d.conv.weight"]).cuda(), sd["d.conv.bias"].cuda(),
                                  stride=2, pad_lo=0, pad_hi=1)
    _check(f"downsampler {hw} C={C}", _nchw(out), o64, o32)


@pytest.mark.parametrize("stride,pads", [(1, (1, 1)), (2, (1, 1)), (1, (0, 0)), (2, (1, 0))])
def test_padded_convolution_other_paddings_residual_and_batch_independence(stride, pads):
    """the remaining forms of the entry point: centred (what every other convolution of the encoder uses, with the residual add), no padding, front
    only; 32 -> 48 channels (a partial 64-wide tile); a sample's result does not depend on the batch it is in"""
    from videogpa_amd import ops
    g = torch.Generator().manual_seed(2)
    x, w, b = torch.randn(2, 32, 9, 13, generator=g), torch.randn(48, 32, 3, 3, generator=g) / 17.0, torch.randn(48, generator=g)
    pad4 = (pads[0], pads[1], pads[0], pads[1])
    o64, o32 = F.conv2d(F.pad(x.double(), pad4), w.double(), b.double(), stride=stride), F.conv2d(F.pad(x, pad4), w, b, stride=stride)
    res = torch.randn(o32.shape, generator=g)
    xd, wd, bd = _nhwc(x).cuda(), ops.pack_conv_weight(w).cuda(), b.cuda()
    with torch.no_grad():
        out = ops.conv3x3_pad_f32(xd, wd, bd, res=_nhwc(res).cuda(), stride=stride, pad_lo=pads[0], pad_hi=pads[1])
        one = ops.conv3x3_pad_f32(xd[1:], wd, bd, res=_nhwc(res[1:]).cuda(), stride=stride, pad_lo=pads[0], pad_hi=pads[1])
    _check(f"conv stride {stride} pads {pads}", _nchw(out), o64 + res.double(), o32 + res)
    assert torch.equal(one[0], out[1])


@pytest.mark.parametrize("hw", [(36, 52), (9, 13)])
def test_stem_3_to_32_channels(hw):
    """conv_in: the causal 3x3x3 convolution of a 3-channel frame = the layout kernel (3 -> 16 channels, zero filled) + the folded 2-D weight"""
    from videogpa_amd import ops
    from videogpa_amd.vae import _fold
    g = torch.Generator().manual_seed(hw[0])
    x = torch.randn(2, 3, 1, *hw, generator=g)
    w, b = torch.randn(32, 3, 3, 3, 3, generator=g) * (1.0 / 81) ** 0.5, 0.1 * torch.randn(32, generator=g)
    o64, o32 = vo.causal_conv3d(x.double(), w.double(), b.double())[:, :, 0], vo.causal_conv3d(x, w, b)[:, :, 0]
    conv = torch.nn.Conv3d(3, 32, 3)
    with torch.no_grad():
        conv.weight.copy_(w)
        wp = _fold(conv)
        wp = torch.cat([wp, wp.new_zeros(3, 3, 13, 32)], dim=2).contiguous().cuda()
        for xin in (x[:, :, 0], x[:, :, 0].to(torch.bfloat16)):
            xin = xin.contiguous().cuda()
            lay = ops.vae_input_f32(xin)
            assert torch.equal(lay[..., :3], _nhwc(xin.float())) and not lay[..., 3:].any()
        out = ops.conv3x3_pad_f32(ops.vae_input_f32(x[:, :, 0].contiguous().cuda()), wp, b.cuda())
    _check(f"stem {hw}", _nchw(out), o64, o32)


# ---------------------------------------------------------------------------------------------------------------- 3. one resnet
def test_resnet_128_to_256_with_shortcut():
    from videogpa_amd.vae import _pack_resnet, _ResnetBlock3D, _resnet_forward
    sd = {k[len("encoder.down_blocks.1.resnets.0."):]: v for k, v in vo.seeded_state_dict(seed=5).items()
          if k.startswith("encoder.down_blocks.1.resnets.0.")}
    assert tuple(sd["conv_shortcut.weight"].shape) == (256, 128, 1, 1, 1)
    x = torch.randn(2, 128, 1, 24, 40, generator=torch.Generator().manual_seed(9))
    named = {"r." + k: v for k, v in sd.items()}
    o64, o32 = vo.resnet(vo.cast(named, torch.float64), "r", x.double(), 32, 1e-6)[:, :, 0], vo.resnet(named, "r", x, 32, 1e-6)[:, :, 0]
    r = _ResnetBlock3D(128, 256, 32, 1e-6)
    r.load_state_dict(sd)
    with torch.no_grad():
        out = _resnet_forward(_pack_resnet(r.cuda()), _nhwc(x[:, :, 0]).cuda(), 32, 1e-6)
    _check("resnet 128->256", _nchw(out), o64, o32)


# ---------------------------------------------------------------------------------------------------------------- 4. / 5. whole encoders
def _encoder_case(kind, shape, seed):
    vae, sd = _vae(kind)
    x = _image(shape, seed)
    m64, m32 = vo.encoder(vo.cast(sd, torch.float64), x.double()), vo.encoder(sd, x)
    with torch.no_grad():
        dist = vae.encode(x.cuda()).latent_dist
        gen = torch.Generator(device="cuda").manual_seed(77)
        sample = dist.sample(generator=gen)
        noise = torch.randn(sample.shape, generator=torch.Generator(device="cuda").manual_seed(77), device="cuda", dtype=vae.dtype).cpu()
    assert sample.dtype == torch.float32 and tuple(sample.shape) == (shape[0], 16, 1, m64.shape[-2], m64.shape[-1])
    mean64, logvar64, std64, sample64 = vo.gaussian(m64, noise.double())
    mean32, logvar32, std32, sample32 = vo.gaussian(m32, noise)
    tag = f"{kind} encoder {tuple(shape)}"
    _check(tag + " mean", dist.mean, mean64, mean32)
    _check(tag + " logvar", dist.logvar, logvar64, logvar32)
    _check(tag + " std", dist.std, std64, std32)
    _check(tag + " sample", sample, sample64, sample32)
    assert torch.equal(dist.mode(), dist.mean)
    assert torch.equal(dist.sample(generator=torch.Generator(device="cuda").manual_seed(77)), sample)       # a generator reproduces the draw


@pytest.mark.parametrize("shape,seed", [((2, 3, 1, 36, 52), 1), ((1, 3, 1, 64, 96), 2)])
def test_narrow_encoder(shape, seed):
    """(32,64,64,64) x 2 layers; 36 x 52 walks through odd intermediate sizes (36 -> 18 -> 9 -> 4, 52 -> 26 -> 13 -> 6)"""
    _encoder_case("narrow", shape, seed)


def test_real_width_encoder():
    """(128,256,256,512) x 3 layers, the 5B-I2V configuration, at 64 x 96"""
    _encoder_case("real", (1, 3, 1, 64, 96), 3)


def test_logvar_clamp_and_scale_in_the_sampling_kernel():
    from videogpa_amd import ops
    m = torch.zeros(1, 1, 2, 32)
    m[0, 0, 0, :16], m[0, 0, 0, 16:] = 1.0, 50.0                  # logvar above the clamp
    m[0, 0, 1, :16], m[0, 0, 1, 16:] = -2.0, -50.0                # and below
    noise = torch.ones(1, 16, 1, 1, 2)
    with torch.no_grad():
        out = ops.vae_sample(m.cuda(), noise=noise.cuda(), scale=0.5, want=("sample", "mean", "logvar", "std"))
    assert torch.equal(out["logvar"][0, :, 0, 0].cpu(), torch.tensor([20.0, -30.0]).expand(16, 2))
    want = torch.tensor([1.0 + float(torch.exp(torch.tensor(10.0))), -2.0 + float(torch.exp(torch.tensor(-15.0)))]) * 0.5
    assert torch.allclose(out["sample"][0, :, 0, 0].cpu(), want.expand(16, 2), rtol=1e-6, atol=0)
    bf = ops.vae_sample(m.cuda(), noise=noise.cuda().to(torch.bfloat16), scale=0.5, dtype=torch.bfloat16)["sample"]
    assert bf.dtype == torch.bfloat16 and torch.equal(bf.float(), out["sample"].to(torch.bfloat16).float())  # one rounding, from the fp32 value


# ---------------------------------------------------------------------------------------------------------------- 6. tiling and slicing
def _tiled_case(tag, **tiling):
    vae, sd = _vae("narrow", sample_height=64, sample_width=96)
    x = _image((1, 3, 1, 64, 96), 4)
    kw = dict(tile_sample_min_height=tiling.get("tile_sample_min_height", 32), tile_sample_min_width=tiling.get("tile_sample_min_width", 48),
              overlap_factor_height=tiling.get("tile_overlap_factor_height", 1 / 6), overlap_factor_width=tiling.get("tile_overlap_factor_width", 1 / 5))
    m64, m32 = vo.tiled_encoder(vo.cast(sd, torch.float64), x.double(), **kw), vo.tiled_encoder(sd, x, **kw)
    saved = {k: getattr(vae, k) for k in ("tile_sample_min_height", "tile_sample_min_width", "tile_latent_min_height", "tile_latent_min_width",
                                          "tile_overlap_factor_height", "tile_overlap_factor_width")}
    try:
        vae.enable_tiling(**tiling)
        with torch.no_grad():
            dist = vae.encode(x.cuda()).latent_dist
            _check(tag + " mean", dist.mean, m64[:, :16], m32[:, :16])
            _check(tag + " logvar", dist.logvar, m64[:, 16:].clamp(-30, 20), m32[:, 16:].clamp(-30, 20))
            vae.disable_tiling()
            untiled = vae.encode(x.cuda()).latent_dist.mean
        return dist.mean, untiled
    finally:
        vae.disable_tiling()
        for k, v in saved.items():
            setattr(vae, k, v)


def test_tiled_encode_default_grid():
    """sample size 64 x 96 -> tiles of 32/32/12 x 48/48/20 pixels: the 3 x 3 grid with short last tiles that 480 x 720 gives"""
    tiled, untiled = _tiled_case("tiled 3x3")
    assert tuple(tiled.shape) == (1, 16, 1, 9, 12) and tuple(untiled.shape) == (1, 16, 1, 8, 12)    # 4 + 4 + 1 rows, as upstream's crop arithmetic gives
    assert not torch.equal(tiled[:, :, :, :8], untiled)                                                 # tiling is a different function of the image


def test_tiled_encode_with_real_ramps_in_both_directions():
    """48-pixel tiles at half overlap: 3 x 4 tiles, blend extents of 3 latent pixels both ways, so the ramps and the reads of already-blended
    neighbours carry weight (the default grid at this size blends one column with weight 0)"""
    _tiled_case("tiled 3x4, overlap 1/2", tile_sample_min_height=48, tile_sample_min_width=48, tile_overlap_factor_height=0.5,
                tile_overlap_factor_width=0.5)


def test_tiling_and_slicing_switches_are_bit_identical_where_they_must_be():
    vae, _ = _vae("narrow", sample_height=64, sample_width=96)
    small, pair = _image((1, 3, 1, 32, 48), 5).cuda(), _image((2, 3, 1, 36, 52), 6).cuda()
    with torch.no_grad():
        try:
            off = vae.encode(small).latent_dist
            vae.enable_tiling()
            on = vae.encode(small).latent_dist                    # no larger than one tile: the untiled path
            vae.disable_tiling()
            assert torch.equal(on.mean, off.mean) and torch.equal(on.logvar, off.logvar)
            whole = vae.encode(pair).latent_dist
            vae.enable_slicing()
            sliced = vae.encode(pair).latent_dist
            assert torch.equal(sliced.mean, whole.mean) and torch.equal(sliced.logvar, whole.logvar)
        finally:
            vae.disable_tiling()
            vae.disable_slicing()


# ---------------------------------------------------------------------------------------------------------------- 7. the trainer's seam
def test_trainer_encodes_the_condition_image_with_the_vae():
    """image_emb through CogVideoXDPOTrainer(vae=...) == the same step fed the latent computed beforehand through the same vae, bit for bit, when the
    sampling noise is the same (the global device generator reseeded to one state); slicing / tiling come from the trainer's config"""
    from oracle import cogvideox as ocv
    from videogpa_amd.lora import LoraConfig, get_peft_model
    from videogpa_amd.trainer import CogVideoXDPOTrainer
    from videogpa_amd.transformer import CogVideoXTransformer3DModel
    from videogpa_amd.vae import AutoencoderKLCogVideoX
    kw = dict(num_attention_heads=2, attention_head_dim=64, num_layers=2, time_embed_dim=32, text_embed_dim=48, sample_width=12, sample_height=8,
              sample_frames=13, max_text_seq_length=6, in_channels=32, use_learned_positional_embeddings=True)
    cfg = ocv.CogVideoXConfig(**kw)
    model = CogVideoXTransformer3DModel(use_rotary_positional_embeddings=True, **kw)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in ocv.init_state_dict(cfg, seed=4, std=0.05, mod_std=0.2).items()}, strict=True)
    pm = get_peft_model(model.to(device="cuda", dtype=torch.bfloat16), LoraConfig(r=4, lora_alpha=8, target_modules=["to_q", "to_k", "to_v", "to_out.0"]))
    own = pm.state_dict()
    for k, v in ocv.init_lora(cfg, r=4, seed=5, b_std=0.05).items():
        own[k[:-len(".weight")] + ".default.weight"].copy_(v)
    # sample size 96 x 80 -> tiles of 48 x 40 pixels at strides 40 x 32: the 64 x 96 image is encoded as 2 x 3 tiles whose kept parts add up to 8 x 12
    vae = AutoencoderKLCogVideoX(sample_height=96, sample_width=80, **NARROW)
    vae.load_state_dict(vo.seeded_state_dict(**NARROW, seed=11))
    vae = vae.to(device="cuda", dtype=torch.bfloat16)
    tr = CogVideoXDPOTrainer({"beta": 1.0}, transformer=pm, vae=vae)
    assert tr.vae is vae and vae.use_slicing and vae.use_tiling and not any(p.requires_grad for p in vae.parameters())
    assert [len(v) for v in (vae.tile_plan(64, 96)["rows"], vae.tile_plan(64, 96)["cols"])] == [2, 3]
    g = torch.Generator().manual_seed(6)
    xw = (0.7 * torch.randn(1, 16, 4, 8, 12, generator=g)).to(torch.bfloat16).cuda()
    xl = (0.7 * torch.randn(1, 16, 4, 8, 12, generator=g)).to(torch.bfloat16).cuda()
    txt = (0.5 * torch.randn(1, 6, cfg.text_embed_dim, generator=g)).to(torch.bfloat16).cuda()
    img = torch.rand(1, 3, 40, 50, generator=g).to(torch.bfloat16).cuda()          # resized to (64, 96), nearest, inside the step
    t, eps = torch.tensor([650]).cuda(), torch.randn(1, 4, 16, 8, 12, generator=g).to(torch.bfloat16).cuda()
    torch.manual_seed(123)
    out = tr._shared_step({"x_win": xw, "x_lose": xl, "prompt_emb": txt, "image_emb": img}, timesteps=t, noise=eps)
    torch.manual_seed(123)
    with torch.no_grad():
        resized = F.interpolate(img, size=(64, 96)).unsqueeze(2)
        il = vae.encode(resized.to(vae.dtype)).latent_dist.sample() * vae.config.scaling_factor
    assert il.dtype == torch.bfloat16 and tuple(il.shape) == (1, 16, 1, 8, 12) and il.float().abs().max() > 0.1
    out1 = tr._shared_step({"x_win": xw, "x_lose": xl, "prompt_emb": txt, "image_latent": il}, timesteps=t, noise=eps)
    assert torch.isfinite(out.loss) and out1.loss.item() == out.loss.item(), (out.loss.item(), out1.loss.item())
    out0 = tr._shared_step({"x_win": xw, "x_lose": xl, "prompt_emb": txt}, timesteps=t, noise=eps)                 # zero condition: another loss
    assert out0.loss.item() != out.loss.item()
    # without a vae or an image_encoder the existing error stands
    with pytest.raises(RuntimeError, match="image_encoder"):
        CogVideoXDPOTrainer({"beta": 1.0}, transformer=pm)._shared_step({"x_win": xw, "x_lose": xl, "prompt_emb": txt, "image_emb": img},
                                                                      timesteps=t, noise=eps)
