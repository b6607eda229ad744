"""videogpa_amd.vae's decoder (with_decoder=True: latents to frames, diffusers' latent frame batches, conv cache, spatially conditioned norms,
up-samplers, tiled decode) and its three kernels against tests/vae_decoder_oracle.py, the plain-torch restatement of diffusers' scheme run on the
CPU in fp64.  -m gpu only.

Accuracy convention (tests/test_gpu_vae_video.py's): error = max |device - o64| / max |o64| per output tensor; bound = max(4 x the SAME quantity of
the oracle run in fp32 on the CPU, 1e-6), computed in the test next to the device's figure and printed.  What has to hold bit for bit (the
up-sampler against up-sampling on the host + ops.conv3x3_pad_f32, the spatial norm's gather against a modulation map resized on the host, a sample
alone against the sample in a batch, slicing, a latent that fits one tile, the bf16 module against the fp32 one rounded once, the uint8 frames) is
checked with torch.equal.

Measured on an MI355X, device error / oracle-fp32 error (every test prints its own figures and its bound):
    up-sampler                        C = 32: 1.8e-7 ... 2.5e-7 / 2.3e-7 ... 5.3e-7;  C = 128: 1.7e-7 ... 3.1e-7 / 2.6e-7 ... 3.4e-7
    spatial norm + SiLU               C = 32: 1.1e-7 ... 2.1e-7 / 1.9e-7 ... 4.0e-7;  C = 128: 1.1e-7 ... 2.1e-7 / 2.3e-7 ... 3.8e-7;
                                      C = 512: 1.2e-7 ... 2.2e-7 / 2.3e-7 ... 3.9e-7;  at 3 -> 5 frames the plain-resize oracle is 0.26 ... 0.42 away
    resnet 256 -> 128 at 6 x 10       first chunk 4.2e-7 / 4.5e-7;  second chunk, with the cache, 5.5e-7 / 4.0e-7
    narrow decoder, F = 1 ... 13      7.6e-7 ... 1.0e-6 / 1.3e-6 ... 1.9e-6;  F = 5: the oracle over the whole latent at once is 0.20 away from the batched oracle
    real-width decoder, F = 3         1.0e-6 / 1.4e-6
    tiled narrow decoder, 4 x 4 tiles 6.9e-7 / 1.4e-6
The K sum in runs of 64 products (27 * 512 products at most) is enough here too.
The CPU fp64 side of the real-width case (3 latent frames of 3 x 4 -> 9 frames of 24 x 32) takes 0.8 s.
"""
import functools
import time

import pytest
import torch
import torch.nn.functional as F

import vae_decoder_oracle as vd
import vae_oracle as vo

pytestmark = pytest.mark.gpu

NARROW = dict(block_out_channels=(32, 64, 64, 64), layers_per_block=2)
SMALL = dict(sample_height=64, sample_width=96)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _check(name, dev, o64, o32):
    """device error against 4 x the fp32 oracle's (floor 1e-6), both printed; returns the bound"""
    e_dev, e_32 = vo.norm_err(dev.detach().cpu(), o64), vo.norm_err(o32, o64)
    bound = max(4.0 * e_32, 1e-6)
    print(f"{name}: device {e_dev:.2e}, oracle fp32 {e_32:.2e}, bound {bound:.2e}")
    assert tuple(dev.shape) == tuple(o64.shape), (name, tuple(dev.shape), tuple(o64.shape))
    assert e_dev <= bound, (name, e_dev, e_32, bound)
    return bound


def _cl(x):
    """[B,C,T,H,W] -> channels-last [B,T,H,W,C] on the device"""
    return x.permute(0, 2, 3, 4, 1).contiguous().cuda()


def _cf(x):
    """channels-last [B,T,H,W,C] -> [B,C,T,H,W]"""
    return x.permute(0, 4, 1, 2, 3)


def _bf16_values(t):
    return t.to(torch.bfloat16).float()


def _latent(shape, seed):
    """a latent of unit scale, bf16-representable"""
    return _bf16_values(torch.randn(shape, generator=torch.Generator().manual_seed(seed)))


@functools.lru_cache(maxsize=None)
def _state_dict(kind):
    arch = NARROW if kind == "narrow" else {}
    return {**vo.seeded_state_dict(**arch, seed=21 if kind == "narrow" else 22), **vd.seeded_decoder_state_dict(**arch, seed=23 if kind == "narrow" else 24)}


def _new_vae(kind, dtype=torch.float32, **cfg):
    from videogpa_amd.vae import AutoencoderKLCogVideoX
    vae = AutoencoderKLCogVideoX(with_decoder=True, **(NARROW if kind == "narrow" else {}), **cfg)
    vae.load_state_dict(_state_dict(kind))
    return vae.to(device="cuda", dtype=dtype).requires_grad_(False).eval()


@functools.lru_cache(maxsize=None)
def _vae(kind, **cfg):
    """a float32 module with the decoder on the device holding the oracles' seeded, bf16-representable state dict (shared by the tests, never changed)"""
    return _new_vae(kind, **cfg), _state_dict(kind)


def _frame_source(T, To):
    """source frame of every output frame of the up-sampler"""
    return list(range(T)) if To == T else [k // 2 for k in range(To)] if To == 2 * T else [0] + [1 + (k - 1) // 2 for k in range(1, To)]


# ---------------------------------------------------------------------------------------------------------------- 1. the up-sampler
@pytest.mark.parametrize("compress_time", [True, False])
@pytest.mark.parametrize("hw", [(5, 7), (18, 26)])
@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
def test_upsampler_against_interpolate_and_conv2d_and_its_exact_properties(T, C, hw, compress_time):
    """CogVideoXUpsample3D against the oracle's F.interpolate + Conv2d, and bit for bit a nearest up-sample by index arithmetic on the host followed by
    ops.conv3x3_pad_f32 per frame.  A frame's 4 H W pixels (140, 1872) are no multiple of the 128-pixel tile: tiles straddle frames and samples."""
    from videogpa_amd import ops
    g = torch.Generator().manual_seed(100 * T + C + hw[0])
    x = torch.randn(2, C, T, *hw, generator=g)
    sd = {"u.conv.weight": torch.randn(C, C, 3, 3, generator=g) * (1.0 / (9 * C)) ** 0.5, "u.conv.bias": 0.1 * torch.randn(C, generator=g)}
    o64, o32 = vd.upsample(vo.cast(sd, torch.float64), "u", x.double(), compress_time), vd.upsample(sd, "u", x, compress_time)
    To = {1: 1, 2: 4, 3: 5, 4: 8, 5: 9}[T] if compress_time else T
    assert tuple(o64.shape) == (2, C, To, 2 * hw[0], 2 * hw[1])
    xd, wd, bd = _cl(x), ops.pack_conv_weight(sd["u.conv.weight"]).cuda(), sd["u.conv.bias"].cuda()
    with torch.no_grad():
        out = ops.vae_upsample_f32(xd, wd, bd, compress_time=compress_time)
        yi, xi = torch.arange(2 * hw[0], device="cuda") // 2, torch.arange(2 * hw[1], device="cuda") // 2
        up = xd[:, _frame_source(T, To)][:, :, yi][:, :, :, xi]
        host = ops.conv3x3_pad_f32(up.reshape(2 * To, 2 * hw[0], 2 * hw[1], C).contiguous(), wd, bd)
        alone = ops.vae_upsample_f32(xd[1:].contiguous(), wd, bd, compress_time=compress_time)
    _check(f"up-sampler T={T} C={C} {hw} compress_time={compress_time}", _cf(out), o64, o32)
    assert torch.equal(out, host.reshape(out.shape))
    assert torch.equal(alone[0], out[1])


# ---------------------------------------------------------------------------------------------------------------- 2. the spatial norm
TIME_PAIRS = [(1, 1), (2, 2), (3, 3), (2, 4), (3, 5), (2, 8), (3, 9)]           # (latent frames, feature frames) as the decoder meets them


def _time_source(t, T):
    return [0] + [1 + ((k - 1) * (t - 1)) // (T - 1) for k in range(1, T)] if T > 1 and T % 2 else [(k * t) // T for k in range(T)]


@pytest.mark.parametrize("ratio", [1, 2, 4, 8])
@pytest.mark.parametrize("C", [32, 128, 512])
def test_spatial_norm_silu_against_the_oracle_and_the_commuting_claim(C, ratio):
    """1, 4 and 16 channels per group; a 3 x 5 latent under a map `ratio` times its size, every (latent frames, feature frames) pair of the decoder.
    The kernel gathers (Y | B) from the latent-resolution map; fed the map resized to full resolution on the host it must give the same bits: a
    1x1 convolution commutes with a nearest-neighbour resize."""
    from videogpa_amd import ops
    from videogpa_amd.vae import _pack_spatial_norm, _SpatialNorm3D
    g = torch.Generator().manual_seed(10 * C + ratio)
    sd = {}
    for k, v in vd.seeded_decoder_state_dict(block_out_channels=(C, 32, 32, 32), layers_per_block=0, seed=C).items():      # norm_out is C wide
        if k.startswith("decoder.norm_out."):
            sd["n." + k[len("decoder.norm_out."):]] = v
    sd64 = vo.cast(sd, torch.float64)
    norm = _SpatialNorm3D(C, 16, 32)
    norm.load_state_dict({k[2:]: v for k, v in sd.items()})
    p = _pack_spatial_norm(norm.cuda())
    H, W = 3 * ratio, 5 * ratio
    for t, T in TIME_PAIRS:
        f, zq = torch.randn(2, C, T, H, W, generator=g) * 1.5 + 0.3, torch.randn(2, 16, t, 3, 5, generator=g)
        o64, o32 = F.silu(vd.spatial_norm(sd64, "n", f.double(), zq.double(), 32)), F.silu(vd.spatial_norm(sd, "n", f, zq, 32))
        fd, zd = _cl(f), _cl(zq)
        with torch.no_grad():
            stats = ops.groupnorm_stats_f32(fd, 32, 1e-6)
            yb = ops.conv1x1_f32(zd, *p["yb"])
            out = ops.spatial_norm_silu_f32(fd, stats, *p["gn"], yb)
            yi, xi = torch.arange(H, device="cuda") // ratio, torch.arange(W, device="cuda") // ratio
            full = yb[:, _time_source(t, T)][:, :, yi][:, :, :, xi].contiguous()
            assert tuple(yb.shape) == (2, t, 3, 5, 2 * C) and tuple(full.shape) == (2, T, H, W, 2 * C)
            assert torch.equal(ops.spatial_norm_silu_f32(fd, stats, *p["gn"], full), out), (t, T)
            assert torch.equal(ops.spatial_norm_silu_f32(fd[1:].contiguous(), stats[1:].contiguous(), *p["gn"], yb[1:].contiguous())[0], out[1])
        bound = _check(f"spatial norm C={C} x{ratio} frames {t}->{T}", _cf(out), o64, o32)
        if (t, T) == (3, 5):
            # the test can tell the odd-frame split from a plain resize
            apart = vo.norm_err(F.silu(vd.spatial_norm(sd64, "n", f.double(), zq.double(), 32, split=False)), o64)
            print(f"spatial norm C={C} x{ratio}: the plain-resize oracle is {apart:.3g} away (bound {bound:.2e})")
            assert apart > 100 * bound


# ---------------------------------------------------------------------------------------------------------------- 3. one decoder resnet
def test_decoder_resnet_256_to_128_with_shortcut_with_and_without_cache():
    """two chunks of T = 3 and T = 2 at 6 x 10 over a 3 x 5 latent: the first without a cache (frame 0 replicated), the second with the cache the first left"""
    from videogpa_amd.vae import _ConvCache, _decoder_resnet_forward, _DecoderResnetBlock3D, _pack_decoder_resnet
    prefix = "decoder.up_blocks.3.resnets.0."
    sd = {k[len(prefix):]: v for k, v in vd.seeded_decoder_state_dict(seed=5).items() if k.startswith(prefix)}
    assert tuple(sd["conv_shortcut.weight"].shape) == (128, 256, 1, 1, 1)
    g = torch.Generator().manual_seed(9)
    x, zq = torch.randn(2, 256, 5, 6, 10, generator=g), torch.randn(2, 16, 5, 3, 5, generator=g)
    named = {"r." + k: v for k, v in sd.items()}
    named64 = vo.cast(named, torch.float64)
    a64, c64 = vd.resnet(named64, "r", x[:, :, :3].double(), zq[:, :, :3].double(), 32)
    b64, _ = vd.resnet(named64, "r", x[:, :, 3:].double(), zq[:, :, 3:].double(), 32, c64)
    a32, c32 = vd.resnet(named, "r", x[:, :, :3], zq[:, :, :3], 32)
    b32, _ = vd.resnet(named, "r", x[:, :, 3:], zq[:, :, 3:], 32, c32)
    r = _DecoderResnetBlock3D(256, 128, 16, 32)
    r.load_state_dict(sd)
    r = r.cuda()
    with torch.no_grad():
        p = _pack_decoder_resnet(r)
        first = _ConvCache()
        a = _decoder_resnet_forward(p, "r", _cl(x[:, :, :3]), _cl(zq[:, :, :3]), 32, first)
        second = _ConvCache(first)
        b = _decoder_resnet_forward(p, "r", _cl(x[:, :, 3:]), _cl(zq[:, :, 3:]), 32, second)
        no_cache = _decoder_resnet_forward(p, "r", _cl(x[:, :, 3:]), _cl(zq[:, :, 3:]), 32, _ConvCache())
    _check("decoder resnet 256->128, first chunk", _cf(a), a64, a32)
    _check("decoder resnet 256->128, second chunk with the cache", _cf(b), b64, b32)
    assert sorted(first.new) == ["r.conv1", "r.conv2"] and tuple(first.new["r.conv1"].shape) == (2, 2, 6, 10, 256)
    assert not torch.equal(b, no_cache)                                                                       # the cache carries weight


# ---------------------------------------------------------------------------------------------------------------- 4. / 5. whole decoders
def _decoder_case(kind, shape, seed):
    vae, sd = _vae(kind)
    z = _latent(shape, seed)
    t0 = time.perf_counter()
    o64 = vd.batched_decoder(vo.cast(sd, torch.float64), z.double())
    seconds64 = time.perf_counter() - t0
    o32 = vd.batched_decoder(sd, z)
    with torch.no_grad():
        out = vae.decode(z.cuda())
        sample = out.sample
        assert vae.decode(z.cuda(), return_dict=False)[0].shape == sample.shape
    assert sample.dtype == torch.float32 and type(out).__name__ == "DecoderOutput"
    bound = _check(f"{kind} decoder {tuple(shape)} (CPU fp64 {seconds64:.1f} s)", sample, o64, o32)
    return z, o64, bound


@pytest.mark.parametrize("shape,seed,frames", [((2, 16, 3, 5, 7), 1, 9), ((1, 16, 5, 5, 7), 2, 17), ((1, 16, 13, 3, 4), 3, 49), ((1, 16, 1, 5, 7), 4, 1),
                                               ((1, 16, 2, 5, 7), 5, 8)])
def test_narrow_decoder_on_latents(shape, seed, frames):
    """(64,64,64,32) x 3 resnets.  3 latent frames are one batch (9 frames); 5 = 3 + 2 and 13 = 3 + 5 x 2 hand the conv cache on; 1 and 2 latent
    frames take the up-samplers' one-frame and even-count branches."""
    z, o64, bound = _decoder_case("narrow", shape, seed)
    assert tuple(o64.shape) == (shape[0], 3, frames, 8 * shape[3], 8 * shape[4])
    if shape[2] == 5:
        # the test can tell a correct frame batching from none: the oracle over the whole latent at once is another function
        _, sd = _vae("narrow")
        whole = vd.decoder(vo.cast(sd, torch.float64), z.double())[0]
        assert whole.shape == o64.shape
        apart = vo.norm_err(whole, o64)
        print(f"whole-latent oracle against the batched oracle: {apart:.3g} (bound {bound:.2e})")
        assert apart > 100 * bound


def test_real_width_decoder():
    """(512,256,256,128) x 4 resnets, the 5B configuration: 3 latent frames of 3 x 4 -> 9 frames of 24 x 32.  The CPU fp64 oracle of this case
    takes 0.8 s (printed with the figures)."""
    _, o64, _ = _decoder_case("real", (1, 16, 3, 3, 4), 6)
    assert tuple(o64.shape) == (1, 3, 9, 24, 32)


# ---------------------------------------------------------------------------------------------------------------- 6. tiling and slicing
def test_tiled_decode():
    """sample size 64 x 96 -> latent tiles of 4 x 6 at strides 3 and 4, blends over 5 and 9 sample pixels: a 10 x 14 latent is 4 x 4 tiles with short
    last ones, each decoded by the frame-batch loop with a cache of its own"""
    vae, sd = _vae("narrow", **SMALL)
    z = _latent((1, 16, 3, 10, 14), 7)
    kw = dict(tile_sample_min_height=32, tile_sample_min_width=48)
    o64, o32 = vd.tiled_batched_decoder(vo.cast(sd, torch.float64), z.double(), **kw), vd.tiled_batched_decoder(sd, z, **kw)
    small = _latent((1, 16, 3, 4, 6), 8).cuda()
    try:
        with torch.no_grad():
            untiled, small_off = vae.decode(z.cuda()).sample, vae.decode(small).sample
            vae.enable_tiling()
            tiled, small_on = vae.decode(z.cuda()).sample, vae.decode(small).sample
    finally:
        vae.disable_tiling()
    _check("tiled narrow decoder 4x4 tiles", tiled, o64, o32)
    assert tuple(untiled.shape) == (1, 3, 9, 80, 112)
    common = (slice(None),) * 3 + (slice(0, min(tiled.shape[3], 80)), slice(0, min(tiled.shape[4], 112)))
    assert not torch.equal(tiled[common], untiled[common])
    assert torch.equal(small_on, small_off)                                 # no larger than one tile: the untiled path


def test_slicing_is_bit_identical():
    vae, _ = _vae("narrow")
    pair = _latent((2, 16, 3, 5, 7), 9).cuda()
    try:
        with torch.no_grad():
            whole = vae.decode(pair).sample
            vae.enable_slicing()
            sliced = vae.decode(pair).sample
    finally:
        vae.disable_slicing()
    assert tuple(whole.shape) == (2, 3, 9, 40, 56) and torch.equal(sliced, whole)


# ---------------------------------------------------------------------------------------------------------------- 7. the pipeline's expression
def test_decode_latents_on_a_bfloat16_module_with_slicing_and_tiling():
    """generate/CogVideoX-5B.py: `pipe.vae.enable_tiling(); pipe.vae.enable_slicing()`, then the pipeline's decode_latents.  The bf16 module computes in
    fp32 from bf16-representable weights, so it is the fp32 module's result rounded once."""
    from videogpa_amd import generate
    vae32, vae16 = _new_vae("narrow", **SMALL), _new_vae("narrow", torch.bfloat16, **SMALL)
    for vae in (vae32, vae16):
        vae.enable_tiling()
        vae.enable_slicing()
    latents = (0.7 * torch.randn(2, 3, 16, 10, 14, generator=torch.Generator().manual_seed(10))).to(torch.bfloat16).cuda()
    frames = generate.decode_latents(vae16, latents)
    with torch.no_grad():
        z = (1 / vae16.config.scaling_factor) * latents.permute(0, 2, 1, 3, 4)
        want = vae32.decode(z.float()).sample
    assert frames.dtype == torch.bfloat16 and frames.shape == want.shape and frames.shape[:3] == (2, 3, 9) and torch.isfinite(frames.float()).all()
    assert torch.equal(frames, want.to(torch.bfloat16))
    # the uint8 frames of the same call, from the fp32 frames: [B,F',H,W,3]
    u8 = generate.decode_latents(vae16, latents, uint8=True)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (2, 9) + tuple(want.shape[3:]) + (3,)
    v = (want.permute(0, 2, 3, 4, 1) / 2 + 0.5).clamp(0, 1) * 255
    diff, at_a_tie = (u8.float() - v.round()).abs(), ((v - v.floor()) - 0.5).abs() <= 1e-6
    assert bool(((diff == 0) | (at_a_tie & (diff <= 1))).all())            # +-1 only within 1e-6 of a .5 boundary (the exact comparison is section 8's)


def test_forward_is_encode_mode_decode():
    vae, _ = _vae("narrow")
    x = _bf16_values(torch.rand(1, 3, 9, 16, 24, generator=torch.Generator().manual_seed(11)) * 2 - 1).cuda()      # 9 frames -> 3 latent frames -> 9 frames
    with torch.no_grad():
        dist = vae.encode(x).latent_dist
        assert torch.equal(vae(x).sample, vae.decode(dist.mode()).sample)
        gen = lambda: torch.Generator(device="cuda").manual_seed(5)
        assert torch.equal(vae(x, sample_posterior=True, generator=gen()).sample, vae.decode(dist.sample(generator=gen())).sample)
        assert tuple(vae(x).sample.shape) == (1, 3, 9, 16, 24)


# ---------------------------------------------------------------------------------------------------------------- 8. the output kernel
def test_vae_output_layouts_and_the_uint8_form_exactly():
    from videogpa_amd import ops
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 3, 9, 11, 16, generator=g) * 0.8
    x[0, 0, 0, 0, :3] = torch.tensor([-1.0, 1.0, 0.25])
    x[0, 0, 0, 1, :3] = torch.tensor([-3.0, 3.0, 0.999])
    xd = x.cuda()
    with torch.no_grad():
        assert torch.equal(ops.vae_output(xd), xd[..., :3].permute(0, 4, 1, 2, 3))
        assert torch.equal(ops.vae_output(xd, torch.bfloat16), xd[..., :3].permute(0, 4, 1, 2, 3).to(torch.bfloat16))
        assert torch.equal(ops.vae_input_f32(ops.vae_output(xd)[:, :, 0].contiguous())[..., :3], xd[:, 0, :, :, :3])      # the inverse of vae_input_f32
        u8 = ops.vae_output(xd, uint8=True)
    v = (x[..., :3] / 2 + 0.5).clamp(0, 1) * 255                            # fp32, as the pipeline's postprocess_video
    assert float(((v - v.floor()) - 0.5).abs().min()) > 1e-6               # no value at a .5 boundary: the comparison below is exact
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (2, 3, 9, 11, 3)
    assert torch.equal(u8.cpu(), v.round().to(torch.uint8))
    assert u8[0, 0, 0, 0].tolist() == [0, 255, 159] and u8[0, 0, 0, 1].tolist()[:2] == [0, 255]
    assert int((u8 == 0).sum()) > 10 and int((u8 == 255).sum()) > 10          # both clamps are met


# ---------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals():
    from videogpa_amd import ops
    from videogpa_amd.vae import AutoencoderKLCogVideoX
    vae, _ = _vae("narrow")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vae.decode(torch.zeros(1, 16, 1, 2, 2))
    with pytest.raises(NotImplementedError, match="use_post_quant_conv"):
        AutoencoderKLCogVideoX(with_decoder=True, use_post_quant_conv=True, **NARROW)
    with pytest.raises(NotImplementedError, match="with_decoder=True"):
        AutoencoderKLCogVideoX(**NARROW).cuda().decode(torch.zeros(1, 16, 1, 2, 2, device="cuda"))
    dev = lambda *s: torch.zeros(*s, device="cuda")
    f, stats, gb = dev(1, 2, 6, 10, 32), dev(1, 32, 2), dev(32)
    with pytest.raises(RuntimeError, match="integral"):
        ops.spatial_norm_silu_f32(f, stats, gb, gb, dev(1, 2, 4, 5, 64))          # 6 rows over 4
    with pytest.raises(RuntimeError, match="integral"):
        ops.spatial_norm_silu_f32(f, stats, gb, gb, dev(1, 2, 3, 3, 64))          # 10 columns over 3
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.spatial_norm_silu_f32(f, stats, gb, gb, dev(1, 2, 3, 5, 32))          # (Y | B) holds 2C channels
    with pytest.raises(RuntimeError, match="frames"):
        ops.spatial_norm_silu_f32(dev(1, 3, 6, 10, 32), stats, gb, gb, dev(1, 1, 3, 5, 64))      # an odd count needs a latent frame behind frame 0
    with pytest.raises(RuntimeError, match="weight"):
        ops.vae_upsample_f32(dev(1, 2, 4, 4, 16), dev(3, 3, 32, 32))
    with pytest.raises(RuntimeError, match=r"\[N,T,H,W,16\]"):
        ops.vae_output(dev(1, 2, 4, 4, 3))
