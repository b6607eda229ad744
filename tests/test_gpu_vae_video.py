"""videogpa_amd.vae on clips (the CogVideoX VAE encoder over F = 4k + 1 frames: frame batches, conv cache, temporal pooling) and its two kernels
against tests/vae_video_oracle.py, the plain-torch restatement of diffusers' scheme run on the CPU in fp64.  -m gpu only.

Accuracy convention (tests/test_gpu_vae.py's): error = max |device - o64| / max |o64| per output tensor; bound = max(4 x the SAME quantity of the
oracle run in fp32 on the CPU, 1e-6), computed in the test next to the device's figure and printed.  What has to hold bit for bit (a clip in one call
against its split into two with the cache handed on, a sample alone against the sample in a batch, pooling in the loader against pooling on the
host, slicing, a clip that fits one tile) is checked with torch.equal.

Measured on an MI355X, device error / oracle-fp32 error (every test prints its own figures and its bound):
    causal convolution alone          16 -> 32: 0.8e-7 ... 1.6e-7 / 1.6e-7 ... 3.9e-7;  32 -> 48: 1.1e-7 ... 2.3e-7 / 3.4e-7 ... 8.2e-7;
                                      128 -> 128: 2.0e-7 ... 4.1e-7 / 3.1e-7 ... 5.8e-7 (T = 1, 2, 3, 5; with and without prev and res; both sizes)
                                      T = 1 against the folded 2-D convolution: 1.8e-7 ... 4.4e-7 of max |o64| apart
    downsampler                       C = 32: 1.5e-7 ... 3.0e-7 / 2.0e-7 ... 4.6e-7;  C = 128: 1.7e-7 ... 3.0e-7 / 2.2e-7 ... 3.5e-7
    resnet 128 -> 256 at 12 x 20      first chunk 3.6e-7 / 3.9e-7;  second chunk, with the cache, 3.8e-7 / 4.4e-7
    narrow encoder, F = 5 ... 21      mean 5.8e-7 ... 8.2e-7 / 0.9e-6 ... 1.3e-6, logvar 5.9e-7 ... 9.1e-7 / 0.9e-6 ... 1.5e-6,
                                      std 3.2e-7 ... 4.0e-7 / 3.9e-7 ... 9.8e-7, sample 2.1e-7 ... 4.7e-7 / 3.6e-7 ... 7.8e-7
                                      F = 17: the oracle over the whole clip at once is 0.22 away from the batched oracle
    real-width encoder, F = 9         mean 6.8e-7 / 1.1e-6, logvar 9.3e-7 / 1.5e-6, std 5.1e-7 / 9.7e-7, sample 6.7e-7 / 8.7e-7
    tiled narrow encoder, F = 9       3 x 3 grid: mean 7.8e-7 / 1.2e-6, logvar 6.3e-7 / 1.1e-6;  3 x 4 at half overlap: mean 6.6e-7 / 9.9e-7, logvar 6.1e-7 / 8.6e-7
The K sum in runs of 64 products (27 * 512 products at most) is enough: no total per temporal tap was needed.
The CPU fp64 side of the real-width case (F = 9 at 32 x 48) takes 1.6 s.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import vae_oracle as vo
import vae_video_oracle as vv

pytestmark = pytest.mark.gpu

NARROW = dict(block_out_channels=(32, 64, 64, 64), layers_per_block=2)


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


@functools.lru_cache(maxsize=None)
def _vae(kind, **cfg):
    """a float32 module on the device holding the oracle's seeded, bf16-representable state dict (shared by the tests, never changed)"""
    from videogpa_amd.vae import AutoencoderKLCogVideoX
    arch = NARROW if kind == "narrow" else {}
    sd = vo.seeded_state_dict(**arch, seed=11 if kind == "narrow" else 12)
    vae = AutoencoderKLCogVideoX(**arch, **cfg)
    vae.load_state_dict(sd)
    return vae.cuda().requires_grad_(False).eval(), sd


def _clip(shape, seed):
    """uniform in [-1, 1], bf16-representable"""
    return _bf16_values(torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1)


# ---------------------------------------------------------------------------------------------------------------- 1. the causal convolution alone
def _ref_causal(x, w, b, prev):
    """F.conv3d behind the two frames in front: `prev`, or frame 0 twice"""
    front = prev if prev is not None else torch.cat([x[:, :, :1]] * 2, dim=2)
    return F.conv3d(F.pad(torch.cat([front, x], dim=2), (1, 1, 1, 1)), w, b)


@pytest.mark.parametrize("T", [1, 2, 3, 5])
@pytest.mark.parametrize("hw", [(9, 13), (36, 52)])
@pytest.mark.parametrize("cin,cout", [(16, 32), (32, 48), (128, 128)])
def test_causal_conv_against_conv3d_and_its_exact_properties(cin, cout, hw, T):
    """(16,32) is the stem's form (3 real channels, 13 zero ones, zero weight rows), (32,48) a partial 64-wide tile, (128,128) the 128-wide tile.
    At 9 x 13, M = 2 T 117 is no multiple of 128: tiles straddle frame and sample boundaries."""
    from videogpa_amd import ops
    g = torch.Generator().manual_seed(1000 * cin + 10 * hw[0] + T)
    real = 3 if cin == 16 else cin
    x, prev = torch.randn(2, real, T, *hw, generator=g), torch.randn(2, real, 2, *hw, generator=g)
    w, b = torch.randn(cout, real, 3, 3, 3, generator=g) * (1.0 / (27 * real)) ** 0.5, 0.1 * torch.randn(cout, generator=g)
    res = torch.randn(2, cout, T, *hw, generator=g)
    zeros = (lambda t, dim: torch.cat([t, t.new_zeros(*t.shape[:dim], cin - real, *t.shape[dim + 1:])], dim=dim)) if real != cin else (lambda t, dim: t)
    xd, pd, wd, bd, rd = _cl(zeros(x, 1)), _cl(zeros(prev, 1)), ops.pack_conv3d_weight(zeros(w, 1)).cuda(), b.cuda(), _cl(res)
    assert tuple(wd.shape) == (3, 3, 3, cin, cout)
    outs = {}
    with torch.no_grad():
        for with_prev in (False, True):
            o64 = _ref_causal(x.double(), w.double(), b.double(), prev.double() if with_prev else None)
            o32 = _ref_causal(x, w, b, prev if with_prev else None)
            for with_res in (False, True):
                out = ops.conv3d_causal_f32(xd, wd, bd, res=rd if with_res else None, prev=pd if with_prev else None)
                outs[with_prev, with_res] = out
                bound = _check(f"causal conv {cin}->{cout} {hw} T={T} prev={with_prev} res={with_res}", _cf(out),
                               o64 + res.double() if with_res else o64, o32 + res if with_res else o32)
            if T == 1 and not with_prev:
                # one frame, replicated: the folded 2-D convolution, in another order of summation
                folded = ops.conv3x3_pad_f32(xd[:, 0], ops.pack_conv_weight(zeros(w, 1).sum(dim=2)).cuda(), bd)
                diff = float((folded.double() - outs[False, False][:, 0].double()).abs().max().cpu() / o64.abs().max())
                print(f"causal conv {cin}->{cout} {hw} T=1 against the folded 2-D convolution: {diff:.2e}, bound {bound:.2e}")
                assert diff <= bound
        # prev = frame 0 twice is prev = None
        twice = torch.cat([xd[:, :1]] * 2, dim=1).contiguous()
        assert torch.equal(ops.conv3d_causal_f32(xd, wd, bd, res=rd, prev=twice), outs[False, True])
        # sample 1 alone is sample 1 inside the batch
        assert torch.equal(ops.conv3d_causal_f32(xd[1:], wd, bd, res=rd[1:], prev=pd[1:])[0], outs[True, True][1])
        assert torch.equal(ops.conv3d_causal_f32(xd[1:], wd, bd)[0], outs[False, False][1])
        if T == 5:
            # one call over the frames is any split into two, the second given the first's last two INPUT frames
            for cut in (2, 3):
                for with_prev in (False, True):
                    first = ops.conv3d_causal_f32(xd[:, :cut].contiguous(), wd, bd, res=rd[:, :cut].contiguous(), prev=pd if with_prev else None)
                    second = ops.conv3d_causal_f32(xd[:, cut:].contiguous(), wd, bd, res=rd[:, cut:].contiguous(),
                                                   prev=xd[:, cut - 2:cut].contiguous())
                    assert torch.equal(torch.cat([first, second], dim=1), outs[with_prev, True]), (cut, with_prev)


def test_causal_conv_refuses_what_it_cannot_run():
    from videogpa_amd import ops
    x, w = torch.zeros(1, 2, 4, 4, 16, device="cuda"), torch.zeros(3, 3, 3, 16, 32, device="cuda")
    with pytest.raises(RuntimeError, match="prev"):
        ops.conv3d_causal_f32(x, w, prev=torch.zeros(1, 1, 4, 4, 16, device="cuda"))
    with pytest.raises(RuntimeError, match="weight"):
        ops.conv3d_causal_f32(x, torch.zeros(3, 3, 16, 32, device="cuda"))
    with pytest.raises(RuntimeError, match="residual"):
        ops.conv3d_causal_f32(x, w, res=torch.zeros(1, 2, 4, 4, 16, device="cuda"))
    with pytest.raises(RuntimeError, match="too small"):
        ops.vae_downsample_f32(torch.zeros(1, 2, 1, 4, 16, device="cuda"), torch.zeros(3, 3, 16, 16, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- 2. the downsampler
def _host_pool(x):
    """x [N,T,H,W,C] on the device -> the temporally pooled [N,(T+1)//2,H,W,C], (a + b) * 0.5 in fp32 (frame 0 of an odd count kept aside)"""
    T = x.shape[1]
    if T % 2:
        return torch.cat([x[:, :1], (x[:, 1::2] + x[:, 2::2]) * 0.5], dim=1)
    return (x[:, 0::2] + x[:, 1::2]) * 0.5


@pytest.mark.parametrize("compress_time", [True, False])
@pytest.mark.parametrize("hw", [(9, 13), (36, 52)])
@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 8, 9])
def test_downsampler_with_temporal_pooling(T, C, hw, compress_time):
    """CogVideoXDownsample3D against the oracle's avg_pool1d + pad + Conv2d, and bit for bit pooling on the host + ops.conv3x3_pad_f32"""
    from videogpa_amd import ops
    g = torch.Generator().manual_seed(100 * T + C + hw[0])
    x = torch.randn(2, C, T, *hw, generator=g)
    sd = {"d.conv.weight": torch.randn(C, C, 3, 3, generator=g) * (1.0 / (9 * C)) ** 0.5, "d.conv.bias": 0.1 * torch.randn(C, generator=g)}
    o64, o32 = vo.downsample(vo.cast(sd, torch.float64), "d", x.double(), compress_time), vo.downsample(sd, "d", x, compress_time)
    To = (T + 1) // 2 if compress_time else T
    assert tuple(o64.shape) == (2, C, To, (hw[0] - 2) // 2 + 1, (hw[1] - 2) // 2 + 1)
    xd, wd, bd = _cl(x), ops.pack_conv_weight(sd["d.conv.weight"]).cuda(), sd["d.conv.bias"].cuda()
    with torch.no_grad():
        out = ops.vae_downsample_f32(xd, wd, bd, compress_time=compress_time)
        pooled = _host_pool(xd) if compress_time else xd
        host = ops.conv3x3_pad_f32(pooled.reshape(2 * To, *pooled.shape[2:]).contiguous(), wd, bd, stride=2, pad_lo=0, pad_hi=1)
    _check(f"downsampler T={T} C={C} {hw} compress_time={compress_time}", _cf(out), o64, o32)
    assert torch.equal(out, host.reshape(out.shape))


# ---------------------------------------------------------------------------------------------------------------- 3. one resnet
def test_resnet_128_to_256_with_shortcut_with_and_without_cache():
    """two chunks of T = 3 at 12 x 20: the first without a cache (frame 0 replicated), the second with the cache the first left"""
    from videogpa_amd.vae import _ConvCache, _pack3d, _pack_resnet, _ResnetBlock3D, _resnet_forward_video
    sd = {k[len("encoder.down_blocks.1.resnets.0."):]: v for k, v in vo.seeded_state_dict(seed=5).items()
          if k.startswith("encoder.down_blocks.1.resnets.0.")}
    assert tuple(sd["conv_shortcut.weight"].shape) == (256, 128, 1, 1, 1)
    x = torch.randn(2, 128, 6, 12, 20, generator=torch.Generator().manual_seed(9))
    named = {"r." + k: v for k, v in sd.items()}
    named64 = vo.cast(named, torch.float64)
    a64, c64 = vv.resnet(named64, "r", x[:, :, :3].double(), 32, 1e-6)
    b64, _ = vv.resnet(named64, "r", x[:, :, 3:].double(), 32, 1e-6, c64)
    a32, c32 = vv.resnet(named, "r", x[:, :, :3], 32, 1e-6)
    b32, _ = vv.resnet(named, "r", x[:, :, 3:], 32, 1e-6, c32)
    r = _ResnetBlock3D(128, 256, 32, 1e-6)
    r.load_state_dict(sd)
    r = r.cuda()
    with torch.no_grad():
        p, w3 = _pack_resnet(r), (_pack3d(r.conv1.conv), _pack3d(r.conv2.conv))
        first = _ConvCache()
        a = _resnet_forward_video(p, w3, "r", _cl(x[:, :, :3]), 32, 1e-6, first)
        second = _ConvCache(first)
        b = _resnet_forward_video(p, w3, "r", _cl(x[:, :, 3:]), 32, 1e-6, second)
    _check("resnet 128->256, first chunk", _cf(a), a64, a32)
    _check("resnet 128->256, second chunk with the cache", _cf(b), b64, b32)
    assert sorted(first.new) == ["r.conv1", "r.conv2"] and tuple(first.new["r.conv2"].shape) == (2, 2, 12, 20, 256)
    assert not torch.equal(b, _resnet_forward_video(p, w3, "r", _cl(x[:, :, 3:]), 32, 1e-6, _ConvCache()))      # the cache carries weight


# ---------------------------------------------------------------------------------------------------------------- 4. / 5. whole encoders
def _encoder_case(kind, shape, seed):
    vae, sd = _vae(kind)
    x = _clip(shape, seed)
    m64, m32 = vv.batched_encoder(vo.cast(sd, torch.float64), x.double()), vv.batched_encoder(sd, x)
    with torch.no_grad():
        dist = vae.encode(x.cuda()).latent_dist
        sample = dist.sample(generator=torch.Generator(device="cuda").manual_seed(77))
        noise = torch.randn(sample.shape, generator=torch.Generator(device="cuda").manual_seed(77), device="cuda", dtype=vae.dtype).cpu()
    frames = (shape[2] - 1) // 4 + 1
    assert sample.dtype == torch.float32 and tuple(sample.shape) == (shape[0], 16, frames, m64.shape[-2], m64.shape[-1])
    mean64, logvar64, std64, sample64 = vo.gaussian(m64, noise.double())
    mean32, logvar32, std32, sample32 = vo.gaussian(m32, noise)
    tag = f"{kind} encoder {tuple(shape)}"
    bound = _check(tag + " mean", dist.mean, mean64, mean32)
    _check(tag + " logvar", dist.logvar, logvar64, logvar32)
    _check(tag + " std", dist.std, std64, std32)
    _check(tag + " sample", sample, sample64, sample32)
    assert torch.equal(dist.mode(), dist.mean)
    assert torch.equal(dist.sample(generator=torch.Generator(device="cuda").manual_seed(77)), sample)       # a generator reproduces the draw
    return x, mean64, bound


@pytest.mark.parametrize("shape,seed", [((2, 3, 5, 20, 28), 1), ((1, 3, 9, 36, 52), 2), ((1, 3, 13, 20, 28), 3), ((1, 3, 17, 36, 52), 4),
                                        ((1, 3, 21, 20, 28), 5)])
def test_narrow_encoder_on_clips(shape, seed):
    """(32,64,64,64) x 2 layers.  5, 9 and 13 frames are one batch; 17 = 9 + 8 and 21 = 13 + 8 hand the conv cache on.  36 x 52 walks through odd
    intermediate sizes."""
    x, mean64, bound = _encoder_case("narrow", shape, seed)
    if shape[2] == 17:
        # the test can tell a correct frame batching from none: the oracle over the whole clip at once (one GroupNorm over 17 frames) is another function
        _, sd = _vae("narrow")
        whole = vo.gaussian(vo.encoder(vo.cast(sd, torch.float64), x.double()))[0]
        apart = vo.norm_err(whole, mean64)
        print(f"whole-clip oracle against the batched oracle: {apart:.3g} (bound {bound:.2e})")
        assert apart > 100 * bound


def test_real_width_encoder_on_a_clip():
    """(128,256,256,512) x 3 layers, the 5B configuration, 9 frames at 32 x 48"""
    _encoder_case("real", (1, 3, 9, 32, 48), 6)


# ---------------------------------------------------------------------------------------------------------------- 6. tiling and slicing
def _tiled_case(tag, **tiling):
    vae, sd = _vae("narrow", sample_height=64, sample_width=96)
    x = _clip((1, 3, 9, 64, 96), 7)
    kw = dict(tile_sample_min_height=tiling.get("tile_sample_min_height", 32), tile_sample_min_width=tiling.get("tile_sample_min_width", 48),
              overlap_factor_height=tiling.get("tile_overlap_factor_height", 1 / 6), overlap_factor_width=tiling.get("tile_overlap_factor_width", 1 / 5))
    m64, m32 = vv.tiled_batched_encoder(vo.cast(sd, torch.float64), x.double(), **kw), vv.tiled_batched_encoder(sd, x, **kw)
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


def test_tiled_clip_default_grid():
    """sample size 64 x 96 -> the 3 x 3 grid with short last tiles that 480 x 720 gives, 9 frames -> 3 latent frames"""
    tiled, untiled = _tiled_case("tiled clip 3x3")
    assert tuple(tiled.shape) == (1, 16, 3, 9, 12) and tuple(untiled.shape) == (1, 16, 3, 8, 12)
    assert not torch.equal(tiled[:, :, :, :8], untiled)


def test_tiled_clip_with_real_ramps_in_both_directions():
    """48-pixel tiles at half overlap: 3 x 4 tiles, blend extents of 3 latent pixels both ways, per frame"""
    _tiled_case("tiled clip 3x4, overlap 1/2", tile_sample_min_height=48, tile_sample_min_width=48, tile_overlap_factor_height=0.5,
                tile_overlap_factor_width=0.5)


def test_tiling_and_slicing_of_clips_are_bit_identical_where_they_must_be():
    vae, _ = _vae("narrow", sample_height=64, sample_width=96)
    small, pair = _clip((1, 3, 9, 32, 48), 8).cuda(), _clip((2, 3, 9, 36, 52), 9).cuda()
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
            assert tuple(whole.mean.shape) == (2, 16, 3, 4, 6)
            assert torch.equal(sliced.mean, whole.mean) and torch.equal(sliced.logvar, whole.logvar)
        finally:
            vae.disable_tiling()
            vae.disable_slicing()


def test_one_frame_still_takes_the_folded_path():
    """F = 1 is the 2-D path of tests/test_gpu_vae.py, not a one-frame clip: its moments stay 4-D and equal _moments' bit for bit"""
    vae, _ = _vae("narrow")
    x = _clip((1, 3, 1, 36, 52), 10).cuda()
    with torch.no_grad():
        dist = vae.encode(x).latent_dist
        assert dist._moments.dim() == 4 and torch.equal(dist._moments, vae._moments(x[:, :, 0]))
        assert tuple(dist.mean.shape) == (1, 16, 1, 4, 6)


# ---------------------------------------------------------------------------------------------------------------- 7. 02_encode.py's expression
def test_the_reference_encode_expression_on_a_bfloat16_module():
    """train/CogVideoX-5B/02_encode.py: `vae.encode(video_tensor.to(vae.dtype)).latent_dist.sample().squeeze(0)` with slicing and tiling enabled"""
    from videogpa_amd import ops
    from videogpa_amd.vae import AutoencoderKLCogVideoX
    vae32, sd = _vae("narrow")
    vae = AutoencoderKLCogVideoX(**NARROW)
    vae.load_state_dict(sd)
    vae = vae.to(device="cuda", dtype=torch.bfloat16).requires_grad_(False).eval()
    vae.enable_slicing()
    vae.enable_tiling()
    v = _clip((1, 3, 9, 36, 52), 11).cuda()
    with torch.no_grad():
        torch.manual_seed(321)
        z = vae.encode(v.to(vae.dtype)).latent_dist.sample().squeeze(0)
        torch.manual_seed(321)
        noise = torch.randn((1, 16, 3, 4, 6), device="cuda", dtype=torch.bfloat16)
        dist32 = vae32.encode(v).latent_dist
        want = ops.vae_sample(dist32._moments, noise=noise.float())["sample"].to(torch.bfloat16).squeeze(0)
    assert z.dtype == torch.bfloat16 and tuple(z.shape) == (16, 3, 4, 6) and torch.isfinite(z.float()).all()
    assert torch.equal(z, want)
