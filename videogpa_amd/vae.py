"""CogVideoX's VAE on the device: the drop-in for `diffusers.AutoencoderKLCogVideoX` where the reference uses it -- the encoder in the I2V trainer and in
the offline data preparation, the decoder (opt-in) at the end of the generate scripts.

SHARED by both sides.  Inference only, fp32 arithmetic, channels-last inside.  The convolutions run on the exact-fp32 MFMA core of the VGGT heads through
the entry points of csrc/vae_conv.hip (`ops.conv3x3_pad_f32`: its form with the padding given per side, for the downsampler, and the K sum in short runs,
for the accuracy bound of tests/test_gpu_vae.py; `ops.conv3d_causal_f32`, the 3x3x3 mode of the same core; `ops.conv1x1_f32` for the shortcuts);
GroupNorm + SiLU, the 3-channel stem's layout change, the Gaussian epilogue, the spatial norm and the output kernel are csrc/vae.hip.  Each decision
of diffusers' scheme is made once: the frame batches (`_ranges`) go one after the other through a whole network (`_batched`), every causal convolution
reading the last two frames of its input in the batch before from the conv cache (`_ConvCache`; frame 0 twice in the first batch), GroupNorm over the
batch's (T,H,W) per sample -- so the result DEPENDS on the batching, as upstream's does.  With tiling (`_tile_plan`, `_tiled`) every tile runs the frame
batches with a cache of its own and the blends are per frame.  The resnet is one body (`_resnet`) under its folded 2-D, cached 3-D and spatially
conditioned forms, and slicing is one loop (`_sliced`).

The ENCODER, where the reference's I2V trainer uses it --
`vae.encode(image[:, :, None]).latent_dist.sample() * vae.config.scaling_factor` inside every training step
(train/CogVideoX-I2V-5B/03_train.py:94-97,121-128):

    from videogpa_amd.vae import AutoencoderKLCogVideoX
    vae = AutoencoderKLCogVideoX.from_pretrained(model_path, subfolder="vae", torch_dtype=torch.bfloat16).cuda()
    vae.enable_slicing(); vae.enable_tiling()
    z = vae.encode(x).latent_dist.sample() * vae.config.scaling_factor      # x [B,3,1,H,W] -> [B,16,1,H/8,W/8]

and where the reference's offline data preparation uses it -- `vae.encode(video_tensor).latent_dist.sample()` on 49-frame clips with slicing and
tiling on (train/CogVideoX-{5B,I2V-5B,1.5-5B}/02_encode.py):

    z = vae.encode(v.to(vae.dtype)).latent_dist.sample()                    # v [B,3,F,H,W], F = 4k + 1 -> [B,16,(F-1)/4+1,H/8,W/8]

ONE frame is a path of its own (`_moments`): a causal 3-D convolution sees its only frame repeated in time, so each folds into a 2-D convolution whose
weight is the sum of the temporal taps (in fp32, from the checkpoint's values), and the temporal pooling of the downsamplers is the identity.
A CLIP of F = 4k + 1 frames (49, 81, 13, ...) is diffusers' `_encode`, restated (`_chunk_moments` under `_batched`): batches of
num_sample_frames_batch_size = 8 frames (`frame_batches`, the first one longer by F % 8), down blocks 0 and 1 halving time inside the downsampler's
loader (`ops.vae_downsample_f32`).  Any other F > 1 (02_encode.py's "clip shorter than 49 frames, take what there is") raises NotImplementedError.
Both walk the encoder through `_encoder_body`, with their own operations.  See DESIGN.md section 5f.

The DECODER is opt-in, `AutoencoderKLCogVideoX(with_decoder=True, ...)` / `from_pretrained(..., with_decoder=True)`: the end of the reference's
generate scripts (`pipe.vae.enable_tiling(); pipe.vae.enable_slicing()`, `output.frames`; videogpa_amd.generate.decode_latents),

    frames = vae.decode(latents.permute(0, 2, 1, 3, 4) / vae.config.scaling_factor).sample     # [B,16,13,60,90] -> [B,3,49,480,720]

diffusers' `_decode` restated (`_chunk_frames` under `_batched`): batches of num_latent_frames_batch_size = 2 latent frames (`latent_frame_batches`, the
first longer by F % 2), every norm a spatial norm conditioned on the batch's latent (`ops.spatial_norm_silu_f32`: the modulation maps stay at latent
resolution), the up-samplers of blocks 0 and 1 doubling time inside the loader (`ops.vae_upsample_f32`), `tiled_decode` over latent tiles
(`decode_tile_plan`).  Without the keyword the module is the encoder side alone: `decoder.*` is dropped on load and `decode` raises.  See DESIGN.md
section 5g.

PARITY UNPINNED (diffusers is neither installed nor vendored): the network, its parameter names, the tiled-encode scheme, the frame batching and
the conv-cache scheme are restated from diffusers' autoencoder_kl_cogvideox.py.  The loader is strict, so the first real checkpoint shows at once if a name here is wrong."""
import json
import os

import torch
import torch.nn as nn

from . import ops
from ._nn import _forward_only, _PackedCache
from .transformer import _Config

DEFAULT_CONFIG = dict(
    in_channels=3, out_channels=3,
    down_block_types=("CogVideoXDownBlock3D",) * 4, up_block_types=("CogVideoXUpBlock3D",) * 4,
    block_out_channels=(128, 256, 256, 512), latent_channels=16, layers_per_block=3, act_fn="silu", norm_eps=1e-6, norm_num_groups=32,
    temporal_compression_ratio=4, sample_height=480, sample_width=720, scaling_factor=0.7, shift_factor=None, latents_mean=None, latents_std=None,
    force_upcast=True, use_quant_conv=False, use_post_quant_conv=False, invert_scale_latents=False)


class _CausalConv3d(nn.Module):
    """CogVideoXCausalConv3d: the parameters live in `.conv` (a Conv3d); spatial zero padding k // 2, the first frame repeated k - 1 times in front"""

    def __init__(self, cin, cout, k=3):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, k)


class _ResnetBlock3D(nn.Module):
    def __init__(self, cin, cout, groups, eps):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, cin, eps=eps)
        self.norm2 = nn.GroupNorm(groups, cout, eps=eps)
        self.conv1 = _CausalConv3d(cin, cout)
        self.conv2 = _CausalConv3d(cout, cout)
        if cin != cout:
            self.conv_shortcut = nn.Conv3d(cin, cout, 1)


class _Downsample3D(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, stride=2, padding=0)


class _DownBlock3D(nn.Module):
    def __init__(self, cin, cout, layers, groups, eps, downsample):
        super().__init__()
        self.resnets = nn.ModuleList([_ResnetBlock3D(cin if j == 0 else cout, cout, groups, eps) for j in range(layers)])
        if downsample:
            self.downsamplers = nn.ModuleList([_Downsample3D(cout)])


class _MidBlock3D(nn.Module):
    def __init__(self, c, groups, eps):
        super().__init__()
        self.resnets = nn.ModuleList([_ResnetBlock3D(c, c, groups, eps) for _ in range(2)])


class _Encoder3D(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        chans, groups, eps = tuple(cfg.block_out_channels), cfg.norm_num_groups, cfg.norm_eps
        self.conv_in = _CausalConv3d(cfg.in_channels, chans[0])
        self.down_blocks = nn.ModuleList([
            _DownBlock3D(chans[max(i - 1, 0)], c, cfg.layers_per_block, groups, eps, downsample=i < len(chans) - 1) for i, c in enumerate(chans)])
        self.mid_block = _MidBlock3D(chans[-1], groups, eps)
        self.norm_out = nn.GroupNorm(groups, chans[-1], eps=eps)
        self.conv_out = _CausalConv3d(chans[-1], 2 * cfg.latent_channels)

    def resnets(self):
        """(cache name, resnet) in the order of the forward pass"""
        return [(f"down_blocks.{i}.resnets.{j}", r) for i, b in enumerate(self.down_blocks) for j, r in enumerate(b.resnets)] + \
               [(f"mid_block.resnets.{j}", r) for j, r in enumerate(self.mid_block.resnets)]


class _SpatialNorm3D(nn.Module):
    """CogVideoXSpatialNorm3D(C, L): GroupNorm(f) * conv_y(zq) + conv_b(zq), zq the latent resized to f; its GroupNorm's eps is 1e-6 whatever the config says"""

    def __init__(self, c, zq_channels, groups):
        super().__init__()
        self.norm_layer = nn.GroupNorm(groups, c, eps=1e-6)
        self.conv_y = _CausalConv3d(zq_channels, c, k=1)
        self.conv_b = _CausalConv3d(zq_channels, c, k=1)


class _DecoderResnetBlock3D(nn.Module):
    def __init__(self, cin, cout, zq_channels, groups):
        super().__init__()
        self.norm1 = _SpatialNorm3D(cin, zq_channels, groups)
        self.norm2 = _SpatialNorm3D(cout, zq_channels, groups)
        self.conv1 = _CausalConv3d(cin, cout)
        self.conv2 = _CausalConv3d(cout, cout)
        if cin != cout:
            self.conv_shortcut = nn.Conv3d(cin, cout, 1)


class _Upsample3D(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, padding=1)


class _UpBlock3D(nn.Module):
    def __init__(self, cin, cout, layers, zq_channels, groups, upsample):
        super().__init__()
        self.resnets = nn.ModuleList([_DecoderResnetBlock3D(cin if j == 0 else cout, cout, zq_channels, groups) for j in range(layers)])
        if upsample:
            self.upsamplers = nn.ModuleList([_Upsample3D(cout)])


class _DecoderMidBlock3D(nn.Module):
    def __init__(self, c, zq_channels, groups):
        super().__init__()
        self.resnets = nn.ModuleList([_DecoderResnetBlock3D(c, c, zq_channels, groups) for _ in range(2)])


class _Decoder3D(nn.Module):
    """CogVideoXDecoder3D under upstream's parameter names: the widths reversed, layers_per_block + 1 resnets per up block, an up-sampler on every block
    but the last, every norm a spatial norm conditioned on the latent"""

    def __init__(self, cfg):
        super().__init__()
        rev, groups, L = tuple(reversed(cfg.block_out_channels)), cfg.norm_num_groups, cfg.latent_channels
        self.conv_in = _CausalConv3d(L, rev[0])
        self.mid_block = _DecoderMidBlock3D(rev[0], L, groups)
        self.up_blocks = nn.ModuleList([
            _UpBlock3D(rev[max(i - 1, 0)], c, cfg.layers_per_block + 1, L, groups, upsample=i < len(rev) - 1) for i, c in enumerate(rev)])
        self.norm_out = _SpatialNorm3D(rev[-1], L, groups)
        self.conv_out = _CausalConv3d(rev[-1], cfg.out_channels)

    def resnets(self):
        """(cache name, resnet) in the order of the forward pass"""
        return [(f"mid_block.resnets.{j}", r) for j, r in enumerate(self.mid_block.resnets)] + \
               [(f"up_blocks.{i}.resnets.{j}", r) for i, b in enumerate(self.up_blocks) for j, r in enumerate(b.resnets)]


def _fold(conv):
    """a causal Conv3d on one frame -> the packed 2-D weight [3,3,Cin,Cout]: the frame fills all kt temporal taps, so they add (fp32)"""
    return ops.pack_conv_weight(conv.weight.detach().float().sum(dim=2))


def _pack3d(conv):
    """a causal Conv3d as it is -> the packed 3-D weight [3,3,3,Cin,Cout] of ops.conv3d_causal_f32"""
    return ops.pack_conv3d_weight(conv.weight)


def _vec(p):
    return p.detach().float().contiguous()


def _group_norm(n):
    return _vec(n.weight), _vec(n.bias)


def _pack_spatial_norm(n):
    """a spatial norm's parameters for the kernels: GroupNorm (gamma, beta), and conv_y | conv_b side by side as one 1x1 convolution [L, 2C] with its
    bias [2C], so that one ops.conv1x1_f32 of the latent gives the (Y | B) map ops.spatial_norm_silu_f32 gathers from"""
    wy, wb = (c.conv.weight.detach().float().reshape(c.conv.weight.shape[0], -1).t() for c in (n.conv_y, n.conv_b))
    return dict(gn=_group_norm(n.norm_layer),
                yb=(torch.cat([wy, wb], dim=1).contiguous(), torch.cat([_vec(n.conv_y.conv.bias), _vec(n.conv_b.conv.bias)])))


def _pack_block(r, norm, pack):
    """fp32 kernel-layout copies of a resnet's parameters: the norms as `norm` leaves them, the convolutions (weight as `pack` leaves it, bias), the
    1x1x1 shortcut as ([Cin,Cout], bias) or None"""
    sc = None
    if hasattr(r, "conv_shortcut"):
        w = r.conv_shortcut.weight.detach().float()
        sc = (w.reshape(w.shape[0], w.shape[1]).t().contiguous(), _vec(r.conv_shortcut.bias))
    return dict(n1=norm(r.norm1), n2=norm(r.norm2), c1=(pack(r.conv1.conv), _vec(r.conv1.conv.bias)),
                c2=(pack(r.conv2.conv), _vec(r.conv2.conv.bias)), sc=sc)


def _pack_resnet(r):
    """an encoder resnet: GroupNorm (gamma, beta), folded convolutions"""
    return _pack_block(r, _group_norm, _fold)


def _pack_decoder_resnet(r):
    """a decoder resnet: spatial norms, the causal convolutions with their temporal taps"""
    return _pack_block(r, _pack_spatial_norm, _pack3d)


class _ConvCache:
    """diffusers' conv_cache of one pass over a chunk of frames: per causal convolution the last two frames of its INPUT (behind the frames in
    front of them: a one-frame chunk keeps the newer of the two it was given), as a contiguous copy of their own, not a view that would keep the
    whole activation alive.  `prev` is the cache the chunk before left (None: the first chunk, frame 0 is replicated)."""

    def __init__(self, prev=None):
        self.prev, self.new = prev.new if prev is not None else {}, {}

    def conv(self, name, x, w, b, res=None):
        prev = self.prev.get(name)
        if x.shape[1] >= 2:
            self.new[name] = x[:, -2:].clone(memory_format=torch.contiguous_format)
        else:
            self.new[name] = torch.cat([prev[:, 1:] if prev is not None else x, x], dim=1)
        return ops.conv3d_causal_f32(x, w, b, res=res, prev=prev)


def _spatial_norm_silu(p, f, zq, groups):
    """silu(CogVideoXSpatialNorm3D(f, zq)) on f [N,T,H,W,C], zq [N,t,h,w,L]: the modulation maps at the latent's resolution (a 1x1 convolution commutes
    with the nearest resize exactly), the resize as the kernel's gather"""
    return ops.spatial_norm_silu_f32(f, ops.groupnorm_stats_f32(f, groups, 1e-6), *p["gn"], ops.conv1x1_f32(zq, *p["yb"]))


def _resnet(p, h, norm, conv):
    """CogVideoXResnetBlock3D on channels-last h: norm1, SiLU, conv1, norm2, SiLU, conv2, plus the input (through the 1x1x1 shortcut convolution when
    the width changes), the add fused into conv2's epilogue.  `norm(i, x)` is norm i with its SiLU and `conv(i, x, res)` convolution i, in the form
    of the three callers below"""
    t = norm(2, conv(1, norm(1, h), None))
    return conv(2, t, h if p["sc"] is None else ops.conv1x1_f32(h, *p["sc"]))


def _resnet_forward(p, h, groups, eps):
    """the encoder's resnet (no time embedding, no spatial norm) on one frame h [N,H,W,C]: the folded 2-D convolutions"""
    return _resnet(p, h, lambda i, x: ops.groupnorm_silu_f32(x, *p[f"n{i}"], groups, eps),
                   lambda i, x, res: ops.conv3x3_pad_f32(x, *p[f"c{i}"], res=res))


def _resnet_forward_video(p, w3, name, h, groups, eps, cache):
    """the encoder's resnet on a chunk h [N,T,H,W,C]: GroupNorm over the chunk's (T,H,W), the causal convolutions (weights w3) with their cache"""
    return _resnet(p, h, lambda i, x: ops.groupnorm_silu_f32(x, *p[f"n{i}"], groups, eps),
                   lambda i, x, res: cache.conv(f"{name}.conv{i}", x, w3[i - 1], p[f"c{i}"][1], res=res))


def _decoder_resnet_forward(p, name, h, zq, groups, cache):
    """the decoder's resnet on a chunk h [N,T,H,W,C]: both norms spatial norms conditioned on zq, the causal convolutions with their cache"""
    return _resnet(p, h, lambda i, x: _spatial_norm_silu(p[f"n{i}"], x, zq, groups),
                   lambda i, x, res: cache.conv(f"{name}.conv{i}", x, *p[f"c{i}"], res=res))


def _ranges(num, size):
    """diffusers' _encode / _decode: the (start, end) ranges `num` frames go through a network in, `size` frames each, the first one longer by the
    remainder (up to 2 * size - 1 frames are one batch).  Pure host arithmetic."""
    rem = num % size
    return [(size * i + (0 if i == 0 else rem), min(size * (i + 1) + rem, num)) for i in range(max(num // size, 1))]


def _batched(x, tdim, ranges, chunk):
    """the frames of x (axis tdim) in `ranges`, one batch after the other through `chunk(frames, cache)`, each with the conv cache the one before left;
    the outputs [N,T',...] joined in time.  GroupNorm statistics are per sample and per batch, as upstream, so the result depends on the batching."""
    cache, out = None, []
    for start, end in ranges:
        cache = _ConvCache(cache)
        out.append(chunk(x.narrow(tdim, start, end - start), cache))
        cache.prev = {}                                                  # the chunk before's frames are no longer needed
    return out[0] if len(out) == 1 else torch.cat(out, dim=1)


def _blend(prev, cur, extent, dim):
    """diffusers' blend_v / blend_h in place on `cur`: a linear ramp over its first `extent` rows / columns from the neighbour's last ones"""
    extent = min(prev.shape[dim], cur.shape[dim], extent)
    if extent > 0:
        shape = [1] * cur.dim()
        shape[dim] = extent
        t = (torch.arange(extent, device=cur.device, dtype=torch.float32) / extent).reshape(shape)
        head = cur.narrow(dim, 0, extent)
        head.copy_(prev.narrow(dim, prev.shape[dim] - extent, extent) * (1 - t) + head * t)


def _stitch(tiles, n_rows, n_cols, blend, keep, ydim):
    """the end of tiled_encode / tiled_decode on channels-last tiles {(row, col): tensor}: row-major, every tile blended in place with the tile above and
    then the tile to its left (so later blends read already-blended neighbours), cropped to `keep`, concatenated.  `ydim` is the tensors' row axis."""
    out_rows = []
    for a in range(n_rows):
        kept = []
        for b in range(n_cols):
            if a > 0:
                _blend(tiles[a - 1, b], tiles[a, b], blend[0], ydim)
            if b > 0:
                _blend(tiles[a, b - 1], tiles[a, b], blend[1], ydim + 1)
            kept.append(tiles[a, b][(slice(None),) * ydim + (slice(0, keep[0]), slice(0, keep[1]))])
        out_rows.append(torch.cat(kept, dim=ydim + 1))
    return torch.cat(out_rows, dim=ydim).contiguous()


def _tiled(x, ydim, plan, run, out_ydim):
    """tiled_encode / tiled_decode: the tiles of `plan` cut out of x (its row axis ydim), those of one size through `run` as one batch, the results
    (row axis out_ydim) blended and joined by _stitch"""
    rows, cols, N = plan["rows"], plan["cols"], x.shape[0]
    by_shape = {}                                                       # tiles of one size share a pass through the network as a batch
    for a, (i, th) in enumerate(rows):
        for b, (j, tw) in enumerate(cols):
            by_shape.setdefault((th, tw), []).append((a, b, i, j))
    tiles = {}
    for (th, tw), members in by_shape.items():
        out = run(torch.cat([x.narrow(ydim, i, th).narrow(ydim + 1, j, tw) for _, _, i, j in members], dim=0))
        for k, (a, b, _, _) in enumerate(members):
            tiles[a, b] = out[k * N:(k + 1) * N]
    return _stitch(tiles, len(rows), len(cols), plan["blend"], plan["keep"], out_ydim)


class DecoderOutput:
    def __init__(self, sample):
        self.sample = sample


class DiagonalGaussianDistribution:
    """diffusers' class of the same name over the encoder's moments (kept as fp32 [N,h,w,2L] channels-last, [N,T,h,w,2L] of a clip): `mean`, `logvar`
    (clamped to [-30, 20]), `std` = exp(logvar / 2), `mode()` and `sample(generator)` are [N,L,T,h,w] (T = 1 of one frame) in the VAE's dtype, each
    rounded once from the fp32 value"""

    def __init__(self, moments, dtype):
        self._moments, self._dtype, self._cache = moments, dtype, {}

    def _get(self, name):
        if name not in self._cache:
            self._cache.update(ops.vae_sample(self._moments, dtype=self._dtype, want=("mean", "logvar", "std")))
        return self._cache[name]

    mean = property(lambda self: self._get("mean"))
    logvar = property(lambda self: self._get("logvar"))
    std = property(lambda self: self._get("std"))

    def mode(self):
        return self.mean

    def sample(self, generator=None):
        """mean + std * randn, the noise drawn by torch.randn on the device in the VAE's dtype (a device generator reproduces it); formed in fp32 and
        rounded once (upstream's result to the rounding of its bf16 intermediates)"""
        N, (h, w, L2) = self._moments.shape[0], self._moments.shape[-3:]
        T = self._moments.shape[1] if self._moments.dim() == 5 else 1
        noise = torch.randn((N, L2 // 2, T, h, w), generator=generator, device=self._moments.device, dtype=self._dtype)
        return ops.vae_sample(self._moments, noise=noise, dtype=self._dtype)["sample"]


class AutoencoderKLOutput:
    def __init__(self, latent_dist):
        self.latent_dist = latent_dist


class AutoencoderKLCogVideoX(nn.Module):
    config_name = "config.json"
    weights_name = "diffusion_pytorch_model.safetensors"

    def __init__(self, with_decoder=False, **kw):
        """with_decoder=True adds `self.decoder` (and decode / forward); without it the module is the encoder side alone and `decoder.*` tensors of a
        checkpoint are dropped.  A constructor keyword, not a config key: it is not kept on `.config`."""
        super().__init__()
        cfg = _Config(DEFAULT_CONFIG)
        cfg.update(kw)                                   # unknown keys are kept on .config (checkpoint configs carry _class_name, _diffusers_version, ...)
        for k in ("block_out_channels", "down_block_types", "up_block_types"):
            cfg[k] = tuple(cfg[k])
        if cfg.use_quant_conv:
            raise NotImplementedError("use_quant_conv=True is not implemented (no CogVideoX checkpoint sets it)")
        if cfg.act_fn not in ("silu", "swish"):
            raise NotImplementedError(f"act_fn={cfg.act_fn!r}: only SiLU runs on the device")
        if cfg.in_channels != 3:
            raise NotImplementedError(f"in_channels={cfg.in_channels}: the stem kernel takes 3-channel images")
        bad = [c for c in cfg.block_out_channels if c % 32 or c > 1024] + ([] if (2 * cfg.latent_channels) % 16 == 0 else [2 * cfg.latent_channels])
        if bad or any(c % cfg.norm_num_groups for c in cfg.block_out_channels):
            raise NotImplementedError(f"block_out_channels {cfg.block_out_channels} / latent_channels {cfg.latent_channels} / norm_num_groups "
                                      f"{cfg.norm_num_groups}: widths must be multiples of 32 (<= 1024) and of the groups, 2 * latent_channels of 16")
        self.config = cfg
        self.encoder = _Encoder3D(cfg)
        self.decoder = None
        if with_decoder:
            if cfg.use_post_quant_conv:
                raise NotImplementedError("use_post_quant_conv=True is not implemented (no CogVideoX checkpoint sets it)")
            if cfg.latent_channels % 16 or cfg.out_channels != 3 or cfg.temporal_compression_ratio not in (4, 8):
                raise NotImplementedError(f"decoder: latent_channels {cfg.latent_channels} (a multiple of 16), out_channels {cfg.out_channels} (3) and "
                                          f"temporal_compression_ratio {cfg.temporal_compression_ratio} (4 or 8) are what runs on the device")
            self.decoder = _Decoder3D(cfg)
        self.use_slicing = self.use_tiling = False
        self.num_sample_frames_batch_size = 8                # frames per pass through the encoder (diffusers' _encode); the first pass takes the remainder too
        self.num_latent_frames_batch_size = 2                # latent frames per pass through the decoder (diffusers' _decode), likewise
        self._set_tile_sample_min(cfg.sample_height // 2, cfg.sample_width // 2)
        self.tile_overlap_factor_height = 1 / 6
        self.tile_overlap_factor_width = 1 / 5
        self._packed = _PackedCache()

    def _set_tile_sample_min(self, height, width):
        """the tile size in sample pixels and, from it, in latent pixels"""
        down = 2 ** (len(self.config.block_out_channels) - 1)
        self.tile_sample_min_height, self.tile_sample_min_width = height, width
        self.tile_latent_min_height, self.tile_latent_min_width = int(height / down), int(width / down)

    # ------------------------------------------------------------------ diffusers' switches
    def enable_slicing(self):
        """one sample per pass through the encoder (peak memory of one); no numerical effect: GroupNorm is per sample and every kernel's summation order
        is independent of the batch"""
        self.use_slicing = True

    def disable_slicing(self):
        self.use_slicing = False

    def enable_tiling(self, tile_sample_min_height=None, tile_sample_min_width=None, tile_overlap_factor_height=None, tile_overlap_factor_width=None):
        self.use_tiling = True
        self._set_tile_sample_min(tile_sample_min_height or self.tile_sample_min_height, tile_sample_min_width or self.tile_sample_min_width)
        self.tile_overlap_factor_height = tile_overlap_factor_height or self.tile_overlap_factor_height
        self.tile_overlap_factor_width = tile_overlap_factor_width or self.tile_overlap_factor_width

    def disable_tiling(self):
        self.use_tiling = False

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    # ------------------------------------------------------------------ loading
    @classmethod
    def from_pretrained(cls, path, subfolder=None, torch_dtype=None, **kw):
        """diffusers' on-disk layout from a LOCAL directory: <path>/<subfolder>/config.json + diffusion_pytorch_model.safetensors, or its shards
        `diffusion_pytorch_model-0000i-of-0000n.safetensors` listed by `diffusion_pytorch_model.safetensors.index.json`.  `decoder.*` tensors are
        skipped unless with_decoder=True is given; a missing or unexpected tensor, or one of another shape, is an error naming it.  torch_dtype=None
        keeps float32."""
        from safetensors.torch import load_file
        root = os.path.join(path, subfolder) if subfolder else path
        if not os.path.isdir(root):
            raise FileNotFoundError(f"AutoencoderKLCogVideoX.from_pretrained: {root!r} is not a local directory (there is no hub access on this path)")
        with open(os.path.join(root, cls.config_name)) as f:
            cfg = json.load(f)
        index = os.path.join(root, cls.weights_name + ".index.json")
        if os.path.isfile(index):
            with open(index) as f:
                files = sorted(set(json.load(f)["weight_map"].values()))
        elif os.path.isfile(os.path.join(root, cls.weights_name)):
            files = [cls.weights_name]
        else:
            raise FileNotFoundError(f"neither {cls.weights_name} nor its .index.json under {root}")
        sd = {}
        for fn in files:
            sd.update(load_file(os.path.join(root, fn)))
        model = cls(**{**cfg, **kw})
        model.load_state_dict(sd)
        if torch_dtype is not None:
            model = model.to(torch_dtype)
        model.eval()
        return model

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """strict: every difference raises with the tensor's name.  An encoder-only module (with_decoder=False) drops `decoder.*` first; one with the
        decoder is as strict on `decoder.*` as on `encoder.*`."""
        sd = {k: v for k, v in state_dict.items() if self.decoder is not None or not k.startswith("decoder.")}
        own = self.state_dict()
        missing, unexpected = sorted(k for k in own if k not in sd), sorted(k for k in sd if k not in own)
        wrong = sorted(f"{k}: checkpoint {tuple(sd[k].shape)}, model {tuple(own[k].shape)}" for k in sd if k in own and sd[k].shape != own[k].shape)
        if strict and (missing or unexpected or wrong):
            raise RuntimeError("AutoencoderKLCogVideoX.load_state_dict: " + "; ".join(
                f"{what}: {', '.join(keys)}" for what, keys in (("missing", missing), ("unexpected", unexpected), ("shape mismatch", wrong)) if keys))
        return super().load_state_dict(sd, strict=strict, assign=assign)

    # ------------------------------------------------------------------ what encode and decode share
    def _sliced(self, x, run):
        """behind an entry's own checks: x on the device and in the module's dtype, through `run` whole or, with slicing on, one sample at a time"""
        if not x.is_cuda:
            raise RuntimeError("videogpa_amd ops need GPU tensors (no CPU fallback)")
        _forward_only(self, x)
        x = x.to(self.dtype)
        if self.use_slicing and x.shape[0] > 1:
            return torch.cat([run(x[i:i + 1]) for i in range(x.shape[0])], dim=0)
        return run(x)

    def _tile_plan(self, height, width, cut, kept):
        """The tile grid of diffusers' tiled_encode / tiled_decode over a height x width map of the side that is cut into tiles of `cut` = (h, w):
        (rows, cols) of (start, size) in its pixels, the blend extents and the kept tile size in pixels of the other side, where a tile is `kept` =
        (h, w) and the results are blended"""
        fh, fw = self.tile_overlap_factor_height, self.tile_overlap_factor_width
        (cut_h, cut_w), (kept_h, kept_w) = cut, kept
        blend_h, blend_w = int(kept_h * fh), int(kept_w * fw)
        rows = [(i, min(cut_h, height - i)) for i in range(0, height, int(cut_h * (1 - fh)))]
        cols = [(j, min(cut_w, width - j)) for j in range(0, width, int(cut_w * (1 - fw)))]
        return dict(rows=rows, cols=cols, blend=(blend_h, blend_w), keep=(kept_h - blend_h, kept_w - blend_w))

    # ------------------------------------------------------------------ encoder: kernel-layout copies
    def packed(self):
        """fp32 kernel-layout copies of every parameter (temporal taps folded, the stem padded to 16 input channels with zero rows), rebuilt when a
        parameter changes or moves.  The resnets are keyed by `_Encoder3D.resnets()`'s names, the downsamplers by their block's index."""
        enc = self.encoder

        def make():
            w_in = _fold(enc.conv_in.conv)
            w_in = torch.cat([w_in, w_in.new_zeros(3, 3, 16 - w_in.shape[2], w_in.shape[3])], dim=2).contiguous()
            return {"conv_in": (w_in, _vec(enc.conv_in.conv.bias)), "conv_out": (_fold(enc.conv_out.conv), _vec(enc.conv_out.conv.bias)),
                    "norm_out": _group_norm(enc.norm_out), "resnets": {name: _pack_resnet(r) for name, r in enc.resnets()},
                    "down": {i: (ops.pack_conv_weight(b.downsamplers[0].conv.weight), _vec(b.downsamplers[0].conv.bias))
                             for i, b in enumerate(enc.down_blocks) if hasattr(b, "downsamplers")}}
        return self._packed.get("all", list(self.parameters()), make)

    def packed_video(self):
        """the causal convolutions with their temporal taps kept, [3,3,3,Cin,Cout] fp32 (the stem padded to 16 input channels), for clips; everything
        else comes from packed().  A cache entry of its own: a module that only ever sees one frame never builds it."""
        enc = self.encoder

        def make():
            w_in = _pack3d(enc.conv_in.conv)
            w_in = torch.cat([w_in, w_in.new_zeros(3, 3, 3, 16 - w_in.shape[3], w_in.shape[4])], dim=3).contiguous()
            return {"conv_in": w_in, "conv_out": _pack3d(enc.conv_out.conv),
                    "resnets": {name: (_pack3d(r.conv1.conv), _pack3d(r.conv2.conv)) for name, r in enc.resnets()}}
        return self._packed.get("video", list(self.parameters()), make)

    def frame_batches(self, num_frames):
        """diffusers' _encode: the (start, end) frame ranges a clip is encoded in, num_sample_frames_batch_size frames each, the first one longer by the
        remainder (49 -> (0,9), (9,17), ..., (41,49); up to 15 frames are one batch)"""
        return _ranges(num_frames, self.num_sample_frames_batch_size)

    # ------------------------------------------------------------------ encoder: forward
    def _encoder_body(self, h, resnet, down, what):
        """the encoder between conv_in and norm_out on channels-last h: `resnet(name, h)` for every resnet, `down(i, h)` behind down block i"""
        enc = self.encoder
        for i, b in enumerate(enc.down_blocks):
            for j in range(len(b.resnets)):
                h = resnet(f"down_blocks.{i}.resnets.{j}", h)
            if hasattr(b, "downsamplers"):
                if min(h.shape[-3], h.shape[-2]) < 2:
                    raise RuntimeError(f"the {what} is too small: a {h.shape[-3]} x {h.shape[-2]} map reached a downsampler")
                h = down(i, h)
        for j in range(len(enc.mid_block.resnets)):
            h = resnet(f"mid_block.resnets.{j}", h)
        return h

    def _moments(self, x):
        """x [N,3,H,W] in the module's dtype -> the encoder's output [N,H/8,W/8,2L] fp32 channels-last: the folded 2-D path of one frame"""
        P, G, eps = self.packed(), self.config.norm_num_groups, self.config.norm_eps
        h = ops.conv3x3_pad_f32(ops.vae_input_f32(x.contiguous()), *P["conv_in"])
        h = self._encoder_body(h, lambda name, h: _resnet_forward(P["resnets"][name], h, G, eps),
                               lambda i, h: ops.conv3x3_pad_f32(h, *P["down"][i], stride=2, pad_lo=0, pad_hi=1),      # temporal pooling: the identity on one frame
                               "image")
        return ops.conv3x3_pad_f32(ops.groupnorm_silu_f32(h, *P["norm_out"], G, eps), *P["conv_out"])

    def _chunk_moments(self, x, cache):
        """one pass of diffusers' encoder over a chunk of frames: x [N,3,T,H,W] in the module's dtype -> [N,T',H/8,W/8,2L] fp32 channels-last, T' the
        frames left by the temporal pooling of down blocks 0 and 1.  `cache` is this pass's _ConvCache (it reads the chunk before's, it keeps its own)."""
        P, V, G, eps = self.packed(), self.packed_video(), self.config.norm_num_groups, self.config.norm_eps
        N, _, T, H, W = x.shape
        n_time = {4: 2, 8: 3}.get(self.config.temporal_compression_ratio, 0)
        frames = ops.vae_input_f32(x.transpose(1, 2).contiguous().view(N * T, 3, H, W)).view(N, T, H, W, 16)       # the 3-channel tensor: a host-side permute
        h = cache.conv("conv_in", frames, V["conv_in"], P["conv_in"][1])
        h = self._encoder_body(h, lambda name, h: _resnet_forward_video(P["resnets"][name], V["resnets"][name], name, h, G, eps, cache),
                               lambda i, h: ops.vae_downsample_f32(h, *P["down"][i], compress_time=i < n_time), "clip")
        return cache.conv("conv_out", ops.groupnorm_silu_f32(h, *P["norm_out"], G, eps), V["conv_out"], P["conv_out"][1])

    def _video_moments(self, x):
        """x [N,3,F,H,W] -> [N,(F-1)/4+1,H/8,W/8,2L]: diffusers' _encode, the frame batches through the whole encoder"""
        return _batched(x, 2, self.frame_batches(x.shape[2]), self._chunk_moments)

    def tile_plan(self, height, width):
        """The tile grid of diffusers' tiled_encode for a height x width image: (rows, cols) of (start, size) in pixels, the blend extents and the kept
        tile size in latent pixels"""
        return self._tile_plan(height, width, (self.tile_sample_min_height, self.tile_sample_min_width), (self.tile_latent_min_height, self.tile_latent_min_width))

    def _encode(self, x):
        """x [N,3,H,W] (one frame: the folded 2-D path) or [N,3,F,H,W] (a clip) -> the moments [N,h,w,2L] or [N,T',h,w,2L], channels-last.  Tiled: every
        tile of a clip runs the frame batches with a conv cache of its own, the blends are per frame."""
        H, W = x.shape[-2], x.shape[-1]
        run = self._video_moments if x.dim() == 5 else self._moments
        if self.use_tiling and (W > self.tile_sample_min_width or H > self.tile_sample_min_height):
            return _tiled(x, x.dim() - 2, self.tile_plan(H, W), run, x.dim() - 3)
        return run(x)

    def encode(self, x, return_dict=True):
        """x [B,3,F,H,W], F = 1 or F = 4k + 1 (the model's clip lengths: 49, 81, 13, ...) -> AutoencoderKLOutput whose `.latent_dist` is the
        DiagonalGaussianDistribution of the [B,L,(F-1)/4+1,H/8,W/8] latent.  The input is rounded to the module's dtype first (the reference's
        `.to(self.vae.dtype)`).  One frame runs the folded 2-D path; a clip runs diffusers' frame batches (frame_batches) with the conv cache."""
        if x.dim() != 5 or x.shape[1] != 3:
            raise RuntimeError(f"encode: expected [B,3,F,H,W], got {tuple(x.shape)}")
        F = x.shape[2]
        if F != 1 and F % 4 != 1:
            raise NotImplementedError(f"encode of {F} frames: one frame (the I2V conditioning image) or 4k + 1 frames (the model's clip lengths, "
                                      "02_encode.py's 49) run on the device; a clip of another length is refused, not padded or cut")
        dist = DiagonalGaussianDistribution(self._sliced(x, lambda s: self._encode(s[:, :, 0] if F == 1 else s)), self.dtype)
        return AutoencoderKLOutput(dist) if return_dict else (dist,)

    # ------------------------------------------------------------------ decoder (with_decoder=True)
    def packed_decoder(self):
        """fp32 kernel-layout copies of the decoder's parameters: causal convolutions [3,3,3,Cin,Cout] (conv_out padded to 16 output channels with zero
        columns), the spatial norms as _pack_spatial_norm leaves them, the up-samplers' 2-D weights [3,3,C,C]"""
        dec = self.decoder

        def make():
            w_out, b_out = _pack3d(dec.conv_out.conv), _vec(dec.conv_out.conv.bias)
            w_out = torch.cat([w_out, w_out.new_zeros(*w_out.shape[:4], 16 - w_out.shape[4])], dim=4).contiguous()
            b_out = torch.cat([b_out, b_out.new_zeros(16 - b_out.shape[0])])
            return {"conv_in": (_pack3d(dec.conv_in.conv), _vec(dec.conv_in.conv.bias)), "conv_out": (w_out, b_out),
                    "norm_out": _pack_spatial_norm(dec.norm_out), "resnets": {name: _pack_decoder_resnet(r) for name, r in dec.resnets()},
                    "up": {i: (ops.pack_conv_weight(b.upsamplers[0].conv.weight), _vec(b.upsamplers[0].conv.bias))
                           for i, b in enumerate(dec.up_blocks) if hasattr(b, "upsamplers")}}
        return self._packed.get("decoder", list(dec.parameters()), make)

    def latent_frame_batches(self, num_frames):
        """diffusers' _decode: the (start, end) latent frame ranges a latent is decoded in, num_latent_frames_batch_size frames each, the first one longer
        by the remainder (13 -> (0,3), (3,5), ..., (11,13); up to 3 frames are one batch)"""
        return _ranges(num_frames, self.num_latent_frames_batch_size)

    def _chunk_frames(self, zq, cache):
        """one pass of diffusers' decoder over a chunk of latent frames: zq [N,t,h,w,L] fp32 channels-last -> [N,T,8h,8w,16] fp32 (channels 0..2 are the
        image, the rest zero), T the frames the up-samplers of blocks 0 and 1 (compress_time) make of t.  Every spatial norm is conditioned on zq."""
        P, G, dec = self.packed_decoder(), self.config.norm_num_groups, self.decoder
        n_time = {4: 2, 8: 3}[self.config.temporal_compression_ratio]
        zq = zq.contiguous()
        h = cache.conv("conv_in", zq, *P["conv_in"])

        def resnet(name, h):
            return _decoder_resnet_forward(P["resnets"][name], name, h, zq, G, cache)

        for j in range(len(dec.mid_block.resnets)):
            h = resnet(f"mid_block.resnets.{j}", h)
        for i, b in enumerate(dec.up_blocks):
            for j in range(len(b.resnets)):
                h = resnet(f"up_blocks.{i}.resnets.{j}", h)
            if i in P["up"]:
                h = ops.vae_upsample_f32(h, *P["up"][i], compress_time=i < n_time)
        return cache.conv("conv_out", _spatial_norm_silu(P["norm_out"], h, zq, G), *P["conv_out"])

    def _latent_frames(self, z):
        """z [N,F,h,w,L] fp32 channels-last -> [N,F',8h,8w,16]: diffusers' _decode, the latent frame batches through the whole decoder"""
        return _batched(z, 1, self.latent_frame_batches(z.shape[1]), self._chunk_frames)

    def decode_tile_plan(self, height, width):
        """The tile grid of diffusers' tiled_decode for a height x width LATENT: (rows, cols) of (start, size) in latent pixels, the blend extents and the
        kept tile size in sample pixels"""
        return self._tile_plan(height, width, (self.tile_latent_min_height, self.tile_latent_min_width), (self.tile_sample_min_height, self.tile_sample_min_width))

    def _decode(self, z):
        """z [N,L,F,h,w] in the module's dtype -> the frames [N,F',8h,8w,16] fp32 channels-last.  Tiled: every latent tile through the frame batches
        with a conv cache of its own, the blends per frame in sample pixels."""
        z = z.permute(0, 2, 3, 4, 1).float().contiguous()               # the latent is small: a host-side permute
        if self.use_tiling and (z.shape[3] > self.tile_latent_min_width or z.shape[2] > self.tile_latent_min_height):
            return _tiled(z, 2, self.decode_tile_plan(z.shape[2], z.shape[3]), self._latent_frames, 2)
        return self._latent_frames(z)

    def _decoded_frames(self, z):
        if self.decoder is None:
            raise NotImplementedError("this module is the encoder side only: construct it (or call from_pretrained) with with_decoder=True to decode")
        if z.dim() != 5 or z.shape[1] != self.config.latent_channels:
            raise RuntimeError(f"decode: expected [B,{self.config.latent_channels},F,h,w], got {tuple(z.shape)}")
        return self._sliced(z, self._decode)

    def decode(self, z, return_dict=True):
        """z [B,L,F,h,w] -> DecoderOutput whose `.sample` is [B,3,F',8h,8w] in the module's dtype, rounded once from fp32; F' = 4 (F - 1) + 1 frames of an
        odd F (13 -> 49), 4 F of an even one (diffusers' latent frame batches, latent_frame_batches).  z is rounded to the module's dtype first."""
        frames = self._decoded_frames(z)
        sample = ops.vae_output(frames, self.dtype)
        return DecoderOutput(sample) if return_dict else (sample,)

    def decode_uint8(self, z):
        """decode followed by the pipeline's postprocess_video, from the fp32 frames: [B,F',8h,8w,3] uint8 = round(clamp(x / 2 + 0.5, 0, 1) * 255)"""
        return ops.vae_output(self._decoded_frames(z), uint8=True)

    def forward(self, sample, sample_posterior=False, return_dict=True, generator=None):
        """diffusers' forward: encode, the posterior's sample (or its mode), decode"""
        if self.decoder is None:
            raise NotImplementedError("AutoencoderKLCogVideoX.forward (encode + decode) needs the decoder: construct the module with with_decoder=True")
        posterior = self.encode(sample).latent_dist
        return self.decode(posterior.sample(generator=generator) if sample_posterior else posterior.mode(), return_dict=return_dict)
