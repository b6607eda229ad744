"""Plain-torch CPU restatement of the decoder side of diffusers' AutoencoderKLCogVideoX (autoencoder_kl_cogvideox.py; PARITY UNPINNED, diffusers is
not installed): the spatially conditioned norm with its odd-frame split, the up-sampler with its three temporal cases, the decoder resnet and the
decoder pass with the conv cache, `_decode`'s loop over batches of latent frames and `tiled_decode`'s loop over latent tiles.  F.interpolate,
F.group_norm and F.conv3d throughout; it reads a state dict under upstream's names, runs in the dtype of that state dict (fp64 as the reference, fp32
for the reference's own error) and shares no code with videogpa_amd/vae.py."""
import torch
import torch.nn.functional as F

import vae_oracle as vo
import vae_video_oracle as vv


def seeded_decoder_state_dict(block_out_channels=(128, 256, 256, 512), layers_per_block=3, latent_channels=16, out_channels=3, seed=0):
    """`decoder.*` of a checkpoint-shaped state dict whose activations stay O(1): He-scaled convolutions (over all 27 taps: the frames differ),
    small biases, GroupNorm weights around 1, the modulation conv_y around 1 and conv_b small.  Every value is bf16-representable."""
    g = torch.Generator().manual_seed(seed)
    sd, L = {}, latent_channels

    def conv(name, cin, cout, shape):
        fan = cin * shape[0] * shape[1] * (shape[2] if len(shape) == 3 else 1)
        sd[name + ".weight"] = torch.randn(cout, cin, *shape, generator=g) * (1.0 / fan) ** 0.5
        sd[name + ".bias"] = 0.1 * torch.randn(cout, generator=g)

    def spatial_norm(name, c):
        sd[name + ".norm_layer.weight"] = 1.0 + 0.2 * torch.randn(c, generator=g)
        sd[name + ".norm_layer.bias"] = 0.2 * torch.randn(c, generator=g)
        sd[name + ".conv_y.conv.weight"] = torch.randn(c, L, 1, 1, 1, generator=g) * (0.1 / L ** 0.5)
        sd[name + ".conv_y.conv.bias"] = 1.0 + 0.1 * torch.randn(c, generator=g)
        sd[name + ".conv_b.conv.weight"] = torch.randn(c, L, 1, 1, 1, generator=g) * (0.1 / L ** 0.5)
        sd[name + ".conv_b.conv.bias"] = 0.1 * torch.randn(c, generator=g)

    def resnet(name, cin, cout):
        spatial_norm(name + ".norm1", cin)
        conv(name + ".conv1.conv", cin, cout, (3, 3, 3))
        spatial_norm(name + ".norm2", cout)
        conv(name + ".conv2.conv", cout, cout, (3, 3, 3))
        if cin != cout:
            conv(name + ".conv_shortcut", cin, cout, (1, 1, 1))

    rev = tuple(reversed(block_out_channels))
    conv("decoder.conv_in.conv", L, rev[0], (3, 3, 3))
    for j in range(2):
        resnet(f"decoder.mid_block.resnets.{j}", rev[0], rev[0])
    for i, c in enumerate(rev):
        for j in range(layers_per_block + 1):
            resnet(f"decoder.up_blocks.{i}.resnets.{j}", rev[max(i - 1, 0)] if j == 0 else c, c)
        if i < len(rev) - 1:
            conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", c, c, (3, 3))
    spatial_norm("decoder.norm_out", rev[-1])
    conv("decoder.conv_out.conv", rev[-1], out_channels, (3, 3, 3))
    return {k: v.to(torch.bfloat16).float() for k, v in sd.items()}


def resize_zq(zq, size, split=True):
    """CogVideoXSpatialNorm3D's resize of the latent zq [B,L,t,h,w] to a feature map's (T,H,W), nearest neighbour: an odd T > 1 sends frame 0 to frame
    0 and resizes the other frames on their own (split=False: the plain resize, for tests that must tell the two apart)"""
    T = size[0]
    if split and T > 1 and T % 2 == 1:
        first = F.interpolate(zq[:, :, :1], size=(1,) + tuple(size[1:]))
        rest = F.interpolate(zq[:, :, 1:], size=(T - 1,) + tuple(size[1:]))
        return torch.cat([first, rest], dim=2)
    return F.interpolate(zq, size=tuple(size))


def spatial_norm(sd, name, f, zq, groups, split=True):
    """CogVideoXSpatialNorm3D.forward: GroupNorm(f) (eps 1e-6) * conv_y(zq resized) + conv_b(zq resized), the two 1x1x1 convolutions at full size"""
    z = resize_zq(zq, f.shape[-3:], split)
    y = F.conv3d(z, sd[name + ".conv_y.conv.weight"], sd[name + ".conv_y.conv.bias"])
    b = F.conv3d(z, sd[name + ".conv_b.conv.weight"], sd[name + ".conv_b.conv.bias"])
    return F.group_norm(f, groups, sd[name + ".norm_layer.weight"], sd[name + ".norm_layer.bias"], 1e-6) * y + b


def upsample_frames(x, compress_time):
    """the interpolation of CogVideoXUpsample3D.forward alone, x [B,C,T,H,W]"""
    B, C, T, H, W = x.shape
    if compress_time:
        if T > 1 and T % 2 == 1:
            first = F.interpolate(x[:, :, 0], scale_factor=2.0)
            rest = F.interpolate(x[:, :, 1:], scale_factor=2.0)
            return torch.cat([first[:, :, None], rest], dim=2)
        if T > 1:
            return F.interpolate(x, scale_factor=2.0)
        return F.interpolate(x[:, :, 0], scale_factor=2.0)[:, :, None]
    x = F.interpolate(x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W), scale_factor=2.0)
    return x.reshape(B, T, C, 2 * H, 2 * W).permute(0, 2, 1, 3, 4)


def upsample(sd, name, x, compress_time):
    """CogVideoXUpsample3D: nearest x2 (in time too with compress_time, frame 0 of an odd count kept single), then the 3x3 Conv2d, padding 1, per frame"""
    x = upsample_frames(x, compress_time)
    B, C, T, H, W = x.shape
    x = F.conv2d(x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W), sd[name + ".conv.weight"], sd[name + ".conv.bias"], padding=1)
    return x.reshape(B, T, -1, H, W).permute(0, 2, 1, 3, 4)


def resnet(sd, name, x, zq, groups, cache=None):
    """CogVideoXResnetBlock3D with spatial norms and the two caches {"conv1", "conv2"}; returns (output, new caches)"""
    cache, new = cache or {}, {}
    h = F.silu(spatial_norm(sd, name + ".norm1", x, zq, groups))
    h, new["conv1"] = vv.causal_conv3d(h, sd[name + ".conv1.conv.weight"], sd[name + ".conv1.conv.bias"], cache.get("conv1"))
    h = F.silu(spatial_norm(sd, name + ".norm2", h, zq, groups))
    h, new["conv2"] = vv.causal_conv3d(h, sd[name + ".conv2.conv.weight"], sd[name + ".conv2.conv.bias"], cache.get("conv2"))
    if name + ".conv_shortcut.weight" in sd:
        x = F.conv3d(x, sd[name + ".conv_shortcut.weight"], sd[name + ".conv_shortcut.bias"])
    return x + h, new


def decoder(sd, z, cache=None, groups=32, temporal_compression_ratio=4):
    """CogVideoXDecoder3D.forward(sample, conv_cache): z [B,L,t,h,w] -> (frames [B,3,T,8h,8w], new cache).  Every spatial norm is conditioned on z, the
    chunk this pass was given."""
    cache, new = cache or {}, {}
    n_blocks = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("decoder.up_blocks."))
    n_time = {4: 2, 8: 3}[temporal_compression_ratio]
    h, new["conv_in"] = vv.causal_conv3d(z, sd["decoder.conv_in.conv.weight"], sd["decoder.conv_in.conv.bias"], cache.get("conv_in"))
    for j in range(2):
        name = f"decoder.mid_block.resnets.{j}"
        h, new[name] = resnet(sd, name, h, z, groups, cache.get(name))
    for i in range(n_blocks):
        j = 0
        while f"decoder.up_blocks.{i}.resnets.{j}.conv1.conv.weight" in sd:
            name = f"decoder.up_blocks.{i}.resnets.{j}"
            h, new[name] = resnet(sd, name, h, z, groups, cache.get(name))
            j += 1
        if f"decoder.up_blocks.{i}.upsamplers.0.conv.weight" in sd:
            h = upsample(sd, f"decoder.up_blocks.{i}.upsamplers.0", h, compress_time=i < n_time)
    h = F.silu(spatial_norm(sd, "decoder.norm_out", h, z, groups))
    h, new["conv_out"] = vv.causal_conv3d(h, sd["decoder.conv_out.conv.weight"], sd["decoder.conv_out.conv.bias"], cache.get("conv_out"))
    return h, new


def latent_frame_batches(num_frames, frame_batch_size=2):
    """AutoencoderKLCogVideoX._decode's ranges, written as upstream's loop (a slice past the end is cut by the tensor)"""
    out = []
    for i in range(max(num_frames // frame_batch_size, 1)):
        remaining = num_frames % frame_batch_size
        out.append((frame_batch_size * i + (0 if i == 0 else remaining), frame_batch_size * (i + 1) + remaining))
    return out


def batched_decoder(sd, z, frame_batch_size=2, **kw):
    """_decode without tiling: the latent frame batches one after the other, the cache handed on; frames [B,3,T,H,W]"""
    cache, out = None, []
    for start, end in latent_frame_batches(z.shape[2], frame_batch_size):
        frames, cache = decoder(sd, z[:, :, start:end], cache, **kw)
        out.append(frames)
    return torch.cat(out, dim=2)


def tiled_batched_decoder(sd, z, tile_sample_min_height, tile_sample_min_width, n_levels=4, overlap_factor_height=1 / 6, overlap_factor_width=1 / 5,
                          frame_batch_size=2, **kw):
    """tiled_decode: overlapping LATENT tiles decoded on their own by the frame-batch loop, each blended IN PLACE with the tile above and then the tile
    to its left over extents counted in sample pixels, cropped and concatenated"""
    h, w = z.shape[-2:]
    lat_h, lat_w = int(tile_sample_min_height / 2 ** (n_levels - 1)), int(tile_sample_min_width / 2 ** (n_levels - 1))
    overlap_h, overlap_w = int(lat_h * (1 - overlap_factor_height)), int(lat_w * (1 - overlap_factor_width))
    blend_h, blend_w = int(tile_sample_min_height * overlap_factor_height), int(tile_sample_min_width * overlap_factor_width)
    limit_h, limit_w = tile_sample_min_height - blend_h, tile_sample_min_width - blend_w
    rows = []
    for i in range(0, h, overlap_h):
        rows.append([batched_decoder(sd, z[:, :, :, i:i + lat_h, j:j + lat_w], frame_batch_size, **kw) for j in range(0, w, overlap_w)])
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = vo._blend_v(rows[i - 1][j], tile, blend_h)
            if j > 0:
                tile = vo._blend_h(row[j - 1], tile, blend_w)
            result_row.append(tile[:, :, :, :limit_h, :limit_w])
        result_rows.append(torch.cat(result_row, dim=4))
    return torch.cat(result_rows, dim=3)


cast, norm_err = vo.cast, vo.norm_err
