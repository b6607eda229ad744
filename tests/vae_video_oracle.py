"""tests/vae_oracle.py extended to clips, as diffusers' AutoencoderKLCogVideoX encodes them (autoencoder_kl_cogvideox.py; PARITY UNPINNED, diffusers is
not installed): the causal convolution with its conv_cache, an encoder pass that takes and returns the cache, `_encode`'s loop over batches of frames
and `tiled_encode`'s loop over tiles, each tile with the frame batches and a cache of its own.  Plain torch on the CPU in the dtype of the state dict
(fp64 as the reference, fp32 for the reference's own error); it shares no code with videogpa_amd/vae.py."""
import torch
import torch.nn.functional as F

import vae_oracle as vo


def causal_conv3d(x, w, b, cache=None):
    """CogVideoXCausalConv3d.forward(inputs, conv_cache), x [B,C,T,H,W]: the kt - 1 frames in front are the cache, or the first frame repeated; the new
    cache is the last kt - 1 frames of the padded input.  Returns (output, new cache)."""
    kt, kh, kw = w.shape[2:]
    if kt > 1:
        x = torch.cat(([cache] if cache is not None else [x[:, :, :1]] * (kt - 1)) + [x], dim=2)
    new = x[:, :, -(kt - 1):].clone() if kt > 1 else None
    return F.conv3d(F.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2)), w, b), new


def resnet(sd, name, x, groups, eps, cache=None):
    """vo.resnet with the two caches {"conv1", "conv2"}; returns (output, new caches)"""
    cache, new = cache or {}, {}
    h = F.silu(F.group_norm(x, groups, sd[name + ".norm1.weight"], sd[name + ".norm1.bias"], eps))
    h, new["conv1"] = causal_conv3d(h, sd[name + ".conv1.conv.weight"], sd[name + ".conv1.conv.bias"], cache.get("conv1"))
    h = F.silu(F.group_norm(h, groups, sd[name + ".norm2.weight"], sd[name + ".norm2.bias"], eps))
    h, new["conv2"] = causal_conv3d(h, sd[name + ".conv2.conv.weight"], sd[name + ".conv2.conv.bias"], cache.get("conv2"))
    if name + ".conv_shortcut.weight" in sd:
        x = F.conv3d(x, sd[name + ".conv_shortcut.weight"], sd[name + ".conv_shortcut.bias"])
    return x + h, new


def encoder(sd, x, cache=None, groups=32, eps=1e-6, temporal_compression_ratio=4):
    """CogVideoXEncoder3D.forward(sample, conv_cache): x [B,3,T,H,W] -> (moments [B,2L,T',H/8,W/8], new cache).  GroupNorm sees the T frames it is
    given, nothing of the frames before them."""
    cache, new = cache or {}, {}
    n_blocks = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.down_blocks."))
    n_time = {4: 2, 8: 3}.get(temporal_compression_ratio, 0)
    h, new["conv_in"] = causal_conv3d(x, sd["encoder.conv_in.conv.weight"], sd["encoder.conv_in.conv.bias"], cache.get("conv_in"))
    for i in range(n_blocks):
        j = 0
        while f"encoder.down_blocks.{i}.resnets.{j}.norm1.weight" in sd:
            name = f"encoder.down_blocks.{i}.resnets.{j}"
            h, new[name] = resnet(sd, name, h, groups, eps, cache.get(name))
            j += 1
        if f"encoder.down_blocks.{i}.downsamplers.0.conv.weight" in sd:
            h = vo.downsample(sd, f"encoder.down_blocks.{i}.downsamplers.0", h, compress_time=i < n_time)
    for j in range(2):
        name = f"encoder.mid_block.resnets.{j}"
        h, new[name] = resnet(sd, name, h, groups, eps, cache.get(name))
    h = F.silu(F.group_norm(h, groups, sd["encoder.norm_out.weight"], sd["encoder.norm_out.bias"], eps))
    h, new["conv_out"] = causal_conv3d(h, sd["encoder.conv_out.conv.weight"], sd["encoder.conv_out.conv.bias"], cache.get("conv_out"))
    return h, new


def frame_batches(num_frames, frame_batch_size=8):
    """AutoencoderKLCogVideoX._encode's ranges, written as upstream's loop (a slice past the end is cut by the tensor)"""
    out = []
    for i in range(max(num_frames // frame_batch_size, 1)):
        remaining = num_frames % frame_batch_size
        out.append((frame_batch_size * i + (0 if i == 0 else remaining), frame_batch_size * (i + 1) + remaining))
    return out


def batched_encoder(sd, x, frame_batch_size=8, **kw):
    """_encode without tiling: the frame batches one after the other, the cache handed on; moments [B,2L,T',h,w]"""
    cache, out = None, []
    for start, end in frame_batches(x.shape[2], frame_batch_size):
        m, cache = encoder(sd, x[:, :, start:end], cache, **kw)
        out.append(m)
    return torch.cat(out, dim=2)


def tiled_batched_encoder(sd, x, tile_sample_min_height, tile_sample_min_width, n_levels=4, overlap_factor_height=1 / 6, overlap_factor_width=1 / 5,
                          frame_batch_size=8, **kw):
    """tiled_encode on a clip: vo.tiled_encoder's grid, blends and crops, every tile encoded by the frame-batch loop with its own cache"""
    H, W = x.shape[-2:]
    lat_h, lat_w = int(tile_sample_min_height / 2 ** (n_levels - 1)), int(tile_sample_min_width / 2 ** (n_levels - 1))
    overlap_h, overlap_w = int(tile_sample_min_height * (1 - overlap_factor_height)), int(tile_sample_min_width * (1 - overlap_factor_width))
    blend_h, blend_w = int(lat_h * overlap_factor_height), int(lat_w * overlap_factor_width)
    limit_h, limit_w = lat_h - blend_h, lat_w - blend_w
    rows = []
    for i in range(0, H, overlap_h):
        rows.append([batched_encoder(sd, x[:, :, :, i:i + tile_sample_min_height, j:j + tile_sample_min_width], frame_batch_size, **kw)
                     for j in range(0, W, overlap_w)])
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
