"""Plain-torch CPU restatement of the encoder side of diffusers' AutoencoderKLCogVideoX (autoencoder_kl_cogvideox.py; PARITY UNPINNED, diffusers is
not installed), in its GENERAL 3-D form: F.conv3d behind the causal first-frame replication, F.group_norm, the downsampler with its temporal
pooling branch, and the tiled-encode loop.  It reads a state dict under upstream's names and shares no code with videogpa_amd/vae.py, so the
one-frame fold of the temporal taps and the one-sided padding of the downsampler are tested there, not assumed.  Runs in the dtype of the state
dict it is given (fp64 as the reference, fp32 for the reference's own error)."""
import torch
import torch.nn.functional as F


def seeded_state_dict(block_out_channels=(128, 256, 256, 512), layers_per_block=3, latent_channels=16, seed=0, with_decoder_keys=False):
    """A checkpoint-shaped state dict whose activations stay O(1): He-scaled convolution weights (over the 27 taps the single frame fills), small
    biases, GroupNorm weights around 1.  Every value is bf16-representable, like a bf16 checkpoint's."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv3d(name, cin, cout, k):
        fan = cin * k * 3 * k if k == 3 else cin                     # the frame is repeated: the three temporal taps add coherently
        sd[name + ".weight"] = torch.randn(cout, cin, k, k, k, generator=g) * (1.0 / fan) ** 0.5
        sd[name + ".bias"] = 0.1 * torch.randn(cout, generator=g)

    def norm(name, c):
        sd[name + ".weight"] = 1.0 + 0.2 * torch.randn(c, generator=g)
        sd[name + ".bias"] = 0.2 * torch.randn(c, generator=g)

    def resnet(name, cin, cout):
        norm(name + ".norm1", cin)
        conv3d(name + ".conv1.conv", cin, cout, 3)
        norm(name + ".norm2", cout)
        conv3d(name + ".conv2.conv", cout, cout, 3)
        if cin != cout:
            conv3d(name + ".conv_shortcut", cin, cout, 1)

    chans = tuple(block_out_channels)
    conv3d("encoder.conv_in.conv", 3, chans[0], 3)
    for i, c in enumerate(chans):
        for j in range(layers_per_block):
            resnet(f"encoder.down_blocks.{i}.resnets.{j}", chans[max(i - 1, 0)] if j == 0 else c, c)
        if i < len(chans) - 1:
            sd[f"encoder.down_blocks.{i}.downsamplers.0.conv.weight"] = torch.randn(c, c, 3, 3, generator=g) * (1.0 / (9 * c)) ** 0.5
            sd[f"encoder.down_blocks.{i}.downsamplers.0.conv.bias"] = 0.1 * torch.randn(c, generator=g)
    for j in range(2):
        resnet(f"encoder.mid_block.resnets.{j}", chans[-1], chans[-1])
    norm("encoder.norm_out", chans[-1])
    conv3d("encoder.conv_out.conv", chans[-1], 2 * latent_channels, 3)
    if with_decoder_keys:
        sd["decoder.conv_in.conv.weight"] = torch.randn(chans[-1], latent_channels, 3, 3, 3, generator=g)
        sd["decoder.conv_in.conv.bias"] = torch.randn(chans[-1], generator=g)
    return {k: v.to(torch.bfloat16).float() for k, v in sd.items()}


def causal_conv3d(x, w, b):
    """CogVideoXCausalConv3d, x [B,C,T,H,W]: spatial zero padding k // 2, the first frame repeated kt - 1 times in front, then a plain conv3d"""
    kt, kh, kw = w.shape[2:]
    if kt > 1:
        x = torch.cat([x[:, :, :1]] * (kt - 1) + [x], dim=2)
    return F.conv3d(F.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2)), w, b)


def resnet(sd, name, x, groups, eps):
    h = F.silu(F.group_norm(x, groups, sd[name + ".norm1.weight"], sd[name + ".norm1.bias"], eps))
    h = causal_conv3d(h, sd[name + ".conv1.conv.weight"], sd[name + ".conv1.conv.bias"])
    h = F.silu(F.group_norm(h, groups, sd[name + ".norm2.weight"], sd[name + ".norm2.bias"], eps))
    h = causal_conv3d(h, sd[name + ".conv2.conv.weight"], sd[name + ".conv2.conv.bias"])
    if name + ".conv_shortcut.weight" in sd:
        x = F.conv3d(x, sd[name + ".conv_shortcut.weight"], sd[name + ".conv_shortcut.bias"])
    return x + h


def downsample(sd, name, x, compress_time):
    """CogVideoXDownsample3D: average pooling over time (the first frame of an odd count is kept aside), then pad right / bottom by one and a
    stride-2 3x3 Conv2d without padding, frame by frame"""
    B, C, T, H, W = x.shape
    if compress_time:
        x = x.permute(0, 3, 4, 1, 2).reshape(B * H * W, C, T)
        if T % 2 == 1:
            first, rest = x[..., 0], x[..., 1:]
            if rest.shape[-1] > 0:
                rest = F.avg_pool1d(rest, kernel_size=2, stride=2)
            x = torch.cat([first[..., None], rest], dim=-1)
        else:
            x = F.avg_pool1d(x, kernel_size=2, stride=2)
        T = x.shape[-1]
        x = x.reshape(B, H, W, C, T).permute(0, 3, 4, 1, 2)
    x = F.pad(x, (0, 1, 0, 1), mode="constant", value=0)
    x = x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H + 1, W + 1)
    x = F.conv2d(x, sd[name + ".conv.weight"], sd[name + ".conv.bias"], stride=2, padding=0)
    return x.reshape(B, T, C, x.shape[-2], x.shape[-1]).permute(0, 2, 1, 3, 4)


def encoder(sd, x, groups=32, eps=1e-6, temporal_compression_ratio=4):
    """x [B,3,T,H,W] -> moments [B,2L,T',H/8,W/8]"""
    n_blocks = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.down_blocks."))
    n_time = {4: 2, 8: 3}.get(temporal_compression_ratio, 0)
    h = causal_conv3d(x, sd["encoder.conv_in.conv.weight"], sd["encoder.conv_in.conv.bias"])
    for i in range(n_blocks):
        j = 0
        while f"encoder.down_blocks.{i}.resnets.{j}.norm1.weight" in sd:
            h = resnet(sd, f"encoder.down_blocks.{i}.resnets.{j}", h, groups, eps)
            j += 1
        if f"encoder.down_blocks.{i}.downsamplers.0.conv.weight" in sd:
            h = downsample(sd, f"encoder.down_blocks.{i}.downsamplers.0", h, compress_time=i < n_time)
    for j in range(2):
        h = resnet(sd, f"encoder.mid_block.resnets.{j}", h, groups, eps)
    h = F.silu(F.group_norm(h, groups, sd["encoder.norm_out.weight"], sd["encoder.norm_out.bias"], eps))
    return causal_conv3d(h, sd["encoder.conv_out.conv.weight"], sd["encoder.conv_out.conv.bias"])


def _blend_v(a, b, extent):
    extent = min(a.shape[3], b.shape[3], extent)
    for y in range(extent):
        b[:, :, :, y, :] = a[:, :, :, -extent + y, :] * (1 - y / extent) + b[:, :, :, y, :] * (y / extent)
    return b


def _blend_h(a, b, extent):
    extent = min(a.shape[4], b.shape[4], extent)
    for x in range(extent):
        b[:, :, :, :, x] = a[:, :, :, :, -extent + x] * (1 - x / extent) + b[:, :, :, :, x] * (x / extent)
    return b


def tiled_encoder(sd, x, tile_sample_min_height, tile_sample_min_width, n_levels=4, overlap_factor_height=1 / 6, overlap_factor_width=1 / 5, **kw):
    """tiled_encode: overlapping tiles encoded on their own, each blended IN PLACE with the tile above and then the tile to its left (so later blends
    read already-blended neighbours), cropped and concatenated"""
    H, W = x.shape[-2:]
    lat_h, lat_w = int(tile_sample_min_height / 2 ** (n_levels - 1)), int(tile_sample_min_width / 2 ** (n_levels - 1))
    overlap_h, overlap_w = int(tile_sample_min_height * (1 - overlap_factor_height)), int(tile_sample_min_width * (1 - overlap_factor_width))
    blend_h, blend_w = int(lat_h * overlap_factor_height), int(lat_w * overlap_factor_width)
    limit_h, limit_w = lat_h - blend_h, lat_w - blend_w
    rows = []
    for i in range(0, H, overlap_h):
        rows.append([encoder(sd, x[:, :, :, i:i + tile_sample_min_height, j:j + tile_sample_min_width], **kw) for j in range(0, W, overlap_w)])
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = _blend_v(rows[i - 1][j], tile, blend_h)
            if j > 0:
                tile = _blend_h(row[j - 1], tile, blend_w)
            result_row.append(tile[:, :, :, :limit_h, :limit_w])
        result_rows.append(torch.cat(result_row, dim=4))
    return torch.cat(result_rows, dim=3)


def gaussian(moments, noise=None):
    """DiagonalGaussianDistribution: (mean, clamped logvar, std, mean + std * noise)"""
    mean, logvar = torch.chunk(moments, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    std = torch.exp(0.5 * logvar)
    return mean, logvar, std, (mean + std * noise if noise is not None else None)


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def norm_err(got, ref64):
    """max |got - ref| / max |ref|"""
    return float((got.double() - ref64).abs().max() / ref64.abs().max())
