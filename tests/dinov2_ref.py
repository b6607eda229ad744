"""DINOv2 (vggt/layers/vision_transformer.py, block.py, attention.py at the aggregator's settings: block_chunks=0, LayerScale, erf-GELU Mlp, no
QK-norm, no RoPE) restated with torch ops over a plain state dict, for the tests and tools: it runs in any dtype (float64 for the kernels' own
accuracy, bf16 autocast for the rounding-noise yardstick d16 and as the torch composition the benchmark times).  Also the seeded parameter recipe of
the DINOv2 goldens: states too large to commit are regenerated from it and checked against per-tensor float64 sums stored in the golden."""
import math
import zlib

import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------------------------------ parameters
def seeded_tensor(name, shape, seed):
    """One parameter of the golden recipe, a function of (name, shape, seed) alone (CPU generator, fp32), so the order of a state dict does not matter.
    What the timm initialisation leaves trivial (zero biases, unit LayerNorm weights and gammas, 1e-6 tokens) is made large enough that dropping it
    shows: biases ~ 0.1, LayerNorm weights 1 +- 0.2, gammas in 0.5 .. 1.5, class / register / camera tokens ~ 0.5, position table ~ 0.3.  Matrices keep
    timm's scale (std 0.02), qkv.weight 4 x that so that the softmax is not flat (and the aggregator's own blocks, which sit behind gammas of 0.01
    upstream, likewise); the patch projection keeps Conv2d's default uniform range."""
    g = torch.Generator().manual_seed((zlib.crc32(name.encode()) + 7919 * seed) & 0x7FFFFFFF)
    shape = tuple(shape)
    leaf = name.split(".")[-1]
    if name.endswith("mask_token"):
        return torch.zeros(shape)
    if leaf == "gamma":
        return 0.5 + torch.rand(shape, generator=g)
    if leaf in ("cls_token", "register_tokens", "camera_token", "register_token"):
        return 0.5 * torch.randn(shape, generator=g)
    if leaf == "pos_embed":
        return 0.3 * torch.randn(shape, generator=g)
    if leaf == "bias":
        return 0.1 * torch.randn(shape, generator=g)
    if leaf == "weight" and len(shape) == 1:
        return 1.0 + 0.2 * (2.0 * torch.rand(shape, generator=g) - 1.0)
    if leaf == "weight" and len(shape) == 4:
        return (2.0 * torch.rand(shape, generator=g) - 1.0) / math.sqrt(math.prod(shape[1:]))
    if leaf == "weight":
        wide = name.endswith("qkv.weight") or name.startswith(("frame_blocks.", "global_blocks."))
        return torch.randn(shape, generator=g) * (0.08 if wide else 0.02)
    raise KeyError(f"no recipe for {name} {shape}")


def seeded_state(shapes, seed, bf16_representable=False):
    """shapes: {name: shape} (a module's own state dict gives them) -> {name: fp32 tensor}"""
    out = {k: seeded_tensor(k, s, seed) for k, s in shapes.items()}
    return {k: v.to(torch.bfloat16).float() for k, v in out.items()} if bf16_representable else out


def state_sums(state):
    return {k: float(v.double().sum()) for k, v in state.items()}


def check_state_sums(state, sums):
    """the regenerated state is THE state of the golden, or the test fails here and not in a tolerance"""
    assert set(state) == set(sums), sorted(set(state) ^ set(sums))
    for k, v in state.items():
        got = float(v.double().sum())
        assert abs(got - sums[k]) <= 1e-9 * max(1.0, abs(sums[k])), f"seeded recipe drifted from the golden at {k}: {got!r} != {sums[k]!r}"


# ------------------------------------------------------------------------------------------------------------------------ forward
def pos_table(pos_embed, w0, h0, antialias=True, offset=0.0):
    """interpolate_pos_encoding (:180-212) for a w0 x h0 patch grid (first, second spatial axis), computed in pos_embed's dtype"""
    N = pos_embed.shape[1] - 1
    M = int(math.sqrt(N))
    if w0 * h0 == N and w0 == h0:
        return pos_embed
    kw = {"scale_factor": (float(w0 + offset) / M, float(h0 + offset) / M)} if offset else {"size": (w0, h0)}
    patch = F.interpolate(pos_embed[:, 1:].reshape(1, M, M, -1).permute(0, 3, 1, 2), mode="bicubic", antialias=antialias, **kw)
    return torch.cat((pos_embed[:, :1], patch.permute(0, 2, 3, 1).reshape(1, w0 * h0, -1)), dim=1)


def prepare_tokens(sd, x, patch, pos):
    """prepare_tokens_with_masks (:214-226) from torch ops: conv, transpose, cat, add, cat.  pos = the [1, 1+P, C] table."""
    t = F.conv2d(x, sd["patch_embed.proj.weight"].to(x.dtype), sd["patch_embed.proj.bias"].to(x.dtype), stride=patch).flatten(2).transpose(1, 2)
    t = torch.cat((sd["cls_token"].to(t.dtype).expand(t.shape[0], -1, -1), t), dim=1)
    t = t + pos.to(t.dtype)
    if sd.get("register_tokens") is not None:
        t = torch.cat((t[:, :1], sd["register_tokens"].to(t.dtype).expand(t.shape[0], -1, -1), t[:, 1:]), dim=1)
    return t


def block(sd, pre, x, heads, eps=1e-6):
    C = x.shape[-1]
    B, N, _ = x.shape
    n = F.layer_norm(x, (C,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], eps)
    qkv = F.linear(n, sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"]).reshape(B, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    a = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(B, N, C)
    a = F.linear(a, sd[pre + "attn.proj.weight"], sd[pre + "attn.proj.bias"])
    x = x + a * sd[pre + "ls1.gamma"]
    n = F.layer_norm(x, (C,), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], eps)
    m = F.linear(F.gelu(F.linear(n, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"])), sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"])
    return x + m * sd[pre + "ls2.gamma"]


def forward(sd, x, patch, heads, antialias=True, offset=0.0, table=None):
    """DinoVisionTransformer.forward_features(x, masks=None) -> the reference's dict.  sd and x in one dtype (float64 / float32), or fp32 under a bf16
    autocast context the caller opened.  `table`: a precomputed position table (the benchmark keeps the interpolation out of the timed region)."""
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    R = 0 if sd.get("register_tokens") is None else sd["register_tokens"].shape[1]
    if table is None:
        table = pos_table(sd["pos_embed"].float(), x.shape[2] // patch, x.shape[3] // patch, antialias, offset)     # fp32 whatever the model, as upstream
    t = prepare_tokens(sd, x, patch, table)
    for i in range(depth):
        t = block(sd, f"blocks.{i}.", t, heads)
    xn = F.layer_norm(t, (t.shape[-1],), sd["norm.weight"], sd["norm.bias"], 1e-6)
    return {"x_norm_clstoken": xn[:, 0], "x_norm_regtokens": xn[:, 1:R + 1], "x_norm_patchtokens": xn[:, R + 1:], "x_prenorm": t, "masks": None}
