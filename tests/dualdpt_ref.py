"""What the DualDPT goldens (tests/golden/make_golden_dualdpt.py) and their tests share: the reduced configuration, the cases, the seeded recipe for
parameters and inputs (the state is too large to commit: it is regenerated from the recipe and checked against per-tensor float64 sums stored in the
golden), and a torch restatement of Depth Anything 3's DualDPT head (depth_anything_3/model/dualdpt.py, dpt.py, utils/head_utils.py) written from the
formulas over a plain state dict, in whatever dtype the state dict and the tokens carry (float64 for the yardstick, fp32 for d32).  NCHW with F.conv2d /
F.interpolate: nothing of the device path is shared.  tests/test_dualdpt_host.py pins it on the reference's goldens."""
import math
import zlib

import torch
import torch.nn.functional as F

PATCH = 14
CFG = dict(dim_in=32, features=32, out_channels=[16, 16, 32, 32])
SEED = 23
# name -> (B, S, (H, W))
CASES = {"A": (1, 3, (42, 56)), "B": (2, 2, (28, 42))}
OUTPUTS = ("depth", "depth_conf", "ray", "ray_conf")


# ------------------------------------------------------------------------------------------------------------------------ parameters and inputs
def seeded_tensor(name, shape, seed):
    """One parameter, a function of (name, shape, seed) alone.  Every matrix is N(0, 1) / sqrt(fan_in) (a ConvTranspose2d sums over its input channels
    only): the residual sums then keep the signal at O(1) down the chains (a gain of 1.6 on top put the depth logits at -500 .. 28); biases ~ 0.1;
    LayerNorm weights 1 + 0.1 N(0, 1); the final auxiliary 1x1 (output_conv2_aux.N.5) x 4: behind a LayerNorm its input is O(1) whatever comes before
    it, and at the plain scale the ray_conf logit stays within a narrow band.  With SEED = 23 every logit of both cases spans several units and both
    signs (the generator prints and stores the ranges); seeds 21 and 22 left the depth logit one-sided."""
    g = torch.Generator().manual_seed((zlib.crc32(name.encode()) + 7919 * seed) & 0x7FFFFFFF)
    shape = tuple(shape)
    leaf = name.split(".")[-1]
    if leaf == "bias":
        return 0.1 * torch.randn(shape, generator=g)
    if len(shape) == 1:
        return 1.0 + 0.1 * torch.randn(shape, generator=g)
    fan_in = shape[0] if name.startswith(("resize_layers.0.", "resize_layers.1.")) else math.prod(shape[1:])
    gain = 1.0 * (4.0 if ".output_conv2_aux." in name and name.endswith(".5.weight") else 1.0)
    return torch.randn(shape, generator=g) * gain / math.sqrt(fan_in)


def seeded_state(shapes, seed=SEED):
    """shapes: {name: shape} (a module's own state dict gives them) -> {name: fp32 tensor}"""
    return {k: seeded_tensor(k, s, seed) for k, s in shapes.items()}


def state_sums(state):
    return {k: float(v.double().sum()) for k, v in state.items()}


def check_state_sums(state, sums):
    """the regenerated state is THE state of the golden, or the test fails here and not in a tolerance"""
    assert set(state) == set(sums), sorted(set(state) ^ set(sums))
    for k, v in state.items():
        got = float(v.double().sum())
        assert abs(got - sums[k]) <= 1e-9 * max(1.0, abs(sums[k])), f"seeded recipe drifted from the golden at {k}: {got!r} != {sums[k]!r}"


def features(name, dim_in=CFG["dim_in"]):
    """the four feature tensors [B,S,P,dim_in] of a case (patch tokens only: DepthAnything3Net calls the head with patch_start_idx = 0)"""
    B, S, (H, W) = CASES[name]
    g = torch.Generator().manual_seed(5000 + zlib.crc32(name.encode()) % 1000)
    return [torch.randn(B, S, (H // PATCH) * (W // PATCH), dim_in, generator=g) for _ in range(4)]


def rel(got, want):
    """max-abs error over max-abs of the float64 answer"""
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


# ------------------------------------------------------------------------------------------------------------------------ the head, restated
def uv_embed(width, height, channels, aspect, dtype, ratio=0.1):
    """position_grid_to_embed(create_uv_grid(...)) * ratio -> [channels, height, width] as DA3 computes it (head_utils.py:96-199): the coordinates in
    the feature map's dtype, omega in float32, the angles in their product's dtype, and the embedding itself fp32 (`emb.float()`) whatever that is"""
    diag = (aspect ** 2 + 1.0) ** 0.5
    sx, sy = aspect / diag, 1.0 / diag
    xs = torch.linspace(-sx * (width - 1) / width, sx * (width - 1) / width, steps=width, dtype=dtype)
    ys = torch.linspace(-sy * (height - 1) / height, sy * (height - 1) / height, steps=height, dtype=dtype)
    half = channels // 2
    omega = torch.arange(half // 2, dtype=torch.float32)
    omega /= half / 2.0
    omega = 1.0 / 100 ** omega

    def sincos(pos):
        ang = pos[:, None] * omega[None, :]
        return torch.cat([ang.sin(), ang.cos()], dim=1).float()
    ex = sincos(xs)[None, :, :].expand(height, width, half)
    ey = sincos(ys)[:, None, :].expand(height, width, half)
    return (torch.cat([ex, ey], dim=-1) * ratio).permute(2, 0, 1)


def _rcu(sd, p, x):
    """ResidualConvUnit with a ReLU that is not in place: the tensor added back is x"""
    t = F.conv2d(F.relu(x), sd[p + ".conv1.weight"], sd[p + ".conv1.bias"], padding=1)
    return F.conv2d(F.relu(t), sd[p + ".conv2.weight"], sd[p + ".conv2.bias"], padding=1) + x


def _fuse(sd, p, x0, x1, size):
    out = x0
    if x1 is not None:
        out = out + _rcu(sd, p + ".resConfUnit1", x1)
    out = _rcu(sd, p + ".resConfUnit2", out)
    out = F.interpolate(out, size=size, mode="bilinear", align_corners=True)
    return F.conv2d(out, sd[p + ".out_conv.weight"], sd[p + ".out_conv.bias"])


def _chain(sd, rn, suffix):
    out = _fuse(sd, "scratch.refinenet4" + suffix, rn[3], None, rn[2].shape[2:])
    out = _fuse(sd, "scratch.refinenet3" + suffix, out, rn[2], rn[1].shape[2:])
    out = _fuse(sd, "scratch.refinenet2" + suffix, out, rn[1], rn[0].shape[2:])
    return _fuse(sd, "scratch.refinenet1" + suffix, out, rn[0], (2 * rn[0].shape[2], 2 * rn[0].shape[3]))


def aux_tail(sd, x, aspect, level=3, pos_embed=True, prefix="scratch.output_conv2_aux."):
    """x [N, C, h, w] -> (preds [N, h, w, od - 1] linear, conf [N, h, w] = 1 + exp): dualdpt.py:250-258"""
    p = f"{prefix}{level}"
    if pos_embed:
        x = x + uv_embed(x.shape[3], x.shape[2], x.shape[1], aspect, x.dtype)[None]
    t = F.conv2d(x, sd[p + ".0.weight"], sd[p + ".0.bias"], padding=1).permute(0, 2, 3, 1)
    t = F.relu(F.layer_norm(t, (t.shape[-1],), sd[p + ".2.weight"], sd[p + ".2.bias"], 1e-5))
    t = F.linear(t, sd[p + ".5.weight"].flatten(1), sd[p + ".5.bias"])
    return t[..., :-1], 1 + t[..., -1].exp()


def head(sd, feats, H, W, patch_start_idx=0, aux=True, pos_embed=True):
    """feats: four [B,S,P,C] token tensors -> {depth [B,S,H',W'], depth_conf, ray [B,S,8ph,8pw,6], ray_conf [B,S,8ph,8pw]}"""
    ph, pw = H // PATCH, W // PATCH
    B, S = feats[0].shape[:2]
    stages = []
    for i in range(4):
        x = feats[i].reshape(B * S, *feats[i].shape[2:])[:, patch_start_idx:]
        C = x.shape[-1]
        x = F.layer_norm(x, (C,), sd["norm.weight"], sd["norm.bias"], 1e-5)
        x = x.permute(0, 2, 1).reshape(B * S, C, ph, pw)
        x = F.conv2d(x, sd[f"projects.{i}.weight"], sd[f"projects.{i}.bias"])
        if pos_embed:
            x = x + uv_embed(pw, ph, x.shape[1], W / H, x.dtype)[None]
        if i == 0:
            x = F.conv_transpose2d(x, sd["resize_layers.0.weight"], sd["resize_layers.0.bias"], stride=4)
        elif i == 1:
            x = F.conv_transpose2d(x, sd["resize_layers.1.weight"], sd["resize_layers.1.bias"], stride=2)
        elif i == 3:
            x = F.conv2d(x, sd["resize_layers.3.weight"], sd["resize_layers.3.bias"], stride=2, padding=1)
        stages.append(x)
    rn = [F.conv2d(f, sd[f"scratch.layer{i + 1}_rn.weight"], padding=1) for i, f in enumerate(stages)]
    out = F.conv2d(_chain(sd, rn, ""), sd["scratch.output_conv1.weight"], sd["scratch.output_conv1.bias"], padding=1)
    out = F.interpolate(out, size=(ph * PATCH, pw * PATCH), mode="bilinear", align_corners=True)
    if pos_embed:
        out = out + uv_embed(out.shape[3], out.shape[2], out.shape[1], W / H, out.dtype)[None]
    out = F.relu(F.conv2d(out, sd["scratch.output_conv2.0.weight"], sd["scratch.output_conv2.0.bias"], padding=1))
    out = F.conv2d(out, sd["scratch.output_conv2.2.weight"], sd["scratch.output_conv2.2.bias"]).permute(0, 2, 3, 1)
    shape = lambda t: t.reshape(B, S, *t.shape[1:])
    result = {"depth": shape(out[..., :-1].exp().squeeze(-1)), "depth_conf": shape(1 + out[..., -1].exp())}
    if aux:
        a = _chain(sd, rn, "_aux")
        for j in range(5):
            a = F.conv2d(a, sd[f"scratch.output_conv1_aux.3.{j}.weight"], sd[f"scratch.output_conv1_aux.3.{j}.bias"], padding=1)
        ray, conf = aux_tail(sd, a, W / H, pos_embed=pos_embed)
        result["ray"], result["ray_conf"] = shape(ray), shape(conf)
    return result
