"""Torch restatement of the VGGT camera and DPT heads (vggt/heads/camera_head.py, dpt_head.py, head_act.py, utils.py), written from the
formulas over a plain state dict, in whatever dtype the state dict and the tokens carry (float64 for the yardstick, fp32 for d32).  NCHW
with F.conv2d / F.interpolate: nothing of the device path is shared.  tests/test_vggt_heads_host.py pins it on the float64 goldens."""
import torch
import torch.nn.functional as F


def uv_embed(width, height, channels, aspect, dtype, ratio=0.1):
    """position_grid_to_embed(create_uv_grid(...)) * ratio -> [channels, height, width]; the embedding itself is fp32 upstream (`emb.float()`)
    whatever the dtype of the coordinates"""
    diag = (aspect ** 2 + 1.0) ** 0.5
    sx, sy = aspect / diag, 1.0 / diag
    xs = torch.linspace(-sx * (width - 1) / width, sx * (width - 1) / width, steps=width, dtype=dtype)
    ys = torch.linspace(-sy * (height - 1) / height, sy * (height - 1) / height, steps=height, dtype=dtype)
    half = channels // 2
    omega = 1.0 / 100 ** (torch.arange(half // 2, dtype=torch.float64) / (half / 2.0))

    def sincos(pos):
        ang = pos.double()[:, None] * omega[None, :]
        return torch.cat([ang.sin(), ang.cos()], dim=1).float()
    ex = sincos(xs)[None, :, :].expand(height, width, half)
    ey = sincos(ys)[:, None, :].expand(height, width, half)
    return (torch.cat([ex, ey], dim=-1) * ratio).permute(2, 0, 1)


def inverse_log(y):
    return torch.sign(y) * torch.expm1(torch.abs(y))


def _rcu(sd, p, x):
    """ResidualConvUnit with its in-place ReLU: the tensor added back is relu(x)"""
    r = F.relu(x)
    t = F.conv2d(r, sd[p + ".conv1.weight"], sd[p + ".conv1.bias"], padding=1)
    return F.conv2d(F.relu(t), sd[p + ".conv2.weight"], sd[p + ".conv2.bias"], padding=1) + r


def _fuse(sd, p, x0, x1, size):
    out = x0
    if x1 is not None:
        out = out + _rcu(sd, p + ".resConfUnit1", x1)
    out = _rcu(sd, p + ".resConfUnit2", out)
    out = F.interpolate(out, size=size, mode="bilinear", align_corners=True)
    return F.conv2d(out, sd[p + ".out_conv.weight"], sd[p + ".out_conv.bias"])


def dpt_features(sd, tokens_list, hw, patch_start_idx, patch_size=14, layer_idx=(0, 1, 2, 3), pos_embed=True):
    """-> the output of scratch.output_conv1, [B*S, features/2, 8ph, 8pw]"""
    H, W = hw
    ph, pw = H // patch_size, W // patch_size
    feats = []
    for i, li in enumerate(layer_idx):
        x = tokens_list[li][:, :, patch_start_idx:]
        B, S, P, C = x.shape
        x = F.layer_norm(x.reshape(B * S, P, C), (C,), sd["norm.weight"], sd["norm.bias"], 1e-5)
        x = x.permute(0, 2, 1).reshape(B * S, C, ph, pw)
        x = F.conv2d(x, sd[f"projects.{i}.weight"], sd[f"projects.{i}.bias"])
        if pos_embed:
            x = x + uv_embed(pw, ph, x.shape[1], W / H, x.dtype)[None].to(x.device)
        if i == 0:
            x = F.conv_transpose2d(x, sd["resize_layers.0.weight"], sd["resize_layers.0.bias"], stride=4)
        elif i == 1:
            x = F.conv_transpose2d(x, sd["resize_layers.1.weight"], sd["resize_layers.1.bias"], stride=2)
        elif i == 3:
            x = F.conv2d(x, sd["resize_layers.3.weight"], sd["resize_layers.3.bias"], stride=2, padding=1)
        feats.append(x)
    rn = [F.conv2d(f, sd[f"scratch.layer{i + 1}_rn.weight"], padding=1) for i, f in enumerate(feats)]
    out = _fuse(sd, "scratch.refinenet4", rn[3], None, rn[2].shape[2:])
    out = _fuse(sd, "scratch.refinenet3", out, rn[2], rn[1].shape[2:])
    out = _fuse(sd, "scratch.refinenet2", out, rn[1], rn[0].shape[2:])
    out = _fuse(sd, "scratch.refinenet1", out, rn[0], (2 * rn[0].shape[2], 2 * rn[0].shape[3]))
    return F.conv2d(out, sd["scratch.output_conv1.weight"], sd["scratch.output_conv1.bias"], padding=1)


def dpt_tail(sd, x, hw, patch_size=14, activation="exp", pos_embed=True):
    """x [N, C, h, w] -> (preds [N, H', W', od-1], conf [N, H', W']) at H' = (H // patch) * patch"""
    H, W = hw
    size = ((H // patch_size) * patch_size, (W // patch_size) * patch_size)
    out = F.interpolate(x, size=size, mode="bilinear", align_corners=True)
    if pos_embed:
        out = out + uv_embed(size[1], size[0], out.shape[1], W / H, out.dtype)[None].to(out.device)
    out = F.relu(F.conv2d(out, sd["scratch.output_conv2.0.weight"], sd["scratch.output_conv2.0.bias"], padding=1))
    out = F.conv2d(out, sd["scratch.output_conv2.2.weight"], sd["scratch.output_conv2.2.bias"]).permute(0, 2, 3, 1)
    xyz, conf = out[..., :-1], out[..., -1]
    preds = torch.exp(xyz) if activation == "exp" else inverse_log(xyz)
    return preds, 1 + conf.exp()


def dpt_head(sd, tokens_list, hw, patch_start_idx, patch_size=14, layer_idx=(0, 1, 2, 3), activation="exp", pos_embed=True):
    B, S = tokens_list[layer_idx[0]].shape[:2]
    x = dpt_features(sd, tokens_list, hw, patch_start_idx, patch_size, layer_idx, pos_embed)
    preds, conf = dpt_tail(sd, x, hw, patch_size, activation, pos_embed)
    return preds.reshape(B, S, *preds.shape[1:]), conf.reshape(B, S, *conf.shape[1:])


def _attention(sd, p, x, num_heads):
    B, N, C = x.shape
    D = C // num_heads
    qkv = F.linear(x, sd[p + ".qkv.weight"], sd[p + ".qkv.bias"]).reshape(B, N, 3, num_heads, D).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    a = torch.softmax((q @ k.transpose(-2, -1)) * D ** -0.5, dim=-1)
    return F.linear((a @ v).transpose(1, 2).reshape(B, N, C), sd[p + ".proj.weight"], sd[p + ".proj.bias"])


def _block(sd, p, x, num_heads):
    C = x.shape[-1]
    n1 = F.layer_norm(x, (C,), sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], 1e-5)
    x = x + sd[p + ".ls1.gamma"] * _attention(sd, p + ".attn", n1, num_heads)
    n2 = F.layer_norm(x, (C,), sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], 1e-5)
    m = F.linear(F.gelu(F.linear(n2, sd[p + ".mlp.fc1.weight"], sd[p + ".mlp.fc1.bias"])), sd[p + ".mlp.fc2.weight"], sd[p + ".mlp.fc2.bias"])
    return x + sd[p + ".ls2.gamma"] * m


def camera_head(sd, tokens_list, num_heads, trunk_depth, num_iterations=4):
    """-> list of [B, S, 9]: translation and quaternion linear, field of view through ReLU"""
    t = tokens_list[-1][:, :, 0]
    B, S, C = t.shape
    t = F.layer_norm(t, (C,), sd["token_norm.weight"], sd["token_norm.bias"], 1e-5)
    pred, out = None, []
    for _ in range(num_iterations):
        inp = sd["empty_pose_tokens"].expand(B, S, -1) if pred is None else pred
        emb = F.linear(inp, sd["embed_pose.weight"], sd["embed_pose.bias"])
        shift, scale, gate = F.linear(F.silu(emb), sd["poseLN_modulation.1.weight"], sd["poseLN_modulation.1.bias"]).chunk(3, dim=-1)
        x = gate * (F.layer_norm(t, (C,), None, None, 1e-6) * (1 + scale) + shift) + t
        for i in range(trunk_depth):
            x = _block(sd, f"trunk.{i}", x, num_heads)
        x = F.layer_norm(x, (C,), sd["trunk_norm.weight"], sd["trunk_norm.bias"], 1e-5)
        delta = F.linear(F.gelu(F.linear(x, sd["pose_branch.fc1.weight"], sd["pose_branch.fc1.bias"])), sd["pose_branch.fc2.weight"],
                         sd["pose_branch.fc2.bias"])
        pred = delta if pred is None else pred + delta
        out.append(torch.cat([pred[..., :7], F.relu(pred[..., 7:])], dim=-1))
    return out


def rel_err(got, want):
    """max-abs error over max-abs of the float64 answer"""
    want = want.double()
    return float((got.double().cpu() - want.cpu()).abs().max() / want.abs().max())
