"""What the Depth Anything 3 goldens (tests/golden/make_golden_da3.py) and their tests share: the reduced configurations, the seeded recipe for parameters
and inputs (states too large to commit are regenerated from it and checked against per-tensor float64 sums stored in the golden), and torch restatements,
in any dtype, of the small formulas the kernels of csrc/da3.hip are checked against (selection metrics, view order)."""
import torch

import dinov2_ref

PATCH, IMG_SIZE = 14, 70            # a 5 x 5 position table: 70 x 70 frames take it as it is, the other shapes interpolate
CONFIGS = {
    # depth 4: a tap before the alternation starts (1), one at alt_start (2, local), one global (3); the state itself is stored
    "a": dict(embed_dim=64, num_heads=1, depth=4, alt_start=2, qknorm_start=2, rope_start=2, out_layers=[1, 2, 3], seed=11),
    # an odd alt_start: the first alternating block is global and the local half of its tap is the block before it with the camera token written in;
    # QK-norm starts one block before RoPE
    "b": dict(embed_dim=128, num_heads=2, depth=6, alt_start=3, qknorm_start=2, rope_start=3, out_layers=[3, 4, 5], seed=12),
    # DINOv2-small's width
    "c": dict(embed_dim=384, num_heads=6, depth=6, alt_start=2, qknorm_start=2, rope_start=2, out_layers=[2, 5], seed=13),
}
# name -> (B, S, (H, W), ref_view_strategy, caller's cam_token?); "saddle*" cases get their input seed from the generator's search
CASES = {
    "s1": (1, 1, (70, 70), "saddle_balanced", False),
    "s2": (2, 2, (42, 56), "saddle_balanced", False),
    "first": (1, 4, (56, 42), "first", False),
    "middle": (1, 4, (70, 70), "middle", False),
    "saddle0": (1, 4, (42, 56), "saddle_balanced", False),
    "saddle1": (1, 4, (42, 56), "saddle_balanced", False),
    "saddle_b2": (2, 4, (42, 56), "saddle_balanced", False),      # the two kept inputs as one batch: one reference view per batch element
    "camtok": (1, 4, (42, 56), "saddle_balanced", True),          # a caller's camera token: no selection
}
CASES_OF = {tag: tuple(CASES) for tag in CONFIGS}


def load_case(golden_dir, tag, name):
    """one case of one configuration; where the outputs of all out layers together pass the size limit of a committed file, the generator stores them in
    one file per out layer (da3_TAG_NAME_L<i>.pt = (out64[i], out32[i])) and they are put back here"""
    import os
    c = torch.load(os.path.join(golden_dir, f"da3_{tag}_{name}.pt"))
    if "out64" not in c:
        layers = [torch.load(os.path.join(golden_dir, f"da3_{tag}_{name}_L{i}.pt")) for i in range(c["layer_files"])]
        c["out64"], c["out32"] = [l[0] for l in layers], [l[1] for l in layers]
    return c


def seeded_state(shapes, seed):
    """the backbone's parameters: dinov2_ref's recipe (q_norm / k_norm are LayerNorms like the others, camera_token a token)"""
    return dinov2_ref.seeded_state(shapes, seed)


def cam_dec_state(shapes, seed):
    """CameraDec's parameters: the same recipe, the matrices scaled to 1 / sqrt(fan_in) so that the outputs are O(1); the fields of view stay around
    1 rad (bias + 1, a tenth of the weight): a zero behind their ReLU would put a focal length of 1e6 x the image size into the comparison"""
    out = {}
    for k, s in shapes.items():
        v = dinov2_ref.seeded_tensor("cam_dec." + k, s, seed)
        if len(s) == 2:
            v = v * (1.0 / 0.02) / float(s[1]) ** 0.5 * (0.1 if k == "fc_fov.0.weight" else 1.0)
        out[k] = v + 1.0 if k == "fc_fov.0.bias" else v
    return out


def images(seed, B, S, hw):
    """normalised frames [B,S,3,H,W] fp32: smooth per-view structure plus noise, so that the views' class tokens differ by more than rounding"""
    g = torch.Generator().manual_seed(7000 + seed)
    H, W = hw
    base = torch.randn(B, S, 3, 1, 1, generator=g)
    ramp = torch.linspace(-1, 1, H).view(1, 1, 1, H, 1) * torch.randn(B, S, 3, 1, 1, generator=g) \
        + torch.linspace(-1, 1, W).view(1, 1, 1, 1, W) * torch.randn(B, S, 3, 1, 1, generator=g)
    return (base + ramp + 0.5 * torch.randn(B, S, 3, H, W, generator=g)).contiguous()


def cam_tokens(seed, B, S, C):
    return 0.5 * torch.randn(B, S, C, generator=torch.Generator().manual_seed(9000 + seed))


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------------------ small formulas
def order(ref, S):
    """reordered position -> original view: [ref, 0, .., ref-1, ref+1, ..]"""
    return [ref] + [j for j in range(S) if j != ref]


def inverse_order(ref, S):
    o = order(ref, S)
    return [o.index(t) for t in range(S)]


def minmax(m):
    lo, hi = m.min(dim=1, keepdim=True).values, m.max(dim=1, keepdim=True).values
    return (m - lo) / (hi - lo + 1e-8)


def select_metrics(cls):
    """class tokens [B,S,C] in the dtype to evaluate in -> (sim_score, norm, var, balance, sim_range), each [B,S]: the mean off-diagonal cosine
    similarity, the norm, the variance of the normalised token, sum |minmax(metric) - 0.5| over the three, and the range of the similarity row"""
    S = cls.shape[1]
    norm = cls.norm(dim=-1)
    f = cls / norm[..., None]
    sim = f @ f.transpose(1, 2) - torch.eye(S, dtype=cls.dtype, device=cls.device)
    sim_score, var = sim.sum(-1) / (S - 1), f.var(dim=-1)
    balance = (minmax(sim_score) - 0.5).abs() + (minmax(norm) - 0.5).abs() + (minmax(var) - 0.5).abs()
    return sim_score, norm, var, balance, sim.max(-1).values - sim.min(-1).values


def select(cls, strategy):
    """-> the reference view per batch element, int64 [B] (cls float64 for the answer)"""
    B, S = cls.shape[:2]
    if S <= 1 or strategy == "first":
        return torch.zeros(B, dtype=torch.long)
    if strategy == "middle":
        return torch.full((B,), S // 2, dtype=torch.long)
    m = select_metrics(cls)
    return (m[3].argmin(dim=1) if strategy == "saddle_balanced" else m[4].argmax(dim=1)).cpu()


def invert_rigid(m):
    """[..., 3, 4] rigid transform [A | t] -> its inverse [A^T | -A^T t], in m's dtype"""
    a, t = m[..., :3], m[..., 3]
    return torch.cat([a.transpose(-1, -2), -torch.einsum("...ji,...j->...i", a, t)[..., None]], dim=-1)


def pinhole(fov_hw, hw):
    """fields of view [..., 2] = (vertical, horizontal) in radians and the image size (H, W) -> intrinsics [..., 3, 3] in fov's dtype: focal length =
    half the size over tan(half the angle), the tangent floored at 1e-6, principal point at the centre"""
    half = torch.tensor([hw[0] / 2.0, hw[1] / 2.0], dtype=fov_hw.dtype)
    f = half / torch.tan(0.5 * fov_hw).clamp_min(1e-6)
    K = torch.zeros(*fov_hw.shape[:-1], 3, 3, dtype=fov_hw.dtype)
    K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2], K[..., 2, 2] = f[..., 1], f[..., 0], half[1], half[0], 1.0
    return K


def rotation(q):
    """scalar-last quaternions [..., 4] (any norm) -> rotation matrices: ((w^2 - |v|^2) I + 2 v v^T + 2 w [v]x) / |q|^2"""
    v, w = q[..., :3], q[..., 3]
    eye = torch.eye(3, dtype=q.dtype)
    cross = torch.zeros(*q.shape[:-1], 3, 3, dtype=q.dtype)
    cross[..., 0, 1], cross[..., 0, 2], cross[..., 1, 2] = -v[..., 2], v[..., 1], -v[..., 0]
    cross = cross - cross.transpose(-1, -2)
    num = (w * w - (v * v).sum(-1))[..., None, None] * eye + 2.0 * v[..., :, None] * v[..., None, :] + 2.0 * w[..., None, None] * cross
    return num / (q * q).sum(-1)[..., None, None]
