"""Plain-torch restatement of transformers' T5EncoderModel (modeling_t5.py, the eager attention path) in the T5-v1.1 configuration, and the fp64
references of the three kernels of csrc/t5.hip.  Nothing from the library under test.  Runs in fp64, fp32 or bf16, on whatever device the state dict
is on (tests: the CPU; tools/t5_bench.py moves it to the GPU as the B side of its A/B).

mode="bf16" issues upstream's operation sequence on bf16 tensors, so every result is rounded where the reference's bf16 module rounds it:
    T5LayerNorm          variance of x.float(); x * rsqrt(var + eps) in fp32; ROUND to bf16; weight * that; ROUND
    q, k, v, o, wi, wo   bf16 GEMM outputs
    scores               q k^T ROUNDED to bf16; + (position_bias + mask) in bf16, ROUND; softmax in fp32, weights ROUNDED to bf16; weights @ v, ROUND
    gelu_new             0.5 * x * (1 + tanh(sqrt(2/pi) * (x + 0.044715 * x^3))), every elementwise operation rounded to bf16
    residual adds        in bf16
mode="fp64" / "fp32" run the same sequence in that type (the upcasts become no-ops): fp64 is the oracle."""
import math

import torch

from attn_tol import RND

DTYPES = {"fp64": torch.float64, "fp32": torch.float32, "bf16": torch.bfloat16}
CFG_KEYS = ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_heads", "relative_attention_num_buckets", "relative_attention_max_distance",
            "layer_norm_epsilon")


def make_cfg(**kw):
    cfg = dict(vocab_size=64, d_model=64, d_kv=64, d_ff=96, num_layers=2, num_heads=2, relative_attention_num_buckets=32,
               relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")
    cfg.update(kw)
    return cfg


def state_dict_names(cfg):
    names = ["shared.weight", "encoder.embed_tokens.weight"]
    for i in range(cfg["num_layers"]):
        p = f"encoder.block.{i}.layer."
        names += [p + f"0.SelfAttention.{n}.weight" for n in "qkvo"]
        if i == 0:
            names.append(p + "0.SelfAttention.relative_attention_bias.weight")
        names.append(p + "0.layer_norm.weight")
        names += [p + f"1.DenseReluDense.{n}.weight" for n in ("wi_0", "wi_1", "wo")]
        names.append(p + "1.layer_norm.weight")
    names.append("encoder.final_layer_norm.weight")
    return names


def seeded_state_dict(cfg, seed=0, norm_jitter=0.3, bias_std=math.sqrt(2.0), q_gain=1.0, dtype=torch.bfloat16, device="cpu"):
    """upstream's initialisation scales (T5PreTrainedModel._init_weights at factor 1) from a seeded generator, with what that initialisation leaves
    degenerate perturbed: norm weights 1 +- norm_jitter (uniform), the relative-position table N(0, bias_std^2).  q_gain multiplies the q weights
    (sharp softmax rows).  Values are rounded to `dtype`; drawn one tensor at a time on `device` (the real configuration is 4.8 B parameters)."""
    g = torch.Generator(device=device).manual_seed(seed)
    D, H, F, V = cfg["d_model"], cfg["num_heads"], cfg["d_ff"], cfg["vocab_size"]
    inner = H * cfg["d_kv"]

    def rn(*shape, std=1.0):
        return (torch.randn(*shape, generator=g, device=device, dtype=torch.float32) * std).to(dtype)

    def norm():
        return (1.0 + norm_jitter * (2.0 * torch.rand(D, generator=g, device=device, dtype=torch.float32) - 1.0)).to(dtype)

    sd = {"shared.weight": rn(V, D)}
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    for i in range(cfg["num_layers"]):
        p = f"encoder.block.{i}.layer."
        sd[p + "0.SelfAttention.q.weight"] = rn(inner, D, std=q_gain * (D * cfg["d_kv"]) ** -0.5)
        sd[p + "0.SelfAttention.k.weight"] = rn(inner, D, std=D ** -0.5)
        sd[p + "0.SelfAttention.v.weight"] = rn(inner, D, std=D ** -0.5)
        sd[p + "0.SelfAttention.o.weight"] = rn(D, inner, std=inner ** -0.5)
        if i == 0:
            sd[p + "0.SelfAttention.relative_attention_bias.weight"] = rn(cfg["relative_attention_num_buckets"], H, std=bias_std)
        sd[p + "0.layer_norm.weight"] = norm()
        sd[p + "1.DenseReluDense.wi_0.weight"] = rn(F, D, std=D ** -0.5)
        sd[p + "1.DenseReluDense.wi_1.weight"] = rn(F, D, std=D ** -0.5)
        sd[p + "1.DenseReluDense.wo.weight"] = rn(D, F, std=F ** -0.5)
        sd[p + "1.layer_norm.weight"] = norm()
    sd["encoder.final_layer_norm.weight"] = norm()
    return sd


# ---------------------------------------------------------------------------------------------- upstream's pieces
def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """T5Attention._relative_position_bucket, bidirectional"""
    num_buckets //= 2
    relative_buckets = (relative_position > 0).to(torch.long) * num_buckets
    relative_position = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    large = max_exact + (torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return relative_buckets + torch.where(is_small, relative_position, large)


def position_bias(table, S, num_buckets, max_distance):
    """T5Attention.compute_bias: table [buckets, H] -> [1, H, S, S]"""
    ctx = torch.arange(S, dtype=torch.long, device=table.device)[:, None]
    mem = torch.arange(S, dtype=torch.long, device=table.device)[None, :]
    return table[relative_position_bucket(mem - ctx, num_buckets, max_distance)].permute(2, 0, 1).unsqueeze(0)


def layer_norm(x, w, eps, mode):
    var = (x.float() if mode == "bf16" else x).pow(2).mean(-1, keepdim=True)
    h = x * torch.rsqrt(var + eps)
    return w * h.to(w.dtype)


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def prepare(sd, mode, device=None):
    """the state dict in the mode's type (on `device`)"""
    return {k: v.to(device=device or v.device, dtype=DTYPES[mode]) for k, v in sd.items()}


def forward(sd, cfg, input_ids, attention_mask=None, mode="fp64", prepared=False):
    """-> last_hidden_state [B,S,d_model] in the mode's type"""
    dt = DTYPES[mode]
    if not prepared:
        sd = prepare(sd, mode)
    dev = sd["shared.weight"].device
    ids = input_ids.to(dev)
    B, S = ids.shape
    H, dk, eps = cfg["num_heads"], cfg["d_kv"], cfg["layer_norm_epsilon"]
    x = sd["shared.weight"][ids]
    pb = position_bias(sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], S, cfg["relative_attention_num_buckets"],
                       cfg["relative_attention_max_distance"])
    if attention_mask is not None:
        ext = (1.0 - attention_mask.to(dev)[:, None, None, :].to(dt)) * torch.finfo(dt).min
        pb = pb + ext
    lin = torch.nn.functional.linear
    for i in range(cfg["num_layers"]):
        p = f"encoder.block.{i}.layer."
        n = layer_norm(x, sd[p + "0.layer_norm.weight"], eps, mode)
        q, k, v = (lin(n, sd[p + f"0.SelfAttention.{c}.weight"]).view(B, S, H, dk).transpose(1, 2) for c in "qkv")
        scores = torch.matmul(q, k.transpose(3, 2))
        scores = scores + pb
        w = torch.softmax(scores.float() if mode == "bf16" else scores, dim=-1).type_as(scores)
        a = torch.matmul(w, v).transpose(1, 2).contiguous().view(B, S, H * dk)
        x = x + lin(a, sd[p + "0.SelfAttention.o.weight"])
        n = layer_norm(x, sd[p + "1.layer_norm.weight"], eps, mode)
        g = gelu_new(lin(n, sd[p + "1.DenseReluDense.wi_0.weight"])) * lin(n, sd[p + "1.DenseReluDense.wi_1.weight"])
        x = x + lin(g, sd[p + "1.DenseReluDense.wo.weight"])
    return layer_norm(x, sd["encoder.final_layer_norm.weight"], eps, mode)


def rel_err(got, o64):
    """|| got - o64 ||_2 / || o64 ||_2 over the whole output"""
    o64 = o64.double()
    return float((got.detach().double().to(o64.device) - o64).norm() / o64.norm())


# ---------------------------------------------------------------------------------------------- the attention kernel alone
def bias_delta_from_table(table, S, num_buckets=32, max_distance=128):
    """table [buckets, H] -> fp32 [H, 2S-1], entry [h, d + S - 1] for d = j - i, through upstream's bucket function"""
    d = torch.arange(-(S - 1), S, dtype=torch.long)
    return table.float()[relative_position_bucket(d, num_buckets, max_distance)].t().contiguous()


def attn_sums64(q, k, v, bias_row, keep=None):
    """One (batch, head) slice in fp64 with the sums tests/attn_tol.py::o_tol takes (the dict of tests/attn_ref64.py, forward part): q, k, v [S,64];
    bias_row fp32 [2S-1] indexed by j - i + S - 1; keep bool [S] or None.  Scores are in NATURAL units here (T5 has no scale and the kernel takes
    exp of s - max); o_tol wants the score error in log2 units, so snorm is returned in log2 units: log2(e) * (|q_i| max_j |k_j| + 16 / D *
    max_j |s_ij + bias_ij|) -- the second term is the ONE fp32 addition per score of the bias (2^-24 relative of the sum), written so that
    score_err(snorm, D) = (D / 16) 2^-24 snorm is the sum of both."""
    q, k, v = q.double(), k.double(), v.double()
    S, D = q.shape
    i = torch.arange(S)
    bias = bias_row.double()[(i[None, :] - i[:, None]) + S - 1]                # [i, j]
    s = q @ k.t() + bias
    valid = torch.ones(S, dtype=torch.bool) if keep is None else keep.bool()
    s = s.masked_fill(~valid[None, :], float("-inf"))
    w = torch.softmax(s, dim=-1)
    e2 = (RND * RND) * w * w
    o = w @ v
    sabs = s.masked_fill(~valid[None, :], 0.0).abs().amax(-1)
    snorm = math.log2(math.e) * (q.norm(dim=-1) * k[valid].norm(dim=-1).max() + (16.0 / D) * sabs)
    return {"o": o, "e2": e2.sum(-1), "e2v": e2 @ v, "e2v2": e2 @ (v * v), "wabsv": w @ v.abs(), "snorm": snorm, "conc": (w * w).sum(-1), "D": D,
            "rounded_rowsum": True, "rows": i, "Skv": S, "bwd": False}


# ---------------------------------------------------------------------------------------------- the row kernel and the gated GELU
def rms64(x_new, w, eps):
    x = x_new.double()
    return w.double() * x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32)))


def gated_gelu64(u):
    """u [..., 2F] -> gelu_tanh(a) b in fp64, gelu as x sigmoid(2z) (tests/row_tol.py::gelu_ref64: the tanh form cancels below x = -8.3 in fp64)"""
    F = u.shape[-1] // 2
    a, b = u[..., :F].double(), u[..., F:].double()
    return a * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (a + 0.044715 * a ** 3)) * b
