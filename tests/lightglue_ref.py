"""A torch restatement of upstream LightGlue (cvg/LightGlue: lightglue/lightglue.py, features="superpoint") written from its definitions, for one
pair (no batch axis), on the CPU.  It imports nothing from videogpa_amd.  `lightglue` is not installed here: every name, default and formula below is
restated from memory and UNPINNED (DESIGN.md section 5m lists them).

Modes:  "f64"   the answer;  "f32"   everything in fp32;  "ref16"  the reference's own arithmetic on its flash path: q, k, v (after rotary and scale)
and the softmax weights are rounded to fp16 around the two attention products, everything else is fp32.
Comparisons against thresholds are torch's own (tensor against Python scalar, or against the fp32 buffer `confidence_thresholds`), so the promotion
rule is torch's.  `variant` selects one deliberately WRONG restatement (tests/test_lightglue_host.py shows the comparisons reject each)."""
import math

import torch
import torch.nn.functional as F

N_LAYERS, HEADS, DIM = 9, 4, 256
DEFAULT_CONF = {"depth_confidence": 0.95, "width_confidence": 0.99, "filter_threshold": 0.1, "pruning_threshold": 1536}
VARIANTS = ("qkv_blocks", "rotate_halves", "cross_scale_twice", "num_points_after_prune", "no_col_softmax")


def confidence_threshold(i, n_layers=N_LAYERS):
    return min(max(0.8 + 0.1 * math.exp(-4.0 * i / n_layers), 0.0), 1.0)


def names():
    """{state-dict name: shape} with the module spelling transformers.{i}.self_attn / cross_attn"""
    out = {"posenc.Wr.weight": (32, 2)}
    for i in range(N_LAYERS):
        s, c = f"transformers.{i}.self_attn.", f"transformers.{i}.cross_attn."
        for k, (o, n) in {s + "Wqkv": (768, 256), s + "out_proj": (256, 256), s + "ffn.0": (512, 512), s + "ffn.3": (256, 512), c + "to_qk": (256, 256),
                          c + "to_v": (256, 256), c + "to_out": (256, 256), c + "ffn.0": (512, 512), c + "ffn.3": (256, 512),
                          f"log_assignment.{i}.matchability": (1, 256), f"log_assignment.{i}.final_proj": (256, 256)}.items():
            out[k + ".weight"], out[k + ".bias"] = (o, n), (o,)
        for k in (s + "ffn.1", c + "ffn.1"):
            out[k + ".weight"], out[k + ".bias"] = (512,), (512,)
        if i < N_LAYERS - 1:
            out[f"token_confidence.{i}.token.0.weight"], out[f"token_confidence.{i}.token.0.bias"] = (1, 256), (1,)
    out["confidence_thresholds"] = (N_LAYERS,)
    return out


def checkpoint_spelling(sd):
    """the released checkpoint's names: self_attn.{i}.* / cross_attn.{i}.* (upstream renames them to transformers.{i}.* on load)"""
    out = {}
    for k, v in sd.items():
        p = k.split(".")
        out[".".join([p[2], p[1]] + p[3:]) if p[0] == "transformers" else k] = v
    return out


def state(seed):
    """scaled-normal weights: N(0, 1 / fan_in) matrices, 0.1 N(0, 1) biases, LayerNorm 1 + 0.1 N / 0.1 N, Wr N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in names().items():
        if k == "confidence_thresholds":
            sd[k] = torch.tensor([confidence_threshold(i) for i in range(N_LAYERS)], dtype=torch.float32)
        elif k == "posenc.Wr.weight":
            sd[k] = torch.randn(shp, generator=g)
        elif ".ffn.1." in k:
            sd[k] = (1.0 if k.endswith("weight") else 0.0) + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("weight"):
            sd[k] = torch.randn(shp, generator=g) / shp[1] ** 0.5
        else:
            sd[k] = 0.1 * torch.randn(shp, generator=g)
    return sd


def matching_state(seed):
    """`state` made to match: small residual updates (ffn.3 x 0.03), a near-identity final projection (15 I + 0.2 W) and matchability bias 3.
    With plain `state` no pair passes the 0.1 filter threshold."""
    sd = state(seed)
    for k in sd:
        if ".ffn.3." in k:
            sd[k] = sd[k] * 0.03
        elif k.endswith("final_proj.weight"):
            sd[k] = 15.0 * torch.eye(DIM) + 0.2 * sd[k]
        elif k.endswith("matchability.bias"):
            sd[k] = torch.full_like(sd[k], 3.0)
    return sd


def stop_state(seed, layer):
    """matching_state whose token confidence at `layer` is sigmoid(~8): the pair stops there"""
    sd = matching_state(seed)
    sd[f"token_confidence.{layer}.token.0.bias"] = torch.full((1,), 8.0)
    return sd


def prune_state(seed, token_bias=1.0, token_gain=100.0, match_gain=2000.0, match_bias=0.0):
    """matching_state with spread-out token confidences (weights x token_gain, bias +1: a share of the points stays below the threshold, so the pair
    does not stop early, the rest is confident) and a sharpened matchability (weights x match_gain): the confident, unmatchable share gets pruned.
    Use with a lowered pruning threshold (64).  With these descriptors a bias of +3 alone makes every token confident and the pair stops at layer 1."""
    sd = matching_state(seed)
    for i in range(N_LAYERS):
        if i < N_LAYERS - 1:
            sd[f"token_confidence.{i}.token.0.weight"] = sd[f"token_confidence.{i}.token.0.weight"] * token_gain
            sd[f"token_confidence.{i}.token.0.bias"] = torch.full((1,), float(token_bias))
        sd[f"log_assignment.{i}.matchability.weight"] = sd[f"log_assignment.{i}.matchability.weight"] * match_gain
        sd[f"log_assignment.{i}.matchability.bias"] = torch.full((1,), float(match_bias))
    return sd


def pair(m, n, seed, extra=0, image_size=True):
    """keypoints0 uniform in a 160 x 120 image with unit-norm random descriptors; image 1 is n <= m of them drawn WITHOUT replacement, moved by
    N(0, 1.5 px), descriptors + 0.05 N(0, 1) renormalised, then `extra` unmatched random points.  gt[j] = the image-0 index of image-1 point j (-1)."""
    g = torch.Generator().manual_seed(seed)
    size = torch.tensor([160.0, 120.0])
    k0 = torch.rand(m, 2, generator=g) * size
    d0 = F.normalize(torch.randn(m, DIM, generator=g), dim=-1)
    sel = torch.randperm(m, generator=g)[:n]
    k1 = k0[sel] + 1.5 * torch.randn(n, 2, generator=g)
    d1 = F.normalize(d0[sel] + 0.05 * torch.randn(n, DIM, generator=g), dim=-1)
    if extra:
        k1 = torch.cat([k1, torch.rand(extra, 2, generator=g) * size])
        d1 = torch.cat([d1, F.normalize(torch.randn(extra, DIM, generator=g), dim=-1)])
        sel = torch.cat([sel, torch.full((extra,), -1, dtype=sel.dtype)])
    out = {"keypoints0": k0, "keypoints1": k1, "descriptors0": d0, "descriptors1": d1, "gt": sel}
    if image_size:
        out["image_size0"], out["image_size1"] = size.clone(), size.clone()
    return out


def normalize_keypoints(k, size=None):
    if size is None:
        size = 1 + k.max(-2).values - k.min(-2).values
    size = size.to(k)
    return (k - (size / 2)[None]) / (size.max(-1).values / 2)


def rotate_half(x, variant=None):
    if variant == "rotate_halves":
        a, b = x.chunk(2, -1)
        return torch.cat((-b, a), -1)
    x = x.unflatten(-1, (-1, 2))
    a, b = x.unbind(-1)
    return torch.stack((-b, a), -1).flatten(-2)


def rope(enc, t, variant=None):
    return t * enc[0] + rotate_half(t, variant) * enc[1]


def posenc(Wr, k):
    p = k @ Wr.t()
    return torch.stack([p.cos(), p.sin()], 0).unsqueeze(-3).repeat_interleave(2, -1)          # [2, 1, N, 64]


def split_qkv(qkv, variant=None):
    """[T,768] -> q, k, v [4,T,64]: upstream's unflatten(-1, (4, 64, 3)), the three of q / k / v the FASTEST axis"""
    if variant == "qkv_blocks":
        q, k, v = qkv.unflatten(-1, (3, HEADS, 64)).permute(1, 2, 0, 3)
        return q, k, v
    t = qkv.unflatten(-1, (HEADS, 64, 3)).transpose(0, 1)
    return t[..., 0], t[..., 1], t[..., 2]


def attention(q, k, v, mode):
    """softmax(q k^T / 8) v; ref16 rounds q, k, v and the weights to fp16 (what the fp16 sdpa of the flash path holds), products in fp32"""
    if mode == "ref16":
        q, k, v = (t.half().float() for t in (q, k, v))
    p = torch.softmax((q @ k.transpose(-1, -2)) * 0.125, -1)
    if mode == "ref16":
        p = p.half().float()
    return p @ v


def _lin(sd, name, x):
    return F.linear(x, sd[name + ".weight"].to(x.dtype), sd[name + ".bias"].to(x.dtype))


def _ffn(sd, p, x, msg):
    h = _lin(sd, p + "ffn.0", torch.cat([x, msg], -1))
    h = F.layer_norm(h, (512,), sd[p + "ffn.1.weight"].to(x.dtype), sd[p + "ffn.1.bias"].to(x.dtype), 1e-5)
    return x + _lin(sd, p + "ffn.3", F.gelu(h))


def self_block(sd, i, x, enc, mode, variant=None):
    p = f"transformers.{i}.self_attn."
    q, k, v = split_qkv(_lin(sd, p + "Wqkv", x), variant)
    ctx = attention(rope(enc, q, variant), rope(enc, k, variant), v, mode)
    return _ffn(sd, p, x, _lin(sd, p + "out_proj", ctx.transpose(0, 1).flatten(1)))


def cross_block(sd, i, x0, x1, mode, variant=None):
    p = f"transformers.{i}.cross_attn."
    heads = lambda t: t.unflatten(-1, (HEADS, 64)).transpose(0, 1)
    s = 64 ** -0.25 if variant != "cross_scale_twice" else 64 ** -0.5
    qk0, qk1 = heads(_lin(sd, p + "to_qk", x0)) * s, heads(_lin(sd, p + "to_qk", x1)) * s
    v0, v1 = heads(_lin(sd, p + "to_v", x0)), heads(_lin(sd, p + "to_v", x1))
    m0 = attention(qk0, qk1, v1, mode).transpose(0, 1).flatten(1)
    m1 = attention(qk1, qk0, v0, mode).transpose(0, 1).flatten(1)
    return _ffn(sd, p, x0, _lin(sd, p + "to_out", m0)), _ffn(sd, p, x1, _lin(sd, p + "to_out", m1))


def log_assignment(sd, i, x0, x1, variant=None):
    """-> (scores [(m+1),(n+1)], sim, z0, z1)"""
    p = f"log_assignment.{i}."
    md0, md1 = _lin(sd, p + "final_proj", x0) / DIM ** 0.25, _lin(sd, p + "final_proj", x1) / DIM ** 0.25
    sim = md0 @ md1.t()
    z0, z1 = _lin(sd, p + "matchability", x0), _lin(sd, p + "matchability", x1)          # [m,1], [n,1]
    m, n = sim.shape
    s = F.log_softmax(sim, 1)
    if variant != "no_col_softmax":
        s = s + F.log_softmax(sim, 0)
    scores = sim.new_zeros(m + 1, n + 1)
    scores[:m, :n] = s + (F.logsigmoid(z0) + F.logsigmoid(z1).t())
    scores[:m, n] = F.logsigmoid(-z0[:, 0])
    scores[m, :n] = F.logsigmoid(-z1[:, 0])
    return scores, sim, z0[:, 0], z1[:, 0]


def filter_matches(scores, th):
    """-> matches0, matches1, mscores0, mscores1 (upstream's filter_matches without the batch axis)"""
    max0, max1 = scores[:-1, :-1].max(1), scores[:-1, :-1].max(0)
    m0, m1 = max0.indices, max1.indices
    i0, i1 = torch.arange(m0.shape[0]), torch.arange(m1.shape[0])
    mutual0, mutual1 = i0 == m1[m0], i1 == m0[m1]
    ms0 = torch.where(mutual0, max0.values.exp(), max0.values.new_zeros(()))
    ms1 = torch.where(mutual1, ms0[m1], ms0.new_zeros(()))
    valid0 = mutual0 & (ms0 > th)
    valid1 = mutual1 & valid0[m1]
    return torch.where(valid0, m0, -1), torch.where(valid1, m1, -1), ms0, ms1


def forward(sd, data, mode="f64", conf=None, variant=None):
    """-> dict: desc [(x0, x1) per layer run, before pruning], conf [(t0, t1)], keep [(mask0 | None, mask1 | None)], msig (the matchability sigmoids behind keep), ind0, ind1, stop, scores (the log
    assignment at the stop layer, over the rows left), sim, matches [K,2] (original indices), mscores [K], matches0, matches1, matching_scores0,
    matching_scores1, prune0, prune1"""
    c = {**DEFAULT_CONF, **(conf or {})}
    dt = torch.float64 if mode == "f64" else torch.float32
    k0 = normalize_keypoints(data["keypoints0"].to(dt), data.get("image_size0"))
    k1 = normalize_keypoints(data["keypoints1"].to(dt), data.get("image_size1"))
    x0, x1 = data["descriptors0"].to(dt), data["descriptors1"].to(dt)
    m, n = x0.shape[0], x1.shape[0]
    Wr = sd["posenc.Wr.weight"].to(dt)
    e0, e1 = posenc(Wr, k0), posenc(Wr, k1)
    do_stop, do_prune = c["depth_confidence"] > 0, c["width_confidence"] > 0
    ind0, ind1 = torch.arange(m), torch.arange(n)
    prune0, prune1 = torch.ones(m, dtype=torch.int64), torch.ones(n, dtype=torch.int64)
    out = {"desc": [], "conf": [], "keep": [], "msig": []}
    thr = sd["confidence_thresholds"]
    t0 = t1 = None
    for i in range(N_LAYERS):
        x0, x1 = self_block(sd, i, x0, e0, mode, variant), self_block(sd, i, x1, e1, mode, variant)
        x0, x1 = cross_block(sd, i, x0, x1, mode, variant)
        out["desc"].append((x0, x1))
        if i == N_LAYERS - 1:
            break
        if do_stop:
            t0 = torch.sigmoid(_lin(sd, f"token_confidence.{i}.token.0", x0))[:, 0]
            t1 = torch.sigmoid(_lin(sd, f"token_confidence.{i}.token.0", x1))[:, 0]
            out["conf"].append((t0, t1))
            num_points = (x0.shape[0] + x1.shape[0]) if variant == "num_points_after_prune" else (m + n)     # upstream: the ORIGINAL count
            ratio = 1.0 - (torch.cat([t0, t1]) < thr[i]).float().sum() / num_points
            if bool(ratio > c["depth_confidence"]):
                break
        masks, sigs = [None, None], [None, None]
        if do_prune:
            for side, (x, t) in enumerate(((x0, t0), (x1, t1))):
                if x.shape[0] > c["pruning_threshold"]:
                    sc = torch.sigmoid(_lin(sd, f"log_assignment.{i}.matchability", x))[:, 0]
                    keep = sc > (1 - c["width_confidence"])
                    if t is not None:
                        keep = keep | (t <= thr[i])
                    masks[side], sigs[side] = keep, sc
            if masks[0] is not None:
                ind0, x0, e0 = ind0[masks[0]], x0[masks[0]], e0[..., masks[0], :]
                prune0[ind0] += 1
            if masks[1] is not None:
                ind1, x1, e1 = ind1[masks[1]], x1[masks[1]], e1[..., masks[1], :]
                prune1[ind1] += 1
        out["keep"].append(tuple(masks))
        out["msig"].append(tuple(sigs))
    scores, sim, z0, z1 = log_assignment(sd, i, x0, x1, variant)
    a0, a1, ms0, ms1 = filter_matches(scores, c["filter_threshold"])
    valid = a0 > -1
    out.update(stop=i + 1, scores=scores, sim=sim, ind0=ind0, ind1=ind1, matches=torch.stack([ind0[valid], ind1[a0[valid]]], -1), mscores=ms0[valid])
    if do_prune:
        m0_, m1_ = torch.full((m,), -1), torch.full((n,), -1)
        m0_[ind0] = torch.where(a0 == -1, -1, ind1[a0.clamp(min=0)])
        m1_[ind1] = torch.where(a1 == -1, -1, ind0[a1.clamp(min=0)])
        s0_, s1_ = ms0.new_zeros(m), ms0.new_zeros(n)
        s0_[ind0], s1_[ind1] = ms0, ms1
        out.update(matches0=m0_, matches1=m1_, matching_scores0=s0_, matching_scores1=s1_, prune0=prune0, prune1=prune1)
    else:
        out.update(matches0=a0, matches1=a1, matching_scores0=ms0, matching_scores1=ms1, prune0=torch.ones_like(ms0) * N_LAYERS,
                   prune1=torch.ones_like(ms1) * N_LAYERS)
    return out


def err(a, b):
    """the section-5d measure: max-abs difference over the max-abs of the reference b"""
    b = b.double()
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300))


def top2_gap(scores):
    """per row of the log assignment without its dustbins: the best score minus the second best (inf for a single column)"""
    s = scores[:-1, :-1]
    if s.shape[1] < 2:
        return torch.full((s.shape[0],), float("inf"), dtype=s.dtype)
    t = s.topk(2, dim=1).values
    return t[:, 0] - t[:, 1]


def steer(data, sd, layer, alpha=0.3):
    """`data` with every descriptor pushed by alpha along token_confidence.{layer}'s weight and renormalised: under prune_state's sharpened token
    confidence the pair becomes confident, and stops, at that layer (the residual updates of matching_state are small, so the push survives)."""
    w = F.normalize(sd[f"token_confidence.{layer}.token.0.weight"][0].float(), dim=0)
    out = dict(data)
    for k in ("descriptors0", "descriptors1"):
        out[k] = F.normalize(data[k] + alpha * w, dim=-1)
    return out
