"""LightGlue on the device: the drop-in for `lightglue.LightGlue(features="superpoint")` (cvg/LightGlue: lightglue/lightglue.py) that the reference's
LightGlueMatcher builds behind SuperPoint at metrics/epipolar.py:85.

    from videogpa_amd.lightglue import LightGlue
    net = LightGlue.from_pretrained(".../weights").cuda()
    out = net({"image0": feats0, "image1": feats1})      # upstream's dict: matches0, matches1, matching_scores0/1, matches, scores, stop, prune0/1
    outs = net.match_batch(extractor.extract_clip(frames))   # every consecutive pair of a clip as ONE padded batch, one dict per pair

Inference only, fp32 activations.  All of it is csrc/lightglue.hip: the dense Linears and sim = md0 md1^T (exact fp32 MFMA, every element one fixed sum
over k: a vendor GEMM changes its summation order with the number of rows, and a batched pair must equal its own B = 1 call bit for bit), the attention (fp32 operands read in place from the GEMM output, rotary and scale in the loader, fp16 MFMA as upstream's flash path computes in fp16),
the positional encoding, LayerNorm + GELU, the confidences, point pruning and the assignment with filter_matches.  Both images of a pair share every
GEMM and every launch: a sample's activations are one [Mmax + Nmax, .] block.  cat[x, msg] is never formed: the residual stream is the left half of a
[.,512] buffer and the out_proj / to_out GEMM writes the right half.  Pairs of a batch stop and prune on their own: after every layer ONE small vector
(stop counts and row counts) is read from the device, the pairs that stopped are assigned with that layer's log_assignment and leave the batch.
Weights are LOCAL files only, nothing is ever fetched.

Restated from memory and NOT pinned (lightglue is not a dependency; DESIGN.md section 5m has the list): the state-dict names, the defaults below, the
pruning thresholds, the confidence-threshold formula and the fp16 cast of the flash path."""
import math
import os

import torch
import torch.nn as nn

from . import ops
from ._nn import _PackedCache, read_state_file as _read

WEIGHT_FILES = ("superpoint_lightglue.pth", "superpoint_lightglue.safetensors")
DEFAULT_CONF = {"name": "lightglue", "input_dim": 256, "descriptor_dim": 256, "add_scale_ori": False, "n_layers": 9, "num_heads": 4, "flash": True,
                "mp": False, "depth_confidence": 0.95, "width_confidence": 0.99, "filter_threshold": 0.1, "weights": None}
DIM, HEADS = 256, 4


def confidence_threshold(layer_index, n_layers):
    """upstream's LightGlue.confidence_threshold: clip(0.8 + 0.1 exp(-4 i / n_layers), 0, 1)"""
    return min(max(0.8 + 0.1 * math.exp(-4.0 * layer_index / n_layers), 0.0), 1.0)


def qkv_feature_index(head, dim, which):
    """the output feature of Wqkv that holds element `dim` of head `head` of q (which = 0), k (1) or v (2): upstream's unflatten(-1, (4, 64, 3))"""
    return head * 192 + dim * 3 + which


def _f32(x):
    """the fp32 value torch compares an fp32 tensor against when given this Python scalar, as a Python float"""
    return float(torch.tensor(x, dtype=torch.float32))


def _ffn():
    return nn.Sequential(nn.Linear(2 * DIM, 2 * DIM), nn.LayerNorm(2 * DIM), nn.GELU(), nn.Linear(2 * DIM, DIM))


class _SelfBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.Wqkv, self.out_proj, self.ffn = nn.Linear(DIM, 3 * DIM), nn.Linear(DIM, DIM), _ffn()


class _CrossBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.to_qk, self.to_v, self.to_out, self.ffn = nn.Linear(DIM, DIM), nn.Linear(DIM, DIM), nn.Linear(DIM, DIM), _ffn()


class _Layer(nn.Module):
    def __init__(self):
        super().__init__()
        self.self_attn, self.cross_attn = _SelfBlock(), _CrossBlock()


class _Assignment(nn.Module):
    def __init__(self):
        super().__init__()
        self.matchability, self.final_proj = nn.Linear(DIM, 1), nn.Linear(DIM, DIM)


class _Token(nn.Module):
    def __init__(self):
        super().__init__()
        self.token = nn.Sequential(nn.Linear(DIM, 1), nn.Sigmoid())


class _Posenc(nn.Module):
    def __init__(self):
        super().__init__()
        self.Wr = nn.Linear(2, 32, bias=False)


class LightGlue(nn.Module):
    pruning_keypoint_thresholds = {"cpu": -1, "mps": -1, "cuda": 1024, "flash": 1536}

    def __init__(self, features="superpoint", pretrained=False, weights_path=None, seed=0, **conf):
        """Upstream's configuration keywords and defaults; unknown keys raise.  Only features="superpoint" is built.  pretrained=False is a seeded random
        network (tests, benchmarks); `weights_path` is upstream's superpoint_lightglue.pth, a local file."""
        super().__init__()
        unknown = set(conf) - set(DEFAULT_CONF)
        if unknown:
            raise TypeError(f"LightGlue: unknown configuration {sorted(unknown)}")
        if features != "superpoint":
            raise NotImplementedError(f"LightGlue(features={features!r}): only 'superpoint' is implemented (no DISK / ALIKED / SIFT / DoGHardNet)")
        self.conf = c = {**DEFAULT_CONF, **conf}
        if c["input_dim"] != DIM or c["descriptor_dim"] != DIM or c["num_heads"] != HEADS:
            raise NotImplementedError("LightGlue: input_dim = descriptor_dim = 256 with 4 heads only (input_proj is the identity)")
        if c["add_scale_ori"]:
            raise NotImplementedError("LightGlue: add_scale_ori is not implemented")
        if c["mp"]:
            raise NotImplementedError("LightGlue: mp (autocast) is not implemented: activations are fp32, the attention products fp16")
        if not c["flash"]:
            raise NotImplementedError("LightGlue: flash=False is not implemented: the attention kernel computes in fp16 as upstream's flash path does")
        if not 1 <= int(c["n_layers"]) <= 9:
            raise NotImplementedError("LightGlue: 1..9 layers")
        L = self.n_layers = int(c["n_layers"])
        self.posenc = _Posenc()
        self.transformers = nn.ModuleList([_Layer() for _ in range(L)])
        self.log_assignment = nn.ModuleList([_Assignment() for _ in range(L)])
        self.token_confidence = nn.ModuleList([_Token() for _ in range(L - 1)])
        self.register_buffer("confidence_thresholds", torch.tensor([confidence_threshold(i, L) for i in range(L)], dtype=torch.float32))
        self._packed = _PackedCache()
        if pretrained:
            if weights_path is None:
                raise RuntimeError(f"LightGlue(pretrained=True) needs a local weight file and never downloads: weights_path = upstream's {WEIGHT_FILES[0]} "
                                   "(LightGlue.from_pretrained(dir) finds it in a directory); LightGlue(pretrained=False) is a seeded random network")
            self.load_state_dict(_read(weights_path))
        else:
            self._seeded_init(seed)
        self.requires_grad_(False)
        self.eval()

    def compile(self, *a, **k):
        raise NotImplementedError("LightGlue.compile (static lengths) is not implemented: the kernels take variable lengths as they are")

    def _seeded_init(self, seed=0):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name == "posenc.Wr.weight":
                    p.copy_(torch.randn(p.shape, generator=g))
                elif ".ffn.1." in name:
                    p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
                elif p.dim() == 2:
                    p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
                else:
                    p.copy_(0.1 * torch.randn(p.shape, generator=g))

    @staticmethod
    def _module_spelling(sd):
        """the released checkpoint spells the blocks self_attn.{i}.* / cross_attn.{i}.*; upstream renames them to transformers.{i}.* on load"""
        out = {}
        for k, v in sd.items():
            p = k.split(".")
            if p[0] in ("self_attn", "cross_attn") and len(p) > 2 and p[1].isdigit():
                k = ".".join(["transformers", p[1], p[0]] + p[2:])
            out[k] = v
        return out

    def load_state_dict(self, state_dict, strict=True, **kw):
        return super().load_state_dict(self._module_spelling(state_dict), strict=strict, **kw)

    @classmethod
    def from_pretrained(cls, path, **kw):
        """superpoint_lightglue.pth / superpoint_lightglue.safetensors from one LOCAL directory (or that file itself)"""
        path = os.fspath(path)
        if os.path.isdir(path):
            found = [os.path.join(path, f) for f in WEIGHT_FILES if os.path.isfile(os.path.join(path, f))]
            if not found:
                raise FileNotFoundError(f"{path}: needs {' or '.join(WEIGHT_FILES)}; from_pretrained reads local files only")
            path = found[0]
        elif not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: no such weight file or directory; from_pretrained reads local files only")
        return cls(pretrained=True, weights_path=path, **kw)

    def pruning_min_kpts(self):
        """upstream's pruning_min_kpts on a CUDA / ROCm device with flash=True"""
        return self.pruning_keypoint_thresholds["flash"]

    # ---- kernel-layout copies --------------------------------------------------------------------------------------------------------------
    def packed(self):
        params = list(self.parameters())

        def lin(m):
            return m.weight.detach().float().contiguous(), m.bias.detach().float().contiguous()   # [N][K] as torch keeps it: lg_gemm's second operand

        def make():
            layers = []
            for t in self.transformers:
                s, c = t.self_attn, t.cross_attn
                to_qkv = (torch.cat([c.to_qk.weight, c.to_v.weight], 0).detach().float().contiguous(),   # to_qk | to_v as one GEMM
                          torch.cat([c.to_qk.bias, c.to_v.bias], 0).detach().float().contiguous())
                blk = lambda b: {"f0": lin(b.ffn[0]), "ln": (b.ffn[1].weight.detach().float().contiguous(), b.ffn[1].bias.detach().float().contiguous()),
                                 "eps": b.ffn[1].eps, "f3": lin(b.ffn[3])}
                layers.append({"Wqkv": lin(s.Wqkv), "out_proj": lin(s.out_proj), "self": blk(s), "to_qkv": to_qkv, "to_out": lin(c.to_out), "cross": blk(c)})
            row = lambda m: (m.weight.detach().float().reshape(-1).contiguous(), float(m.bias.detach().float()))
            return {"layers": layers, "Wr": self.posenc.Wr.weight.detach().float().contiguous(),
                    "assign": [{"match": row(a.matchability), "final": lin(a.final_proj)} for a in self.log_assignment],
                    "token": [row(t.token[0]) for t in self.token_confidence],
                    "thr": [float(v) for v in self.confidence_thresholds.float().cpu()]}
        return self._packed.get("all", params, make)

    # ---- checks ----------------------------------------------------------------------------------------------------------------------------
    def _check_feats(self, f, what):
        for key in ("keypoints", "descriptors"):
            if key not in f:
                raise ValueError(f"LightGlue: {what} needs '{key}'")
        kp, d = f["keypoints"], f["descriptors"]
        if kp.dtype != torch.float32 or d.dtype != torch.float32:
            raise ValueError(f"LightGlue: fp32 inputs only, {what} has {kp.dtype} keypoints and {d.dtype} descriptors")
        if torch.is_grad_enabled() and (kp.requires_grad or d.requires_grad):
            raise RuntimeError("LightGlue on the device is forward only: call it under torch.no_grad()")
        if not kp.is_cuda or not d.is_cuda:
            raise RuntimeError("videogpa_amd.lightglue.LightGlue runs on the GPU only (no CPU fallback)")
        if not self.posenc.Wr.weight.is_cuda:
            raise RuntimeError("LightGlue: the module's weights are not on the GPU (no CPU fallback): call .cuda() first")
        if kp.dim() != 3 or kp.shape[2] != 2 or d.dim() != 3 or d.shape[2] != DIM or d.shape[:2] != kp.shape[:2]:
            raise ValueError(f"LightGlue: {what} holds keypoints [B,N,2] and descriptors [B,N,256], got {tuple(kp.shape)} and {tuple(d.shape)}")
        if kp.shape[1] > ops.LG_MAX_N:
            raise NotImplementedError(f"LightGlue: at most {ops.LG_MAX_N} keypoints per image")

    # ---- the network -----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _ffn_block(p, st, seg):
        buf = st["buf"]
        u = ops.lg_gemm(buf, p["f0"][0], bias=p["f0"][1], seg=seg)
        h = ops.lg_ln_gelu(u, *p["ln"], seg, eps=p["eps"], resid=buf[..., :DIM], resid_bias=p["f3"][1])
        ops.lg_gemm(h, p["f3"][0], out=buf[..., :DIM], accumulate=True, seg=seg)                     # x += h W3^T (its bias went in with the row pass)

    def _layer(self, i, st, S0):
        p = self.packed()["layers"][i]
        buf, cs, sn, c0, c1 = st["buf"], st["cos"], st["sin"], st["c0"], st["c1"]
        B, R = buf.shape[:2]
        seg = (S0, c0, c1)
        x, msg = buf[..., :DIM], buf[..., DIM:]
        ctx = torch.empty(B, R, DIM, device=buf.device, dtype=torch.float32)
        # self block: both images in one launch, q / k / v read in place from the interleaved Wqkv output
        qkv = ops.lg_gemm(x, p["Wqkv"][0], bias=p["Wqkv"][1], seg=seg).view(B, R, HEADS, 64, 3)
        dirs = []
        for sl, n in ((slice(0, S0), c0), (slice(S0, R), c1)):
            rope = (cs[:, sl], sn[:, sl])
            dirs.append({"q": qkv[:, sl, :, :, 0], "k": qkv[:, sl, :, :, 1], "v": qkv[:, sl, :, :, 2], "nq": n, "nk": n, "rope_q": rope, "rope_k": rope,
                         "out": ctx[:, sl]})
        ops.lg_attention(dirs)
        ops.lg_gemm(ctx, p["out_proj"][0], out=msg, bias=p["out_proj"][1], seg=seg)
        self._ffn_block(p["self"], st, seg)
        # cross block: both directions in one launch
        qkv = ops.lg_gemm(x, p["to_qkv"][0], bias=p["to_qkv"][1], seg=seg).view(B, R, 2, HEADS, 64)
        qk, v = qkv[:, :, 0], qkv[:, :, 1]
        a, b = slice(0, S0), slice(S0, R)
        ops.lg_attention([{"q": qk[:, a], "k": qk[:, b], "v": v[:, b], "nq": c0, "nk": c1, "out": ctx[:, a]},
                          {"q": qk[:, b], "k": qk[:, a], "v": v[:, a], "nq": c1, "nk": c0, "out": ctx[:, b]}], q_premul=64 ** -0.25)
        ops.lg_gemm(ctx, p["to_out"][0], out=msg, bias=p["to_out"][1], seg=seg)
        self._ffn_block(p["cross"], st, seg)

    def _assign(self, i, st, rows, S0, want_scores):
        """log_assignment[i] and filter_matches for the batch rows `rows` (None: all) -> the device tensors of ops.lg_assign, prune0 / prune1 added"""
        P = self.packed()["assign"][i]
        sel = (lambda t: t) if rows is None else (lambda t: t.index_select(0, rows))
        buf, ind, c0, c1 = sel(st["buf"]), sel(st["ind"]), sel(st["c0"]), sel(st["c1"])
        B, R = buf.shape[:2]
        x = buf[..., :DIM]
        md = ops.lg_gemm(x, P["final"][0], bias=P["final"][1], seg=(S0, c0, c1))
        # md / 256^0.25 on both sides = sim / 16: a power of two, exact
        sim = ops.lg_gemm(md[:, :S0], md[:, S0:], out=torch.zeros(B, S0, R - S0, device=buf.device), alpha=0.0625, seg=(S0, c0, None), ncount=c1)
        _, z = ops.lg_confidence(x, *P["match"], (S0, c0, c1), want_conf=False, want_z=True)
        out = ops.lg_assign(sim, z[:, :S0].contiguous(), z[:, S0:].contiguous(), c0, c1, _f32(self.conf["filter_threshold"]),
                            ind[:, :S0].contiguous(), ind[:, S0:].contiguous(), M0=S0, N0=R - S0, want_scores=want_scores)
        out["prune0"], out["prune1"], out["sim"] = sel(st["prune0"]).clone(), sel(st["prune1"]).clone(), sim
        return out

    def _run(self, kp0, d0, n0, size0, kp1, d1, n1, size1, taps=None, want_scores=False):
        """kp [B,Nmax,2], d [B,Nmax,256] padded, n = Python lists of counts (all >= 1) -> a list of per-pair result dicts (device tensors, sliced)"""
        P = self.packed()
        dev = kp0.device
        B, S0, N1 = kp0.shape[0], kp0.shape[1], kp1.shape[1]
        R = S0 + N1
        L = self.n_layers
        i32 = dict(device=dev, dtype=torch.int32)
        st = {"buf": torch.zeros(B, R, 2 * DIM, device=dev), "cos": torch.zeros(B, R, 32, device=dev), "sin": torch.zeros(B, R, 32, device=dev),
              "c0": torch.tensor(n0, **i32), "c1": torch.tensor(n1, **i32),
              "ind": torch.cat([torch.arange(S0, **i32), torch.arange(N1, **i32)])[None].repeat(B, 1),
              "prune0": torch.ones(B, S0, **i32), "prune1": torch.ones(B, N1, **i32)}
        st["buf"][:, :S0, :DIM] = d0
        st["buf"][:, S0:, :DIM] = d1
        ops.lg_posenc(kp0.contiguous(), st["c0"], P["Wr"], size0, out=(st["cos"][:, :S0], st["sin"][:, :S0]))
        ops.lg_posenc(kp1.contiguous(), st["c1"], P["Wr"], size1, out=(st["cos"][:, S0:], st["sin"][:, S0:]))
        do_stop, do_prune = self.conf["depth_confidence"] > 0, self.conf["width_confidence"] > 0
        pth = self.pruning_min_kpts()
        active = list(range(B))                                        # the pair behind every batch row
        num_points = [n0[j] + n1[j] for j in range(B)]                # upstream's quirk: the ORIGINAL count, pruned points count as confident
        cur0, cur1 = list(n0), list(n1)
        spare = None
        done = []                                                      # (pairs, layer, device outputs)
        tap = (lambda k, v: taps.setdefault(k, []).append((list(active), v))) if taps is not None else (lambda k, v: None)
        for i in range(L):
            self._layer(i, st, S0)
            if taps is not None:
                tap("desc", st["buf"][..., :DIM].clone())
            if i == L - 1:
                done.append((list(active), i, self._assign(i, st, None, S0, want_scores)))
                break
            if not do_stop and not (do_prune and any(a > pth or b > pth for a, b in zip(cur0, cur1))):
                continue                                               # nothing can stop and no side can shrink (counts only fall): no host read
            seg = (S0, st["c0"], st["c1"])
            x = st["buf"][..., :DIM]
            below = torch.zeros(len(active), **i32)
            conf = None
            if do_stop:
                conf, _ = ops.lg_confidence(x, *P["token"][i], seg, thr=P["thr"][i], below=below)
                tap("conf", conf)
            host = torch.cat([below, st["c0"], st["c1"]]).tolist()     # the one host read of the layer
            nb = len(active)
            cur0, cur1 = host[nb:2 * nb], host[2 * nb:]
            if do_stop:
                ratio = 1.0 - torch.tensor(host[:nb], dtype=torch.float32) / torch.tensor([num_points[j] for j in active], dtype=torch.float32)
                stop = (ratio > self.conf["depth_confidence"]).tolist()                              # torch's own fp32 comparison
                if any(stop):
                    rows = [r for r in range(nb) if stop[r]]
                    rt = None if len(rows) == nb else torch.tensor(rows, device=dev)
                    done.append(([active[r] for r in rows], i, self._assign(i, st, rt, S0, want_scores)))
                    keep_rows = [r for r in range(nb) if not stop[r]]
                    if not keep_rows:
                        break
                    kt = torch.tensor(keep_rows, device=dev)
                    st = {k: v.index_select(0, kt) for k, v in st.items()}
                    conf = conf.index_select(0, kt)
                    spare = None
                    active = [active[r] for r in keep_rows]
                    cur0, cur1 = [cur0[r] for r in keep_rows], [cur1[r] for r in keep_rows]
            if do_prune and any(a > pth or b > pth for a, b in zip(cur0, cur1)):
                seg = (S0, st["c0"], st["c1"])
                x = st["buf"][..., :DIM]
                msig, _ = ops.lg_confidence(x, *P["assign"][i]["match"], seg)
                if spare is None:
                    spare = {k: torch.zeros_like(st[k]) for k in ("buf", "cos", "sin", "ind", "c0", "c1")}
                keep = ops.lg_prune(conf if conf is not None else msig, msig, P["thr"][i] if conf is not None else -1.0,
                                    _f32(1 - self.conf["width_confidence"]), pth, x, spare["buf"][..., :DIM], (st["cos"], st["sin"]),
                                    (spare["cos"], spare["sin"]), st["ind"], spare["ind"], (st["prune0"], st["prune1"]), seg, (spare["c0"], spare["c1"]),
                                    want_keep=taps is not None)
                tap("keep", keep)
                for k in spare:
                    st[k], spare[k] = spare[k], st[k]
        counts = torch.cat([o["count"] for _, _, o in done]).tolist() if done else []                # one read at the end: the match counts
        res = [None] * B
        at = 0
        for pairs, layer, o in done:
            for r, j in enumerate(pairs):
                k = counts[at]
                at += 1
                res[j] = {"matches0": o["matches0"][r, :n0[j]].long(), "matches1": o["matches1"][r, :n1[j]].long(),
                          "matching_scores0": o["matching_scores0"][r, :n0[j]], "matching_scores1": o["matching_scores1"][r, :n1[j]],
                          "matches": o["matches"][r, :k].long(), "scores": o["scores"][r, :k], "stop": layer + 1,
                          "prune0": o["prune0"][r, :n0[j]].long(), "prune1": o["prune1"][r, :n1[j]].long()}
                if not do_prune:
                    res[j]["prune0"] = torch.ones_like(res[j]["matching_scores0"]) * L
                    res[j]["prune1"] = torch.ones_like(res[j]["matching_scores1"]) * L
                if want_scores:
                    res[j]["log_assignment"], res[j]["sim"] = o["log_assignment"][r], o["sim"][r]
        return res

    def _empty(self, m, n, dev):
        L = self.n_layers
        z = lambda k, dt: torch.zeros(k, device=dev, dtype=dt)
        ones = (lambda k: torch.ones(k, device=dev, dtype=torch.int64)) if self.conf["width_confidence"] > 0 else (lambda k: torch.ones(k, device=dev) * L)
        return {"matches0": z(m, torch.int64) - 1, "matches1": z(n, torch.int64) - 1, "matching_scores0": z(m, torch.float32),
                "matching_scores1": z(n, torch.float32), "matches": torch.zeros(0, 2, device=dev, dtype=torch.int64), "scores": z(0, torch.float32),
                "stop": 0, "prune0": ones(m), "prune1": ones(n)}

    def _pairs(self, pairs, taps=None, want_scores=False):
        """pairs: [(feats0, feats1)] with a batch axis of 1 each -> one result dict per pair (no batch axis).  Pairs with an empty side launch nothing."""
        dev = pairs[0][0]["keypoints"].device
        cnt = [(f0["keypoints"].shape[1], f1["keypoints"].shape[1]) for f0, f1 in pairs]
        live = [j for j, (a, b) in enumerate(cnt) if a > 0 and b > 0]
        out = [self._empty(a, b, dev) for a, b in cnt]
        if live:
            Mmax, Nmax = max(cnt[j][0] for j in live), max(cnt[j][1] for j in live)

            def pad(side, key, width, N):
                t = torch.zeros(len(live), N, width, device=dev)
                for r, j in enumerate(live):
                    t[r, :cnt[j][side]] = pairs[j][side][key][0]
                return t

            def sizes(side):
                s = [pairs[j][side].get("image_size") for j in live]
                if all(v is None for v in s):
                    return None
                if any(v is None for v in s):
                    raise ValueError("LightGlue: image_size is given for every pair of a batch or for none")
                return torch.cat([v.reshape(1, 2).float() for v in s]).to(dev).contiguous()
            res = self._run(pad(0, "keypoints", 2, Mmax), pad(0, "descriptors", DIM, Mmax), [cnt[j][0] for j in live], sizes(0),
                            pad(1, "keypoints", 2, Nmax), pad(1, "descriptors", DIM, Nmax), [cnt[j][1] for j in live], sizes(1), taps, want_scores)
            for r, j in enumerate(live):
                out[j] = res[r]
        return out

    def forward(self, data, taps=None, want_scores=False):
        """upstream's call: data = {"image0": feats0, "image1": feats1}, each with keypoints [B,N,2], descriptors [B,N,256] and optionally image_size
        [B,2] -> upstream's dict with a batch axis (matches and scores: one tensor per sample).  Unlike upstream every sample of a batch stops and prunes
        on its own, so `stop` is an int for B = 1 and a list for B > 1."""
        f0, f1 = data["image0"], data["image1"]
        self._check_feats(f0, "image0")
        self._check_feats(f1, "image1")
        B = f0["keypoints"].shape[0]
        if f1["keypoints"].shape[0] != B or B < 1:
            raise ValueError("LightGlue: image0 and image1 hold the same number of samples")
        one = lambda f, b: {k: (v[b:b + 1] if isinstance(v, torch.Tensor) else v) for k, v in f.items()}
        with torch.no_grad():
            res = self._pairs([(one(f0, b), one(f1, b)) for b in range(B)], taps, want_scores)
        out = {k: torch.stack([r[k] for r in res]) for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "prune0", "prune1")}
        out["matches"], out["scores"] = [r["matches"] for r in res], [r["scores"] for r in res]
        out["stop"] = res[0]["stop"] if B == 1 else [r["stop"] for r in res]
        if want_scores:
            out["log_assignment"], out["sim"] = [r.get("log_assignment") for r in res], [r.get("sim") for r in res]
        return out

    def match_batch(self, feats_list, taps=None):
        """The per-frame dicts of SuperPoint.extract_clip (batch axis 1 each) -> one upstream-style dict (batch axis 1) per consecutive pair, all pairs
        run as one padded batch; each equals its own B = 1 call."""
        if len(feats_list) < 2:
            return []
        for t, f in enumerate(feats_list):
            self._check_feats(f, f"frame {t}")
            if f["keypoints"].shape[0] != 1:
                raise ValueError("LightGlue.match_batch: every frame's features carry a batch axis of 1")
        with torch.no_grad():
            res = self._pairs([(feats_list[t], feats_list[t + 1]) for t in range(len(feats_list) - 1)], taps)
        return [{k: (v[None] if isinstance(v, torch.Tensor) and k not in ("matches", "scores") else ([v] if k in ("matches", "scores") else v))
                 for k, v in r.items()} for r in res]
