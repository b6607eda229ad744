"""T5 encoder on the device: transformers' T5EncoderModel (modeling_t5.py) in the T5-v1.1 configuration the CogVideoX pipelines ship as
`text_encoder` -- gated gelu_new feed-forward, RMS-only norms, no linear biases, a relative-position bias learned in block 0 and shared by all blocks,
attention without the 1/sqrt(d) scale.  Reference call sites: train/*/02_encode.py (`pipeline.text_encoder(input_ids)[0]` at max_length 226, no
attention mask) and diffusers' CogVideoXPipeline._get_t5_prompt_embeds; both work unchanged on this module.

State-dict names are upstream's (`shared.weight`, `encoder.embed_tokens.weight` tied to it, `encoder.block.{i}.layer.0.SelfAttention.{q,k,v,o}.weight`,
`encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight`, `encoder.block.{i}.layer.{0,1}.layer_norm.weight`,
`encoder.block.{i}.layer.1.DenseReluDense.{wi_0,wi_1,wo}.weight`, `encoder.final_layer_norm.weight`).

What runs where.  Per block: two row kernels (ops.t5_rms: residual add + T5LayerNorm), one attention kernel (ops.t5_attention), one gated-GELU kernel
(ops.t5_gated_gelu) and four GEMMs on the vendor library through torch (q|k|v as one, o, wi_0|wi_1 as one, wo: bf16 operands, fp32 accumulation, bf16
outputs).  The first norm is fused with the embedding gather (ops.t5_embed_rms).  The fused weights are built once and the q / k / v (wi_0 / wi_1)
parameters become views of them, so nothing is held twice.

DEVIATION from the reference's all-bf16 module: the residual stream is fp32 (as in the VGGT backbone, csrc/dino_stream.hip).  Upstream rounds the
stream to bf16 after every add and the normalised activations twice (x * rsqrt, then * weight); here x stays fp32 between blocks and only GEMM operands
and GEMM outputs are bf16.  tests/test_gpu_t5.py holds the result to the error of the reference's own bf16 arithmetic against fp64.

Forward only, bf16 parameters, no CPU fallback.  Refused: a decoder stack, a non-gated or ReLU feed-forward (T5 v1.0), d_kv != 64, more than 512
tokens, fp16, a mask that is not [B,S].  Tokenisation (sentencepiece string work on the host) stays the caller's."""
import json
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

MAX_TOKENS = ops.T5_MAX_S


class T5Config:
    """the fields of transformers' T5Config that an encoder reads; built from keywords, a dict (config.json) or any object with these attributes"""
    _DEFAULTS = dict(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64, relative_attention_num_buckets=32,
                     relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu", is_decoder=False)

    def __init__(self, config=None, **kw):
        src = {}
        if isinstance(config, dict):
            src = dict(config)
        elif config is not None:
            src = {k: getattr(config, k) for k in self._DEFAULTS if hasattr(config, k)}
        src.update(kw)
        unknown = sorted(k for k in kw if k not in self._DEFAULTS)
        if unknown:
            raise TypeError(f"T5Config: unknown fields {unknown}")
        for k, d in self._DEFAULTS.items():
            setattr(self, k, src.get(k, d))
        if self.is_decoder:
            raise NotImplementedError("videogpa_amd.t5: is_decoder=True (a decoder stack) is not implemented: this is the encoder only")
        ff = str(self.feed_forward_proj)
        if ff not in ("gated-gelu", "gated-gelu_new"):
            raise NotImplementedError(f"videogpa_amd.t5: feed_forward_proj={ff!r}: only the gated gelu_new feed-forward of T5 v1.1 is implemented "
                                      "(T5 v1.0's ReLU / non-gated feed-forward is not)")
        if self.d_kv != 64:
            raise NotImplementedError(f"videogpa_amd.t5: d_kv={self.d_kv}: the attention kernel is head_dim 64 only")
        if self.d_model % 64 or self.d_model > 4096 or self.d_ff % 8:
            raise NotImplementedError(f"videogpa_amd.t5: d_model={self.d_model} (a multiple of 64, at most 4096) / d_ff={self.d_ff} (a multiple of 8)")
        self.dense_act_fn, self.is_gated_act = "gelu_new", True


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """T5Attention._relative_position_bucket(bidirectional=True) on an integer tensor of memory_position - query_position, with upstream's float32
    operations in upstream's order (log of the float32 quotient, divided by the Python float log, times the integer, truncated), so that the
    bucket of every distance is the integer upstream computes."""
    num_buckets //= 2
    buckets = (relative_position > 0).to(torch.long) * num_buckets
    rp = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = rp < max_exact
    large = max_exact + (torch.log(rp.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(is_small, rp, large)


_BUCKETS = {}


def delta_buckets(S, num_buckets=32, max_distance=128):
    """int64 [2S-1] on the host: entry d + S - 1 is the bucket of relative position d = j - i (key minus query), d = -(S-1) .. S-1.  Built once per S."""
    key = (int(S), int(num_buckets), int(max_distance))
    if key not in _BUCKETS:
        _BUCKETS[key] = relative_position_bucket(torch.arange(-(S - 1), S, dtype=torch.long), num_buckets, max_distance)
    return _BUCKETS[key]


class T5LayerNorm(nn.Module):
    def __init__(self, d, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.variance_epsilon = eps
        self._w32 = None

    def w32(self):
        """the weight as the row kernel reads it (fp32; exact for a bf16 parameter), rebuilt when the parameter changed"""
        w = self.weight
        tag = (w.data_ptr(), w._version, w.device)
        if self._w32 is None or self._w32[0] != tag:
            self._w32 = (tag, w.detach().float().contiguous())
        return self._w32[1]


def _fuse(cache, linears):
    """one [sum out, in] weight for several Linear layers that read the same input; the layers' parameters become views of it"""
    ws = [l.weight for l in linears]
    f = cache[0]
    off, ok = 0, f is not None and f.device == ws[0].device and f.dtype == ws[0].dtype
    for w in ws:
        ok = ok and w.data_ptr() == f.data_ptr() + off * f.shape[1] * f.element_size()
        off += w.shape[0]
    if not ok:
        f = torch.cat([w.detach() for w in ws], 0).contiguous()
        off = 0
        for w in ws:
            w.data = f[off:off + w.shape[0]]
            off += w.shape[0]
        cache[0] = f
    return f


class T5Attention(nn.Module):
    def __init__(self, cfg, has_relative_attention_bias):
        super().__init__()
        inner = cfg.num_heads * cfg.d_kv
        self.n_heads = cfg.num_heads
        self.q = nn.Linear(cfg.d_model, inner, bias=False)
        self.k = nn.Linear(cfg.d_model, inner, bias=False)
        self.v = nn.Linear(cfg.d_model, inner, bias=False)
        self.o = nn.Linear(inner, cfg.d_model, bias=False)
        if has_relative_attention_bias:
            self.relative_attention_bias = nn.Embedding(cfg.relative_attention_num_buckets, cfg.num_heads)
        self._qkv = [None]

    def forward(self, n, bias_delta, mask):
        B, S, _ = n.shape
        H = self.n_heads
        qkv = F.linear(n, _fuse(self._qkv, (self.q, self.k, self.v))).view(B, S, 3, H, 64)
        a = ops.t5_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], bias_delta, mask)
        return F.linear(a, self.o.weight)


class T5LayerSelfAttention(nn.Module):
    def __init__(self, cfg, has_relative_attention_bias):
        super().__init__()
        self.SelfAttention = T5Attention(cfg, has_relative_attention_bias)
        self.layer_norm = T5LayerNorm(cfg.d_model, cfg.layer_norm_epsilon)


class T5DenseGatedActDense(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.wi_0 = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.wi_1 = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.wo = nn.Linear(cfg.d_ff, cfg.d_model, bias=False)
        self._wi = [None]

    def forward(self, n):
        return F.linear(ops.t5_gated_gelu(F.linear(n, _fuse(self._wi, (self.wi_0, self.wi_1)))), self.wo.weight)


class T5LayerFF(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.DenseReluDense = T5DenseGatedActDense(cfg)
        self.layer_norm = T5LayerNorm(cfg.d_model, cfg.layer_norm_epsilon)


class T5Block(nn.Module):
    def __init__(self, cfg, has_relative_attention_bias):
        super().__init__()
        self.layer = nn.ModuleList([T5LayerSelfAttention(cfg, has_relative_attention_bias), T5LayerFF(cfg)])


class T5Stack(nn.Module):
    def __init__(self, cfg, embed_tokens):
        super().__init__()
        self.embed_tokens = embed_tokens
        self.block = nn.ModuleList([T5Block(cfg, i == 0) for i in range(cfg.num_layers)])
        self.final_layer_norm = T5LayerNorm(cfg.d_model, cfg.layer_norm_epsilon)


class EncoderOutput:
    """what both call sites read: `.last_hidden_state`, or `[0]`"""

    def __init__(self, last_hidden_state):
        self.last_hidden_state = last_hidden_state

    def __getitem__(self, i):
        return (self.last_hidden_state,)[i]


class T5EncoderModel(nn.Module):
    config_name = "config.json"
    weights_name = "model.safetensors"

    def __init__(self, config=None, **kw):
        super().__init__()
        self.config = config if isinstance(config, T5Config) and not kw else T5Config(config, **kw)
        self.shared = nn.Embedding(self.config.vocab_size, self.config.d_model)
        self.encoder = T5Stack(self.config, nn.Embedding(self.config.vocab_size, self.config.d_model))
        self.encoder.embed_tokens.weight = self.shared.weight              # tied, as upstream
        self._dev_buckets = {}
        self.eval()

    @property
    def dtype(self):
        return self.shared.weight.dtype

    # ------------------------------------------------------------------ loading (local file system only)
    @classmethod
    def from_pretrained(cls, path, subfolder=None, torch_dtype=None, **kw):
        """`T5EncoderModel.from_pretrained(model_path, subfolder="text_encoder", torch_dtype=torch.bfloat16)`: `config.json` plus
        `model.safetensors`, or the shards listed by `model.safetensors.index.json` (`weight_map`: name -> file).  The loader of
        wan_model.WanModel.from_pretrained: a meta skeleton and an assigning strict load (never two copies of a 4.8 B-parameter model), dtype rules
        of upstream (None: float32; a torch.dtype: cast per tensor; "auto": as stored).  A missing `encoder.embed_tokens.weight` is filled from
        `shared.weight` (and the reverse): they are one tensor.  `decoder.*` and `lm_head.*` of a full T5 checkpoint are dropped; any other
        unexpected or missing name is an error.  No hub access: `path` must be a local directory."""
        from safetensors.torch import load_file
        root = os.path.join(path, subfolder) if subfolder else path
        if not os.path.isdir(root):
            raise FileNotFoundError(f"T5EncoderModel.from_pretrained: {root!r} is not a local directory (there is no hub access on this path)")
        with open(os.path.join(root, cls.config_name)) as f:
            cfg = T5Config({k: v for k, v in json.load(f).items() if k in T5Config._DEFAULTS}, **kw)
        index = os.path.join(root, cls.weights_name + ".index.json")
        if os.path.isfile(index):
            with open(index) as f:
                files = sorted(set(json.load(f)["weight_map"].values()))
        elif os.path.isfile(os.path.join(root, cls.weights_name)):
            files = [cls.weights_name]
        else:
            files = sorted(f for f in os.listdir(root) if f.endswith(".safetensors"))
        if not files:
            raise FileNotFoundError(f"no .safetensors weights under {root}")
        sd = {}
        for fn in files:
            sd.update(load_file(os.path.join(root, fn)))
        sd = {k: v for k, v in sd.items() if not k.startswith(("decoder.", "lm_head."))}
        a, b = "shared.weight", "encoder.embed_tokens.weight"
        if a in sd or b in sd:
            sd[a] = sd[b] = sd.get(a, sd.get(b))
        if torch_dtype != "auto":
            want = torch.float32 if torch_dtype is None else torch_dtype
            done = {}
            sd = {k: done.setdefault(id(v), v.to(want) if v.is_floating_point() else v) for k, v in sd.items()}     # the tied pair stays one tensor
        with torch.device("meta"):
            model = cls(cfg)
        model.load_state_dict(sd, strict=True, assign=True)
        model.encoder.embed_tokens.weight = model.shared.weight
        model.eval()
        return model

    # ------------------------------------------------------------------ forward
    def bias_delta(self, S):
        """fp32 [H, 2S-1]: relative_attention_bias gathered through the delta -> bucket table, entry [h, j - i + S - 1]"""
        rel = self.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        key = (S, rel.device)
        if key not in self._dev_buckets:
            self._dev_buckets[key] = delta_buckets(S, self.config.relative_attention_num_buckets, self.config.relative_attention_max_distance).to(rel.device)
        return rel.detach().float()[self._dev_buckets[key]].t().contiguous()

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, return_dict=True, output_dtype=None, **unsupported):
        """input_ids int [B,S] (S <= 512), attention_mask None | [B,S] (nonzero = keep; every sample keeps a token) -> EncoderOutput whose
        last_hidden_state is [B,S,d_model] in output_dtype (default: the parameters' bfloat16, what the reference's module returns; torch.float32
        gives the final norm before its rounding).  Padded query rows are computed like any other, as upstream does."""
        extra = sorted(k for k, v in unsupported.items() if v is not None and v is not False)
        if extra:
            raise NotImplementedError(f"videogpa_amd.t5: forward arguments {extra} are not implemented")
        if input_ids is None or input_ids.dim() != 2 or input_ids.is_floating_point():
            raise ValueError("videogpa_amd.t5: input_ids must be an integer tensor [B,S]")
        B, S = input_ids.shape
        if S < 1 or S > MAX_TOKENS:
            raise RuntimeError(f"videogpa_amd.t5: {S} tokens; the attention kernel holds a whole key row on chip and takes 1 .. {MAX_TOKENS}")
        if attention_mask is not None and tuple(attention_mask.shape) != (B, S):
            raise ValueError(f"videogpa_amd.t5: attention_mask must be [B,S] = {(B, S)}, got {tuple(attention_mask.shape)}")
        table = self.shared.weight
        if table.dtype == torch.float16 or output_dtype == torch.float16:
            raise NotImplementedError("videogpa_amd.t5: fp16 is not implemented (bfloat16 parameters, bfloat16 or float32 output)")
        if not table.is_cuda:
            raise RuntimeError("videogpa_amd.t5 needs its parameters on the GPU (no CPU fallback)")
        if table.dtype != torch.bfloat16:
            raise NotImplementedError(f"videogpa_amd.t5: parameters are {table.dtype}; cast the module with .to(torch.bfloat16)")
        output_dtype = torch.bfloat16 if output_dtype is None else output_dtype
        if not input_ids.is_cuda and (int(input_ids.min()) < 0 or int(input_ids.max()) >= self.config.vocab_size):
            raise IndexError(f"videogpa_amd.t5: token ids outside [0, {self.config.vocab_size})")
        ids = input_ids.to(device=table.device, dtype=torch.int64).contiguous()
        mask = None if attention_mask is None else (attention_mask.to(table.device) != 0).to(torch.uint8).contiguous()
        bias = self.bias_delta(S)
        enc = self.encoder
        x, n = ops.t5_embed_rms(ids, table.detach(), enc.block[0].layer[0].layer_norm.w32(), self.config.layer_norm_epsilon)
        eps = self.config.layer_norm_epsilon
        for i, blk in enumerate(enc.block):
            att, ff = blk.layer[0], blk.layer[1]
            x, n = ops.t5_rms(x, ff.layer_norm.w32(), att.SelfAttention(n, bias, mask), eps)
            y = ff.DenseReluDense(n)
            if i + 1 < len(enc.block):
                x, n = ops.t5_rms(x, enc.block[i + 1].layer[0].layer_norm.w32(), y, eps)
            else:
                _, n = ops.t5_rms(x, enc.final_layer_norm.w32(), y, eps, n_dtype=output_dtype, keep_stream=False)
        return EncoderOutput(n) if return_dict else (n,)
