"""The VGGT aggregator's attention path on the HIP kernels (the scorer's front half shares the kernel family of the
denoiser -- QK-norm over head_dim 64, rotary embedding, full attention).  Mirrors the reference-held modules so that their
checkpoints load by name:

    Attention                vggt/layers/attention.py:20-72   (qkv, q_norm, k_norm, proj; forward(x, pos=None))
    RotaryPositionEmbedding2D vggt/layers/rope.py:60-188       (frequency 100; here it only carries the frequency -- the rotation is
                                                                fused into the QK-norm kernel, rope_mode 1)
    Block                    vggt/layers/block.py:30-108      (norm1, attn, ls1, norm2, mlp.fc1 / fc2, ls2; forward(x, pos=None))
    alternating_attention    vggt/models/aggregator.py:236-306 (frame attention on (B*S, P, C), global attention on (B, S*P, C))
    Aggregator               vggt/models/aggregator.py:25-258  (camera / register tokens, positions, aa_block_num x aa_order loop, list of concatenated
                                                                intermediates; state-dict names patch_embed.*, frame_blocks.N.*, global_blocks.N.*,
                                                                camera_token, register_token)

Unlike the CogVideoX attention (un-vendored diffusers), this code is IN the reference tree, so the kernels behind it are pinned
against reference outputs: tests/golden/vggt_attention.pt, tests/test_gpu_vggt.py.  The backbone is frozen in the reference's use
(metrics only): gradients flow to the input and to the Linear layers (torch autograd around the kernels); LayerNorm / LayerScale
parameters get none.  head_dim must be 64 and qk_norm on (what VGGT-1B's aggregator uses: dim 1024, 16 heads).

The aggregator's patch embedding is reference-held as well (forward only, bf16 GEMMs and attention around an fp32 residual stream; pinned on
tests/golden/vggt_dinov2*.pt, tests/test_gpu_dinov2.py):

    DinoVisionTransformer    vggt/layers/vision_transformer.py:42-331 (block_chunks=0, ffn_layer="mlp"; patch projection + class / register tokens +
                                                                position table in ONE launch, csrc/dino_embed.hip; blocks without QK-norm / RoPE:
                                                                stream_ln -> qkv -> attention -> proj -> stream_ln -> mlp -> stream_ln, csrc/dino_stream.hip)
    vit_small / vit_base / vit_large / vit_giant2             :341-397; Aggregator(patch_embed="dinov2_vit{s,b,l}14_reg" | "dinov2_vitg2_reg")
                                                                builds them as vggt/models/aggregator.py:143-182 does

The prediction heads are reference-held too and sit below the aggregator (fp32, forward only, csrc/vggt_heads.hip; pinned on
tests/golden/vggt_heads.pt, tests/test_gpu_vggt_heads.py):

    CameraHead               vggt/heads/camera_head.py:19-149 (trunk of head_dim-128 blocks without QK-norm on the small fp32 attention)
    DPTHead                  vggt/heads/dpt_head.py:21-484    (the head shared with Depth Anything 3, videogpa_amd/dpt.py: channels-last, every
                                                                convolution the fp32-MFMA implicit GEMM, the full-resolution end one fused launch;
                                                                this file adds the constructor's refusals and the chunking along S)
    VGGT                     vggt/models/vggt.py:17-96        (aggregator + camera / depth / point heads; no track head)"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._nn import _PackedCache, _forward_only, read_checkpoint
from .dpt import DPTBase
from .transformer import _f32


class RotaryPositionEmbedding2D(nn.Module):
    def __init__(self, frequency: float = 100.0, scaling_factor: float = 1.0):
        super().__init__()
        if scaling_factor != 1.0:
            raise NotImplementedError("scaling_factor != 1 is not used by VGGT")
        self.base_frequency = frequency

    def tables(self, pos, head_dim):
        """pos [B, N, 2] (identical for every batch row, as the aggregator builds it) -> (cos, sin) fp32 [N, head_dim]"""
        if pos.ndim == 3:
            if pos.shape[0] > 1 and not bool((pos == pos[:1]).all()):
                raise NotImplementedError("per-sample positions: the aggregator uses one grid for every frame")
            pos = pos[0]
        return ops.rope2d_tables(pos, head_dim, self.base_frequency)


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=True, proj_bias=True, attn_drop=0.0, proj_drop=0.0, norm_layer=nn.LayerNorm, qk_norm=False,
                 fused_attn=True, rope=None):
        super().__init__()
        if dim % num_heads or dim // num_heads != 64 or not qk_norm or attn_drop or proj_drop:
            raise NotImplementedError("the HIP attention path covers head_dim 64 with QK-norm and no dropout (VGGT's aggregator blocks)")
        self.num_heads, self.head_dim = num_heads, 64
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.q_norm, self.k_norm = norm_layer(64), norm_layer(64)
        self.proj = nn.Linear(dim, dim, bias=proj_bias)
        self.rope = rope

    def forward(self, x, pos=None):
        B, N, C = x.shape
        qkv = self.qkv(x)                                   # [B, N, 3, H, 64] in memory: the layout the fused kernel reads
        rope = self.rope.tables(pos, 64) if (self.rope is not None and pos is not None) else None
        o = ops.qknorm_attention(qkv.contiguous(), _f32(self.q_norm.weight), _f32(self.q_norm.bias), _f32(self.k_norm.weight), _f32(self.k_norm.bias),
                                 self.num_heads, text_len=0, rope=rope, eps=self.q_norm.eps, rope_mode=1)
        return self.proj(o)


class LayerScale(nn.Module):
    def __init__(self, dim, init_values=1e-5):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features, bias=True):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features, bias=bias)
        self.fc2 = nn.Linear(hidden_features, in_features, bias=bias)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))               # nn.GELU() = the erf form (the tanh kernel of the denoiser is a different function)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=True, proj_bias=True, ffn_bias=True, init_values=None, norm_layer=nn.LayerNorm,
                 qk_norm=False, fused_attn=True, rope=None, ln_eps=None):
        super().__init__()
        if not init_values:
            raise NotImplementedError("blocks without LayerScale are not used by VGGT's aggregator")
        if ln_eps is not None:      # Depth Anything 3's DINOv2 block (depth_anything_3/model/dinov2/layers/block.py:26-75) passes ln_eps = 1e-6
            base_norm = norm_layer
            norm_layer = lambda d: base_norm(d, eps=ln_eps)
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, proj_bias=proj_bias, qk_norm=qk_norm, rope=rope)
        self.ls1 = LayerScale(dim, init_values)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio), bias=ffn_bias)
        self.ls2 = LayerScale(dim, init_values)

    def forward(self, x, pos=None):
        B = x.shape[0]
        n1 = ops.ln_modulate(x, _f32(self.norm1.weight), _f32(self.norm1.bias), None, 0, self.norm1.eps)
        a = self.attn(n1, pos=pos)
        g1 = _f32(self.ls1.gamma)[None, None].expand(B, 2, -1).contiguous()      # LayerScale = the gate of the fused residual + LayerNorm kernel
        x, n2 = ops.residual_ln(x, a, g1, _f32(self.norm2.weight), _f32(self.norm2.bias), None, 0, self.norm2.eps)
        g2 = _f32(self.ls2.gamma)[None, None].expand(B, 2, -1).contiguous()
        return ops.gate_residual(x, self.mlp(n2), g2, 0)


def alternating_attention(tokens, frame_blocks, global_blocks, B, S, pos=None, aa_order=("frame", "global")):
    """The aggregator's loop (vggt/models/aggregator.py:236-306) over already embedded tokens [B*S, P, C]: for every depth, a frame
    block on (B*S, P, C) and a global block on (B, S*P, C); returns the per-depth concatenated intermediates [B, S, P, 2C]."""
    P, C = tokens.shape[1], tokens.shape[2]
    outs = []
    for fb, gb in zip(frame_blocks, global_blocks):
        inter = {}
        for kind in aa_order:
            if kind == "frame":
                tokens = fb(tokens.reshape(B * S, P, C), pos=None if pos is None else pos.reshape(B * S, P, 2))
            elif kind == "global":
                tokens = gb(tokens.reshape(B, S * P, C), pos=None if pos is None else pos.reshape(B, S * P, 2))
            else:
                raise ValueError(f"Unknown attention type: {kind}")
            inter[kind] = tokens.reshape(B, S, P, C)
        outs.append(torch.cat([inter["frame"], inter["global"]], dim=-1))
    return outs, tokens


class PositionGetter:
    """vggt/layers/rope.py:24-57: (y, x) grid coordinates of the patches, [batch, height * width, 2] integer, cached per grid size"""

    def __init__(self):
        self.position_cache = {}

    def __call__(self, batch_size, height, width, device):
        key = (height, width, str(device))
        if key not in self.position_cache:
            yy, xx = torch.meshgrid(torch.arange(height, device=device), torch.arange(width, device=device), indexing="ij")
            self.position_cache[key] = torch.stack([yy.reshape(-1), xx.reshape(-1)], dim=-1)
        return self.position_cache[key][None].expand(batch_size, -1, -1).clone()


class PatchEmbed(nn.Module):
    """vggt/layers/patch_embed.py:25-78 (the aggregator's patch_embed="conv" form): Conv2d with kernel = stride = patch, flattened row-major"""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        self.patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = nn.Identity()

    def forward(self, x):
        ph, pw = self.patch_size
        if x.shape[-2] % ph or x.shape[-1] % pw:
            raise AssertionError(f"input image size {tuple(x.shape[-2:])} is not a multiple of the patch size {self.patch_size}")
        return self.proj(x).flatten(2).transpose(1, 2)


def slice_expand_and_flatten(token_tensor, B, S):
    """vggt/models/aggregator.py:309-331: a (1, 2, X, C) special token -> (B*S, X, C): entry 0 for the first frame of every sequence, entry 1 for the
    other S - 1 frames"""
    first = token_tensor[:, 0:1].expand(B, 1, *token_tensor.shape[2:])
    rest = token_tensor[:, 1:2].expand(B, S - 1, *token_tensor.shape[2:])
    return torch.cat([first, rest], dim=1).reshape(B * S, *token_tensor.shape[2:])


# ---------------------------------------------------------------------------------------------------------------- DINOv2 patch embedding
class DinoAttention(nn.Module):
    """vggt/layers/attention.py:21-93 as DINOv2 builds it (MemEffAttention without xFormers = Attention): no QK-norm, no RoPE, head_dim 64.  The
    parameters only live here; DinoBlock runs them."""

    def __init__(self, dim, num_heads=8, qkv_bias=True, proj_bias=True):
        super().__init__()
        if dim % num_heads or dim // num_heads != 64:
            raise NotImplementedError("the HIP attention path covers head_dim 64 (every DINOv2 variant: 384/6, 768/12, 1024/16, 1536/24)")
        self.num_heads, self.head_dim, self.scale = num_heads, 64, 64 ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim, bias=proj_bias)


class DinoBlock(nn.Module):
    """vggt/layers/block.py:27-98 at DINOv2's settings (LayerScale on, LayerNorm eps 1e-6, erf-GELU Mlp), forward only.  The residual stream is fp32, as
    bf16 autocast keeps it upstream (ops.stream_ln: LayerNorm, and x + gamma * y with the LayerNorm behind it in one pass); the GEMMs and the head_dim-64
    flash attention (on the three strided views of the qkv GEMM's output) are bf16: stream_ln (norm1) -> qkv -> attention -> proj -> stream_ln (ls1.gamma,
    norm2) -> fc1, GELU, fc2 -> stream_ln (ls2.gamma).  head_dim**-0.5 * log2(e), which the attention kernel wants on q, is folded into the q rows of a cached bf16
    copy of qkv.weight / qkv.bias (one bf16 rounding, as ops.prescale_q costs): no permute, no prescale pass."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=True, proj_bias=True, ffn_bias=True, init_values=None, eps=1e-6, attn_class=DinoAttention):
        super().__init__()
        if not init_values:
            raise NotImplementedError("DINOv2 blocks without LayerScale are not used by VGGT's aggregator (init_values=1.0)")
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = attn_class(dim, num_heads=num_heads, qkv_bias=qkv_bias, proj_bias=proj_bias)     # a subclass with further parameters: videogpa_amd.da3
        self.ls1 = LayerScale(dim, init_values)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = Mlp(dim, int(dim * mlp_ratio), bias=ffn_bias)
        self.ls2 = LayerScale(dim, init_values)
        self._packed = _PackedCache()

    def _qkv(self):
        w, b = self.attn.qkv.weight, self.attn.qkv.bias

        def make():
            C = w.shape[1]
            f = torch.ones(3 * C, device=w.device, dtype=torch.float32)
            f[:C] = self.attn.scale * ops.LOG2E
            return (w.detach().float() * f[:, None]).to(torch.bfloat16).contiguous(), \
                (None if b is None else (b.detach().float() * f).to(torch.bfloat16).contiguous())
        return self._packed.get("qkv", [w] + ([] if b is None else [b]), make)

    def forward(self, x):
        """x fp32 [B,N,C] (the residual stream stays fp32, as bf16 autocast keeps it upstream) -> fp32 [B,N,C]"""
        B, N, C = x.shape
        H = self.attn.num_heads
        _, n1 = ops.stream_ln(x, None, None, _f32(self.norm1.weight), _f32(self.norm1.bias), self.norm1.eps)
        qkv = F.linear(n1, *self._qkv()).view(B, N, 3, H, 64)          # q already carries scale * log2(e)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))   # [B,H,N,64] views of the GEMM output, read in place
        o, _ = ops.attention_fwd_raw(q, k, v, scale=self.attn.scale, q_prescaled=True)
        a = self.attn.proj(o)
        x, n2 = ops.stream_ln(x, a.contiguous(), _f32(self.ls1.gamma), _f32(self.norm2.weight), _f32(self.norm2.bias), self.norm2.eps)
        return ops.stream_ln(x, self.mlp(n2).contiguous(), _f32(self.ls2.gamma))[0]


class DinoVisionTransformer(nn.Module):
    """vggt/layers/vision_transformer.py:42-331 on the HIP kernels: the reference's constructor arguments and, with block_chunks=0, its state-dict
    names (patch_embed.proj.*, cls_token, pos_embed, register_tokens, mask_token, blocks.N.*, norm.*), so the `aggregator.patch_embed.*` part of a
    VGGT checkpoint loads by name.  `forward(x [N,3,H,W], already normalised) -> {x_norm_clstoken, x_norm_regtokens, x_norm_patchtokens, x_prenorm,
    masks: None}` in fp32 (what bf16 autocast returns upstream).  Forward only; bf16 parameters, or fp32 parameters under bf16 autocast (the contract of the
    aggregator's blocks).  What the
    aggregator never builds raises: block_chunks > 0, ffn_layer other than "mlp", masks, list inputs, qk_norm, stochastic depth in training."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0, qkv_bias=True, ffn_bias=True,
                 proj_bias=True, drop_path_rate=0.0, drop_path_uniform=False, init_values=None, embed_layer=PatchEmbed, act_layer=nn.GELU,
                 block_fn=DinoBlock, ffn_layer="mlp", block_chunks=1, num_register_tokens=0, interpolate_antialias=False, interpolate_offset=0.1,
                 qk_norm=False):
        super().__init__()
        if block_chunks > 0:
            raise NotImplementedError("block_chunks > 0 (FSDP wrapping; renames the blocks): the aggregator builds block_chunks=0")
        if ffn_layer != "mlp":
            raise NotImplementedError(f"ffn_layer={ffn_layer!r}: the aggregator's DINOv2 uses 'mlp'")
        if qk_norm:
            raise NotImplementedError("qk_norm=True: DINOv2 has no QK-norm (the aggregator's own blocks do: vggt.Block)")
        if in_chans != 3 or act_layer is not nn.GELU or embed_layer is not PatchEmbed or isinstance(patch_size, (tuple, list)):
            raise NotImplementedError("DinoVisionTransformer on the HIP path: 3 input channels, square patches, PatchEmbed, nn.GELU")
        if embed_dim % num_heads or embed_dim // num_heads != 64:
            raise NotImplementedError("the HIP attention path covers head_dim 64")
        if num_register_tokens < 0:
            raise ValueError("num_register_tokens must be >= 0")
        self.num_features = self.embed_dim = embed_dim
        self.num_tokens, self.n_blocks, self.num_heads, self.patch_size = 1, depth, num_heads, patch_size
        self.num_register_tokens, self.interpolate_antialias, self.interpolate_offset = num_register_tokens, interpolate_antialias, interpolate_offset
        self.drop_path_rate, self.chunked_blocks = drop_path_rate, False
        self.patch_embed = embed_layer(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        grid = (img_size // patch_size, img_size // patch_size) if isinstance(img_size, int) else (img_size[0] // patch_size, img_size[1] // patch_size)
        num_patches = grid[0] * grid[1]
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + self.num_tokens, embed_dim))
        self.register_tokens = nn.Parameter(torch.zeros(1, num_register_tokens, embed_dim)) if num_register_tokens else None
        self.blocks = nn.ModuleList([block_fn(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, proj_bias=proj_bias,
                                              ffn_bias=ffn_bias, init_values=init_values) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        self.head = nn.Identity()
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))
        self._packed = _PackedCache()
        self.init_weights()

    def init_weights(self):
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        if self.register_tokens is not None:
            nn.init.normal_(self.register_tokens, std=1e-6)
        for m in self.modules():                                 # init_weights_vit_timm
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    # ---- position table: a function of the parameter and the grid only
    def _interpolated(self, w0, h0):
        """fp32 [1, 1 + w0 * h0, C]; `w0` counts patches along the image's FIRST spatial axis, as the reference names it (:180-212)"""
        pos = self.pos_embed.detach().float()
        N = pos.shape[1] - 1
        M = int(math.sqrt(N))
        assert N == M * M
        kwargs = {}
        if self.interpolate_offset:
            kwargs["scale_factor"] = (float(w0 + self.interpolate_offset) / M, float(h0 + self.interpolate_offset) / M)
        else:
            kwargs["size"] = (w0, h0)
        patch = F.interpolate(pos[:, 1:].reshape(1, M, M, -1).permute(0, 3, 1, 2), mode="bicubic", antialias=self.interpolate_antialias, **kwargs)
        assert (w0, h0) == tuple(patch.shape[-2:])
        return torch.cat((pos[:, :1], patch.permute(0, 2, 3, 1).reshape(1, w0 * h0, -1)), dim=1).contiguous()

    def pos_table(self, w, h):
        """interpolate_pos_encoding for an image of w x h pixels (first, second spatial axis): the parameter itself when the grid is the trained
        square one, else the bicubic resample in fp32, cached per (grid, device, pos_embed._version)"""
        w0, h0 = w // self.patch_size, h // self.patch_size
        if w0 * h0 == self.pos_embed.shape[1] - 1 and w == h:
            return self.pos_embed
        return self._packed.get(("pos", w0, h0), [self.pos_embed], lambda: self._interpolated(w0, h0))

    def interpolate_pos_encoding(self, x, w, h):
        assert x.shape[1] - 1 == (w // self.patch_size) * (h // self.patch_size)
        t = self.pos_table(w, h)
        return t if t is self.pos_embed else t.to(x.dtype)

    def _embed_params(self):
        pe = self.patch_embed.proj
        ps = [pe.weight, pe.bias, self.cls_token] + ([] if self.register_tokens is None else [self.register_tokens])
        return self._packed.get("embed", ps, lambda: (ops.pack_patch_weight(pe.weight), pe.bias.detach().float().contiguous(),
                                                      self.cls_token.detach().float().reshape(-1).contiguous(),
                                                      None if self.register_tokens is None else self.register_tokens.detach().float()[0].contiguous()))

    def prepare_tokens_with_masks(self, x, masks=None, out_dtype=torch.float32):
        """:214-226 in one launch (ops.dino_embed); x [N,3,w,h] fp32 | bf16 -> [N, 1 + R + P, C]"""
        if masks is not None:
            raise NotImplementedError("masks (iBOT training) are not used by VGGT")
        _forward_only(self, x)
        _, _, w, h = x.shape
        if w % self.patch_size or h % self.patch_size:
            raise AssertionError(f"input image size {(w, h)} is not a multiple of the patch size {self.patch_size}")
        pos = self.pos_table(w, h)
        if pos is self.pos_embed:
            pos = _f32(pos)
        wp, bias, cls, reg = self._embed_params()
        return ops.dino_embed(x.contiguous(), wp, bias, cls, reg, pos[0], out_dtype)

    def _tokens(self, x, masks=None):
        if isinstance(x, (list, tuple)):
            raise NotImplementedError("list inputs (nested tensors, xFormers) are not used by VGGT")
        if self.training and self.drop_path_rate > 0:
            raise NotImplementedError("stochastic depth (drop_path_rate > 0 in training mode): the backbone is forward only")
        if next(self.blocks.parameters()).dtype != torch.bfloat16 and not torch.is_autocast_enabled():
            raise RuntimeError("DinoVisionTransformer computes in bf16: bf16 parameters, or fp32 parameters under torch.autocast(dtype=torch.bfloat16)")
        return self.prepare_tokens_with_masks(x, masks)

    def _norm(self, x):
        return ops.stream_ln(x, None, None, _f32(self.norm.weight), _f32(self.norm.bias), self.norm.eps, n_dtype=torch.float32)[1]

    def forward_features(self, x, masks=None):
        x = self._tokens(x, masks)
        for blk in self.blocks:
            x = blk(x)
        x_norm, R = self._norm(x), self.num_register_tokens
        return {"x_norm_clstoken": x_norm[:, 0], "x_norm_regtokens": x_norm[:, 1:R + 1], "x_norm_patchtokens": x_norm[:, R + 1:], "x_prenorm": x,
                "masks": masks}

    def get_intermediate_layers(self, x, n=1, reshape=False, return_class_token=False, norm=True):
        t = self._tokens(x)
        take = range(len(self.blocks) - n, len(self.blocks)) if isinstance(n, int) else n
        outputs = []
        for i, blk in enumerate(self.blocks):
            t = blk(t)
            if i in take:
                outputs.append(t)
        assert len(outputs) == len(take), f"only {len(outputs)} / {len(take)} blocks found"
        if norm:
            outputs = [self._norm(o) for o in outputs]
        class_tokens = [o[:, 0] for o in outputs]
        outputs = [o[:, 1 + self.num_register_tokens:] for o in outputs]
        if reshape:
            B, _, w, h = x.shape
            outputs = [o.reshape(B, w // self.patch_size, h // self.patch_size, -1).permute(0, 3, 1, 2).contiguous() for o in outputs]
        return tuple(zip(outputs, class_tokens)) if return_class_token else tuple(outputs)

    def forward(self, *args, is_training=True, **kwargs):
        ret = self.forward_features(*args, **kwargs)
        return ret if is_training else self.head(ret["x_norm_clstoken"])


def vit_small(patch_size=16, num_register_tokens=0, **kwargs):
    return DinoVisionTransformer(patch_size=patch_size, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4, num_register_tokens=num_register_tokens, **kwargs)


def vit_base(patch_size=16, num_register_tokens=0, **kwargs):
    return DinoVisionTransformer(patch_size=patch_size, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, num_register_tokens=num_register_tokens, **kwargs)


def vit_large(patch_size=16, num_register_tokens=0, **kwargs):
    return DinoVisionTransformer(patch_size=patch_size, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, num_register_tokens=num_register_tokens, **kwargs)


def vit_giant2(patch_size=16, num_register_tokens=0, **kwargs):
    return DinoVisionTransformer(patch_size=patch_size, embed_dim=1536, depth=40, num_heads=24, mlp_ratio=4, num_register_tokens=num_register_tokens, **kwargs)


DINOV2_MODELS = {"dinov2_vitl14_reg": vit_large, "dinov2_vitb14_reg": vit_base, "dinov2_vits14_reg": vit_small, "dinov2_vitg2_reg": vit_giant2}


class Aggregator(nn.Module):
    """vggt/models/aggregator.py:25-258 on the HIP attention path: `forward(images [B, S, 3, H, W] in [0, 1]) -> (list of [B, S, P, 2C] per depth,
    patch_start_idx)`.  Constructor arguments, parameter names and the order of operations are the reference's, so an aggregator state dict loads with
    load_state_dict.  patch_embed: "conv" builds the reference's PatchEmbed; "dinov2_vitl14_reg" (the default), "dinov2_vitb14_reg",
    "dinov2_vits14_reg" and "dinov2_vitg2_reg" build the DinoVisionTransformer below with the reference's arguments (aggregator.py:147-178); a
    constructed module (anything mapping [B*S, 3, H, W] to patch tokens [B*S, N, C] or to a dict carrying "x_norm_patchtokens") is registered as
    it is under the same name `patch_embed`."""

    def __init__(self, img_size=518, patch_size=14, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4.0, num_register_tokens=4, block_fn=Block,
                 qkv_bias=True, proj_bias=True, ffn_bias=True, patch_embed="dinov2_vitl14_reg", aa_order=("frame", "global"), aa_block_size=1,
                 qk_norm=True, rope_freq=100, init_values=0.01):
        super().__init__()
        if isinstance(patch_embed, nn.Module):
            self.patch_embed = patch_embed
        elif "conv" in patch_embed:
            self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=3, embed_dim=embed_dim)
        else:
            if patch_embed not in DINOV2_MODELS:
                raise KeyError(f"patch_embed={patch_embed!r}: 'conv', one of {sorted(DINOV2_MODELS)}, or a module")
            self.patch_embed = DINOV2_MODELS[patch_embed](img_size=img_size, patch_size=patch_size, num_register_tokens=num_register_tokens,
                                                          interpolate_antialias=True, interpolate_offset=0.0, block_chunks=0, init_values=1.0)
            if self.patch_embed.embed_dim != embed_dim:
                raise ValueError(f"patch_embed={patch_embed!r} is {self.patch_embed.embed_dim} wide, the aggregator {embed_dim}")
            self.patch_embed.mask_token.requires_grad_(False)
        self.rope = RotaryPositionEmbedding2D(frequency=rope_freq) if rope_freq > 0 else None
        self.position_getter = PositionGetter() if self.rope is not None else None
        mk = lambda: block_fn(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, proj_bias=proj_bias, ffn_bias=ffn_bias,
                              init_values=init_values, qk_norm=qk_norm, rope=self.rope)
        self.frame_blocks = nn.ModuleList([mk() for _ in range(depth)])
        self.global_blocks = nn.ModuleList([mk() for _ in range(depth)])
        self.depth, self.aa_order, self.patch_size, self.aa_block_size = depth, list(aa_order), patch_size, aa_block_size
        if depth % aa_block_size != 0:
            raise ValueError(f"depth ({depth}) must be divisible by aa_block_size ({aa_block_size})")
        self.aa_block_num = depth // aa_block_size
        # two camera tokens and two sets of register tokens: one for the first frame, one for the rest
        self.camera_token = nn.Parameter(torch.randn(1, 2, 1, embed_dim))
        self.register_token = nn.Parameter(torch.randn(1, 2, num_register_tokens, embed_dim))
        self.patch_start_idx = 1 + num_register_tokens
        nn.init.normal_(self.camera_token, std=1e-6)
        nn.init.normal_(self.register_token, std=1e-6)
        self.register_buffer("_resnet_mean", torch.tensor([0.485, 0.456, 0.406]).view(1, 1, 3, 1, 1), persistent=False)
        self.register_buffer("_resnet_std", torch.tensor([0.229, 0.224, 0.225]).view(1, 1, 3, 1, 1), persistent=False)
        self.use_reentrant = False

    def _run(self, blocks, idx, tokens, pos):
        if self.training and torch.is_grad_enabled():      # the reference checkpoints every block in training mode (:268-271, :292-295)
            from torch.utils.checkpoint import checkpoint
            return checkpoint(blocks[idx], tokens, pos, use_reentrant=self.use_reentrant)
        return blocks[idx](tokens, pos=pos)

    def forward(self, images):
        B, S, C_in, H, W = images.shape
        if C_in != 3:
            raise ValueError(f"Expected 3 input channels, got {C_in}")
        images = ((images - self._resnet_mean) / self._resnet_std).reshape(B * S, C_in, H, W)
        patch_tokens = self.patch_embed(images.to(next(self.frame_blocks.parameters()).dtype))
        if isinstance(patch_tokens, dict):
            patch_tokens = patch_tokens["x_norm_patchtokens"]
        if isinstance(self.patch_embed, DinoVisionTransformer):
            patch_tokens = patch_tokens.to(torch.bfloat16)       # the backbone returns fp32 (its stream is fp32); the blocks below run a bf16 stream
        tokens = torch.cat([slice_expand_and_flatten(self.camera_token, B, S).to(patch_tokens.dtype),
                            slice_expand_and_flatten(self.register_token, B, S).to(patch_tokens.dtype), patch_tokens], dim=1)
        pos = None
        if self.rope is not None:
            pos = self.position_getter(B * S, H // self.patch_size, W // self.patch_size, device=images.device)
            if self.patch_start_idx > 0:      # special tokens sit at position 0, the patch grid starts at 1 (:215-224)
                pos = torch.cat([pos.new_zeros(B * S, self.patch_start_idx, 2), pos + 1], dim=1)
        _, P, C = tokens.shape
        tokens = tokens.contiguous()
        fi = gi = 0
        out = []
        for _ in range(self.aa_block_num):
            inter = {}
            for kind in self.aa_order:
                if kind not in ("frame", "global"):
                    raise ValueError(f"Unknown attention type: {kind}")
                shape = (B * S, P) if kind == "frame" else (B, S * P)
                tokens = tokens.reshape(*shape, C)
                pk = None if pos is None else pos.reshape(*shape, 2)
                got = []
                for _ in range(self.aa_block_size):
                    if kind == "frame":
                        tokens, fi = self._run(self.frame_blocks, fi, tokens, pk), fi + 1
                    else:
                        tokens, gi = self._run(self.global_blocks, gi, tokens, pk), gi + 1
                    got.append(tokens.reshape(B, S, P, C))
                inter[kind] = got
            out += [torch.cat([f, g], dim=-1) for f, g in zip(inter["frame"], inter["global"])]
        return out, self.patch_start_idx


# ---------------------------------------------------------------------------------------------------------------- prediction heads
class TrunkAttention(nn.Module):
    """vggt/layers/attention.py:21-72 as the camera trunk builds it: no QK-norm, no RoPE, any head_dim in multiples of 32, a few tokens (one per frame)"""

    def __init__(self, dim, num_heads=8, qkv_bias=True, proj_bias=True):
        super().__init__()
        if dim % num_heads or (dim // num_heads) % 32:
            raise NotImplementedError("the small fp32 attention covers head_dim in multiples of 32")
        self.num_heads, self.head_dim = num_heads, dim // num_heads
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim, bias=proj_bias)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, self.head_dim).contiguous()
        return self.proj(ops.attn_small_f32(qkv, self.head_dim ** -0.5))


class HeadMlp(nn.Module):
    """vggt/layers/mlp.py:16-40 with out_features"""

    def __init__(self, in_features, hidden_features=None, out_features=None, bias=True):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features, bias=bias)
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features, bias=bias)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class TrunkBlock(nn.Module):
    """vggt/layers/block.py:27-98 at the camera head's settings (LayerScale on, qk_norm off, no rope), fp32"""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, init_values=None):
        super().__init__()
        if not init_values:
            raise NotImplementedError("blocks without LayerScale are not used by VGGT's camera head")
        self.norm1 = nn.LayerNorm(dim)
        self.attn = TrunkAttention(dim, num_heads=num_heads)
        self.ls1 = LayerScale(dim, init_values)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = HeadMlp(dim, int(dim * mlp_ratio))
        self.ls2 = LayerScale(dim, init_values)

    def forward(self, x):
        x = x + self.attn(self.norm1(x)) * self.ls1.gamma
        return x + self.mlp(self.norm2(x)) * self.ls2.gamma


class CameraHead(nn.Module):
    """vggt/heads/camera_head.py:19-149: iterative refinement of the 9-number pose encoding from the camera tokens of the last aggregator
    output.  The Linear / LayerNorm layers are torch (a handful of tokens); the trunk's attention is ops.attn_small_f32.  fp32 whatever
    autocast says, forward only."""

    def __init__(self, dim_in=2048, trunk_depth=4, pose_encoding_type="absT_quaR_FoV", num_heads=16, mlp_ratio=4, init_values=0.01,
                 trans_act="linear", quat_act="linear", fl_act="relu"):
        super().__init__()
        if pose_encoding_type != "absT_quaR_FoV":
            raise ValueError(f"Unsupported camera encoding type: {pose_encoding_type}")
        self.target_dim = 9
        self.trans_act, self.quat_act, self.fl_act, self.trunk_depth = trans_act, quat_act, fl_act, trunk_depth
        self.trunk = nn.Sequential(*[TrunkBlock(dim=dim_in, num_heads=num_heads, mlp_ratio=mlp_ratio, init_values=init_values)
                                     for _ in range(trunk_depth)])
        self.token_norm = nn.LayerNorm(dim_in)
        self.trunk_norm = nn.LayerNorm(dim_in)
        self.empty_pose_tokens = nn.Parameter(torch.zeros(1, 1, self.target_dim))
        self.embed_pose = nn.Linear(self.target_dim, dim_in)
        self.poseLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(dim_in, 3 * dim_in, bias=True))
        self.adaln_norm = nn.LayerNorm(dim_in, elementwise_affine=False, eps=1e-6)
        self.pose_branch = HeadMlp(in_features=dim_in, hidden_features=dim_in // 2, out_features=self.target_dim)

    @staticmethod
    def _act(x, kind):
        if kind == "linear":
            return x
        if kind == "relu":
            return F.relu(x)
        if kind == "exp":
            return torch.exp(x)
        if kind == "inv_log":
            return torch.sign(x) * torch.expm1(torch.abs(x))
        raise ValueError(f"Unknown act_type: {kind}")

    def forward(self, aggregated_tokens_list, num_iterations=4):
        tokens = aggregated_tokens_list[-1]
        _forward_only(self, tokens)
        with torch.autocast(tokens.device.type, enabled=False):
            pose_tokens = self.token_norm(tokens[:, :, 0].float())
            B, S, C = pose_tokens.shape
            pred, out = None, []
            for _ in range(num_iterations):
                module_input = self.embed_pose(self.empty_pose_tokens.expand(B, S, -1) if pred is None else pred)
                shift, scale, gate = self.poseLN_modulation(module_input).chunk(3, dim=-1)
                x = gate * (self.adaln_norm(pose_tokens) * (1 + scale) + shift) + pose_tokens
                delta = self.pose_branch(self.trunk_norm(self.trunk(x)))
                pred = delta if pred is None else pred + delta
                out.append(torch.cat([self._act(pred[..., :3], self.trans_act), self._act(pred[..., 3:7], self.quat_act),
                                      self._act(pred[..., 7:], self.fl_act)], dim=-1))
        return out


class DPTHead(DPTBase):
    """vggt/heads/dpt_head.py:21-484 on the shared head of videogpa_amd/dpt.py (RELU_RESIDUAL and F32_ANGLES as defined there: VGGT's in-place
    ReLU, float64 embedding angles): `forward(aggregated_tokens_list, images [B,S,3,H,W], patch_start_idx, frames_chunk_size=8) ->
    (preds [B,S,H,W,output_dim-1], conf [B,S,H,W])`, per batch row in chunks of frames_chunk_size frames along S."""

    def __init__(self, dim_in, patch_size=14, output_dim=4, activation="inv_log", conf_activation="expp1", features=256,
                 out_channels=(256, 512, 1024, 1024), intermediate_layer_idx=(4, 11, 17, 23), pos_embed=True, feature_only=False, down_ratio=1):
        if feature_only or down_ratio != 1 or conf_activation != "expp1" or activation not in ("exp", "inv_log"):
            raise NotImplementedError("DPTHead on the HIP path: feature_only=False, down_ratio=1, conf_activation='expp1', activation 'exp' | 'inv_log'")
        super().__init__(dim_in, patch_size, output_dim, activation, conf_activation, features, out_channels, pos_embed, down_ratio)
        self.feature_only, self.intermediate_layer_idx = feature_only, list(intermediate_layer_idx)

    def forward(self, aggregated_tokens_list, images, patch_start_idx, frames_chunk_size=8):
        _forward_only(self, images, *[aggregated_tokens_list[i] for i in self.intermediate_layer_idx])
        B, S, _, H, W = images.shape
        with torch.autocast(images.device.type, enabled=False):
            if frames_chunk_size is None or frames_chunk_size >= S:
                return self._forward_impl(aggregated_tokens_list, (H, W), patch_start_idx, 0, S)
            assert frames_chunk_size > 0
            parts = [self._forward_impl(aggregated_tokens_list, (H, W), patch_start_idx, s0, min(s0 + frames_chunk_size, S))
                     for s0 in range(0, S, frames_chunk_size)]
            return torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts], dim=1)

    def _forward_impl(self, aggregated_tokens_list, hw, patch_start_idx, s0, s1):
        tokens = [aggregated_tokens_list[i][:, s0:s1, patch_start_idx:].float() for i in self.intermediate_layer_idx]
        B, S = tokens[0].shape[:2]
        preds, conf = self._main_tail(*self._pyramid([t.reshape(B * S, -1, t.shape[-1]) for t in tokens], *hw))
        return preds.view(B, S, *preds.shape[1:]), conf.view(B, S, *conf.shape[1:])


class VGGT(nn.Module):
    """vggt/models/vggt.py:17-96 without the track head: `forward(images [S,3,H,W] | [B,S,3,H,W] in [0,1]) -> {pose_enc, pose_enc_list, depth,
    depth_conf, world_points, world_points_conf, images (eval mode)}`.  The aggregator runs in whatever precision the caller set (bf16
    autocast in the scorer); the heads compute in fp32 as upstream (autocast off, :65).  `patch_embed` as the Aggregator takes it (default: the DINOv2
    ViT-L/14-reg built here, so VGGT() matches a VGGT-1B checkpoint; from_pretrained(dir) loads one from local files);
    aggregator_kwargs / camera_kwargs / dpt_kwargs reach the three constructors (reduced configurations; VGGT-1B needs none).  `track_head.*` keys of a reference checkpoint are dropped on load."""

    def __init__(self, img_size=518, patch_size=14, embed_dim=1024, enable_camera=True, enable_point=True, enable_depth=True, enable_track=False,
                 patch_embed="dinov2_vitl14_reg", aggregator_kwargs=None, camera_kwargs=None, dpt_kwargs=None):
        super().__init__()
        if enable_track:
            raise NotImplementedError("the track head is not built (the scorer never queries tracks)")
        self.aggregator = Aggregator(img_size=img_size, patch_size=patch_size, embed_dim=embed_dim, patch_embed=patch_embed, **(aggregator_kwargs or {}))
        ck, dk = camera_kwargs or {}, dpt_kwargs or {}
        self.camera_head = CameraHead(dim_in=2 * embed_dim, **ck) if enable_camera else None
        self.point_head = DPTHead(dim_in=2 * embed_dim, patch_size=patch_size, output_dim=4, activation="inv_log", conf_activation="expp1", **dk) \
            if enable_point else None
        self.depth_head = DPTHead(dim_in=2 * embed_dim, patch_size=patch_size, output_dim=2, activation="exp", conf_activation="expp1", **dk) \
            if enable_depth else None
        self.track_head = None

    def load_state_dict(self, state_dict, strict=True, **kw):
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("track_head.")}, strict=strict, **kw)

    @classmethod
    def from_pretrained(cls, path, **kwargs):
        """A VGGT checkpoint from the LOCAL file system (never the network): `path` is a directory holding model.safetensors or model.pt, or such a
        file; **kwargs reach the constructor (none for VGGT-1B).  `track_head.*` keys are dropped; everything else must match by name."""
        state = read_checkpoint(path)
        model = cls(**kwargs)
        model.load_state_dict(state, strict=True)
        return model.eval()

    def run_heads(self, aggregated_tokens_list, images, patch_start_idx):
        predictions = {}
        if self.camera_head is not None:
            pose_enc_list = self.camera_head(aggregated_tokens_list)
            predictions["pose_enc"], predictions["pose_enc_list"] = pose_enc_list[-1], pose_enc_list
        if self.depth_head is not None:
            predictions["depth"], predictions["depth_conf"] = self.depth_head(aggregated_tokens_list, images=images, patch_start_idx=patch_start_idx)
        if self.point_head is not None:
            predictions["world_points"], predictions["world_points_conf"] = self.point_head(aggregated_tokens_list, images=images,
                                                                                            patch_start_idx=patch_start_idx)
        return predictions

    def forward(self, images, query_points=None):
        if query_points is not None:
            raise NotImplementedError("query_points need the track head, which is not built")
        if images.ndim == 4:
            images = images.unsqueeze(0)
        aggregated_tokens_list, patch_start_idx = self.aggregator(images)
        predictions = self.run_heads(aggregated_tokens_list, images, patch_start_idx)
        if not self.training:
            predictions["images"] = images
        return predictions
