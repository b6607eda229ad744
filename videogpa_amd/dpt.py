"""The dense-prediction head that VGGT and Depth Anything 3 share, on the HIP kernels: what vggt.DPTHead (vggt/heads/dpt_head.py:21-484) and
da3.DualDPT (depth_anything_3/model/dualdpt.py:30-364, model/dpt.py) are both made of.  Channels-last from the tokens to the predictions, fp32
whatever autocast says, forward only.  The modules only hold the parameters under the references' names and shapes (a reference state dict loads by
name); the arithmetic is

    pyramid   LayerNorm (torch) -> projects.N, resize_layers.{0,1} as 1x1 convolutions (+ pixel shuffle) -> resize_layers.3 / layerN_rn as
              ops.conv3x3_f32
    chain     refinenet4..1: ResidualConvUnits as ops.conv3x3_f32 with ReLU, bias and residual adds fused -> out_conv BEFORE the bilinear
              upsample (both linear, the interpolation weights sum to 1: a quarter of the pixels)
    main_tail the chain, output_conv1 -> ops.dpt_tail_f32: the full-resolution end of the head (upsample, embedding, output_conv2, activations) in one launch

The two heads differ in two class attributes, RELU_RESIDUAL and F32_ANGLES (below), in how they chunk the frames, and in DualDPT's auxiliary branch."""
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._nn import _PackedCache


class _ResidualConvUnit(nn.Module):
    def __init__(self, features):
        super().__init__()
        self.conv1 = nn.Conv2d(features, features, kernel_size=3, stride=1, padding=1, bias=True)
        self.conv2 = nn.Conv2d(features, features, kernel_size=3, stride=1, padding=1, bias=True)


class _FeatureFusionBlock(nn.Module):
    def __init__(self, features, has_residual=True):
        super().__init__()
        self.out_conv = nn.Conv2d(features, features, kernel_size=1, stride=1, padding=0, bias=True)
        if has_residual:
            self.resConfUnit1 = _ResidualConvUnit(features)
        self.has_residual = has_residual
        self.resConfUnit2 = _ResidualConvUnit(features)


class DPTBase(nn.Module):
    """`norm`, `projects`, `resize_layers`, `scratch.layer{1..4}_rn`, one `scratch.refinenet{1..4}<suffix>` fusion chain per entry of `chains`,
    `scratch.output_conv1` and `scratch.output_conv2`, registered in that order, and the forward pieces that run them."""

    # What a ResidualConvUnit adds back.  VGGT's ReLU is in place upstream, so the tensor added back is relu(x), not x (dpt_head.py:366-386): True.
    # Depth Anything 3's is not in place: the residual is x itself, and the four `rn` maps feed both fusion chains unchanged: False.
    RELU_RESIDUAL = True
    # The UV embedding's angles: float64 as VGGT computes them (vggt/heads/utils.py:11-109), or Depth Anything 3's float32 recipe
    # (model/utils/head_utils.py:123-146).
    F32_ANGLES = False

    def __init__(self, dim_in, patch_size, output_dim, activation, conf_activation, features, out_channels, pos_embed, down_ratio, chains=("",)):
        super().__init__()
        out_channels = list(out_channels)
        if dim_in % 16 or features % 32 or len(out_channels) != 4 or any(c % 16 for c in out_channels) or not 2 <= output_dim <= 8:
            raise NotImplementedError(f"{type(self).__name__} on the HIP path: four stages, dim_in and out_channels in multiples of 16, features in "
                                      "multiples of 32, output_dim from 2 to 8 (what ops.dpt_tail_f32 takes)")
        self.patch_size, self.activation, self.conf_activation, self.pos_embed, self.down_ratio = patch_size, activation, conf_activation, pos_embed, down_ratio
        self.norm = nn.LayerNorm(dim_in)
        self.projects = nn.ModuleList([nn.Conv2d(dim_in, oc, kernel_size=1, stride=1, padding=0) for oc in out_channels])
        self.resize_layers = nn.ModuleList([
            nn.ConvTranspose2d(out_channels[0], out_channels[0], kernel_size=4, stride=4, padding=0),
            nn.ConvTranspose2d(out_channels[1], out_channels[1], kernel_size=2, stride=2, padding=0),
            nn.Identity(),
            nn.Conv2d(out_channels[3], out_channels[3], kernel_size=3, stride=2, padding=1)])
        sc = self.scratch = nn.Module()
        for i, c in enumerate(out_channels):
            setattr(sc, f"layer{i + 1}_rn", nn.Conv2d(c, features, kernel_size=3, stride=1, padding=1, bias=False))
        for suffix in chains:
            for k in (1, 2, 3, 4):
                setattr(sc, f"refinenet{k}{suffix}", _FeatureFusionBlock(features, has_residual=k != 4))
        sc.output_conv1 = nn.Conv2d(features, features // 2, kernel_size=3, stride=1, padding=1)
        sc.output_conv2 = nn.Sequential(nn.Conv2d(features // 2, 32, kernel_size=3, stride=1, padding=1), nn.ReLU(inplace=True),
                                        nn.Conv2d(32, output_dim, kernel_size=1, stride=1, padding=0))
        self._packed = _PackedCache()
        self._tabs = {}

    # ---- kernel-layout parameters
    def _conv(self, name, conv):
        """-> (weight [kh][kw][Cin][Cout] (a 1x1 as [Cin][Cout]), bias fp32 | None)"""
        def make():
            w = ops.pack_conv_weight(conv.weight)
            return (w[0, 0].contiguous() if w.shape[0] == 1 else w), (None if conv.bias is None else conv.bias.detach().float().contiguous())
        return self._packed.get(name, [conv.weight] + ([] if conv.bias is None else [conv.bias]), make)

    def _deconv(self, name, conv):
        """ConvTranspose2d with kernel = stride k: weight [Cin, Cout, k, k] -> [Cin][(a, b, Cout)], the bias repeated per (a, b)"""
        def make():
            k = conv.kernel_size[0]
            w = conv.weight.detach().float().permute(0, 2, 3, 1).reshape(conv.in_channels, k * k * conv.out_channels).contiguous()
            return w, conv.bias.detach().float().repeat(k * k).contiguous()
        return self._packed.get(name, [conv.weight, conv.bias], make)

    def _vec(self, name, *params):
        """small parameters as fp32 contiguous tensors (the 1x1 weights as [od, 32])"""
        return self._packed.get(name, list(params), lambda: tuple(p.detach().float().reshape(-1, 32).contiguous() if p.ndim == 4 else
                                                                  p.detach().float().contiguous() for p in params))

    def _embed(self, width, height, channels, aspect, device):
        key = (width, height, channels, aspect, str(device))
        if key not in self._tabs:
            if len(self._tabs) > 64:
                self._tabs.clear()
            self._tabs[key] = ops.uv_embed_tables(width, height, channels, aspect, device, f32_angles=self.F32_ANGLES)
        return self._tabs[key]

    # ---- forward pieces
    def _pyramid(self, tokens, H, W):
        """four [n, P, dim_in] token slices of H x W frames -> (the four `rn` maps [n, 4ph | 2ph | ph | ph/2, .., features], ph, pw, W / H)"""
        ph, pw, aspect = H // self.patch_size, W // self.patch_size, W / H
        rn = []
        for i, x in enumerate(tokens):
            n = x.shape[0]
            x = F.layer_norm(x.float(), self.norm.normalized_shape, self.norm.weight.float(), self.norm.bias.float(), self.norm.eps).contiguous()
            x = ops.conv1x1_f32(x, *self._conv(f"projects.{i}", self.projects[i])).reshape(n, ph, pw, self.projects[i].out_channels)
            if self.pos_embed:
                x = ops.upsample_bilinear_ac_f32(x, ph, pw, self._embed(pw, ph, x.shape[-1], aspect, x.device))
            layer = self.resize_layers[i]
            if isinstance(layer, nn.ConvTranspose2d):
                k, oc = layer.kernel_size[0], layer.out_channels
                x = ops.conv1x1_f32(x, *self._deconv(f"resize_layers.{i}", layer)).reshape(n, ph, pw, k, k, oc)
                x = x.permute(0, 1, 3, 2, 4, 5).reshape(n, ph * k, pw * k, oc).contiguous()
            elif isinstance(layer, nn.Conv2d):
                x = ops.conv3x3_f32(x, *self._conv(f"resize_layers.{i}", layer), stride=2)
            rn.append(x)
        return [ops.conv3x3_f32(x, self._conv(f"layer{i + 1}_rn", getattr(self.scratch, f"layer{i + 1}_rn"))[0]) for i, x in enumerate(rn)], ph, pw, aspect

    def _rcu(self, name, unit, x, extra=None):
        """conv2(relu(conv1(relu(x)))) + (relu(x) | x, see RELU_RESIDUAL) (+ extra): two launches; x is left as it is"""
        w1, b1 = self._conv(name + ".conv1", unit.conv1)
        w2, b2 = self._conv(name + ".conv2", unit.conv2)
        t = ops.conv3x3_f32(x, w1, b1, relu_in=True)
        return ops.conv3x3_f32(t, w2, b2, res=x, res2=extra, relu_in=True, relu_res=self.RELU_RESIDUAL)

    def _fuse(self, name, x0, x1, size):
        block = getattr(self.scratch, name)
        out = self._rcu(name + ".resConfUnit1", block.resConfUnit1, x1, extra=x0) if block.has_residual else x0
        out = self._rcu(name + ".resConfUnit2", block.resConfUnit2, out)
        out = ops.conv1x1_f32(out, *self._conv(name + ".out_conv", block.out_conv))
        return ops.upsample_bilinear_ac_f32(out, size[0], size[1])

    def _chain(self, rn, suffix=""):
        """refinenet4..1<suffix> on the four rn maps; refinenet1 upsamples by scale_factor=2"""
        out = self._fuse("refinenet4" + suffix, rn[3], None, rn[2].shape[1:3])
        out = self._fuse("refinenet3" + suffix, out, rn[2], rn[1].shape[1:3])
        out = self._fuse("refinenet2" + suffix, out, rn[1], rn[0].shape[1:3])
        return self._fuse("refinenet1" + suffix, out, rn[0], (2 * rn[0].shape[1], 2 * rn[0].shape[2]))

    def _main_tail(self, rn, ph, pw, aspect):
        """refinenet4..1 and output_conv1 at the fused resolution, then upsample to (patch_size ph, patch_size pw) + embedding + output_conv2 +
        activations in one launch -> (preds [n,Ho,Wo,output_dim-1], conf [n,Ho,Wo]).  Empties the list `rn` once the chain has read it, so that the
        four maps are gone before output_conv1 unless the caller holds them in a list of its own."""
        sc = self.scratch
        fused = self._chain(rn)
        rn.clear()
        out = ops.conv3x3_f32(fused, *self._conv("output_conv1", sc.output_conv1))
        del fused
        Ho, Wo = ph * self.patch_size, pw * self.patch_size
        w1, b1 = self._conv("output_conv2.0", sc.output_conv2[0])
        w2, b2 = self._vec("output_conv2.2", sc.output_conv2[2].weight, sc.output_conv2[2].bias)
        tabs = self._embed(Wo, Ho, out.shape[-1], aspect, out.device) if self.pos_embed else None
        return ops.dpt_tail_f32(out, Ho, Wo, w1, b1, w2, b2, activation=self.activation, tabs=tabs)
