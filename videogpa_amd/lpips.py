"""LPIPS-VGG on the device: the drop-in for `lpips.LPIPS(net='vgg')` (lpips 0.1.x, lpips/lpips.py + pretrained_networks.py) that the reference builds
at train/01_preference_pair.py:102, replicate_scorer.py:64 and metrics/lpips.py:19.

    from videogpa_amd import lpips
    net = lpips.LPIPS(net='vgg', model_path=".../weights/v0.1/vgg.pth", vgg_path=".../vgg16-397923af.pth").cuda()
    d = net(gt, rep)                                    # [N,3,H,W] in [-1,1] -> [N,1,1,1]

Inference only, fp32, channels-last inside.  The thirteen 3x3 convolutions run on `ops.conv3x3_f32` (the exact-fp32 MFMA kernel of the VGGT heads, which
stores pre-ReLU outputs; the next convolution's `relu_in`, the pool and the layer kernel apply the ReLU), the rest on csrc/lpips.hip: the ScalingLayer
and the NCHW -> NHWC change, the 2 x 2 max pool, and one kernel per LPIPS layer (unit-normalise both maps, squared difference, `lin`, spatial mean).
Weights are LOCAL files only, nothing is ever fetched.  The parameter names below are restated from upstream lpips 0.1.x and torchvision's VGG16
(neither is a dependency), see DESIGN.md section 5d."""
import os

import torch
import torch.nn as nn

from . import ops
from ._nn import _PackedCache, read_state_file as _read

# torchvision `vgg16().features` indices of the convolutions of the five slices (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3) and their widths
SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
CHNS = (64, 128, 256, 512, 512)
LIN_FILE = "weights/v0.1/vgg.pth"
VGG_FILE = "vgg16-397923af.pth"


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(ops.LPIPS_SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(ops.LPIPS_SCALE)[None, :, None, None])


class NetLinLayer(nn.Module):
    """a 1x1 convolution without bias behind a Dropout, which is the identity here (inference only): the weight lives at `model.1.weight`"""

    def __init__(self, chn_in, chn_out=1, use_dropout=False):
        super().__init__()
        self.model = nn.Sequential(nn.Identity(), nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False))


class _VGG16Slices(nn.Module):
    """the parameters of torchvision's vgg16().features[:30], grouped and named as lpips.pretrained_networks.vgg16 does: slice{k}.{features index}"""

    def __init__(self):
        super().__init__()
        cin = 3
        for k, (idx, cout) in enumerate(zip(SLICES, CHNS)):
            s = nn.Module()
            for i in idx:
                s.add_module(str(i), nn.Conv2d(cin, cout, 3, padding=1))
                cin = cout
            self.add_module(f"slice{k + 1}", s)

    def convs(self):
        return [[getattr(getattr(self, f"slice{k + 1}"), str(i)) for i in idx] for k, idx in enumerate(SLICES)]


class LPIPS(nn.Module):
    def __init__(self, pretrained=True, net="vgg", version="0.1", lpips=True, spatial=False, pnet_rand=False, pnet_tune=False, use_dropout=True,
                 model_path=None, eval_mode=True, verbose=False, vgg_path=None, frames_chunk=8):
        """Upstream's keywords, plus `vgg_path` (torchvision's VGG16 state dict; `model_path` is upstream's lin-layer file, as there) and `frames_chunk` (pairs per pass through the stack; the result does not depend on it).
        pretrained=True needs both files.  pretrained=False gives seeded random lin layers, on a seeded random backbone with pnet_rand=True (tests,
        benchmarks: no file at all) and on the backbone of `vgg_path` otherwise, as upstream."""
        super().__init__()
        if net not in ("vgg", "vgg16"):
            raise NotImplementedError(f"net={net!r}: only the VGG16 variant ('vgg' / 'vgg16') runs on the device")
        if str(version) != "0.1":
            raise NotImplementedError(f"version={version!r}: only version '0.1' (with the ScalingLayer) is implemented")
        if not lpips:
            raise NotImplementedError("lpips=False (unweighted feature distance) is not implemented")
        if spatial:
            raise NotImplementedError("spatial=True (per-pixel distance maps) is not implemented")
        if pnet_tune:
            raise NotImplementedError("pnet_tune=True: the device path is inference only")
        if int(frames_chunk) < 1:
            raise ValueError("frames_chunk must be at least 1")
        self.pnet_type, self.version, self.frames_chunk = "vgg", "0.1", int(frames_chunk)
        self.chns, self.L = list(CHNS), len(CHNS)
        self.scaling_layer = ScalingLayer()
        self.net = _VGG16Slices()
        for k, c in enumerate(CHNS):
            self.add_module(f"lin{k}", NetLinLayer(c, use_dropout=use_dropout))
        self.lins = nn.ModuleList([getattr(self, f"lin{k}") for k in range(self.L)])
        self._packed = _PackedCache()
        if pretrained:
            if model_path is None or vgg_path is None:
                raise RuntimeError(
                    f"LPIPS(pretrained=True) needs two local files and never downloads: model_path = upstream lpips' {LIN_FILE} (the lin layers) and "
                    f"vgg_path = torchvision's VGG16 state dict ({VGG_FILE}).  LPIPS.from_pretrained(dir) finds both in one directory; "
                    "LPIPS(pretrained=False, pnet_rand=True) is a seeded random network to load_state_dict into")
            self.load_state_dict(_read(vgg_path))
            self.load_state_dict(_read(model_path))
        else:
            self._seeded_init()
            if not pnet_rand:
                if vgg_path is None:
                    raise RuntimeError(f"LPIPS(pretrained=False, pnet_rand=False) keeps the trained backbone and never downloads it: pass vgg_path = "
                                       f"torchvision's VGG16 state dict ({VGG_FILE}), or pnet_rand=True for a seeded random one")
                self.load_state_dict(_read(vgg_path))
        self.requires_grad_(False)
        if eval_mode:
            self.eval()

    def _seeded_init(self, seed=0):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for convs in self.net.convs():
                for c in convs:
                    c.weight.copy_(torch.randn(c.weight.shape, generator=g) * (2.0 / (9 * c.in_channels)) ** 0.5)
                    c.bias.copy_(0.1 * torch.randn(c.bias.shape, generator=g))
            for lin in self.lins:
                lin.model[1].weight.copy_(0.01 * torch.rand(lin.model[1].weight.shape, generator=g))

    @classmethod
    def from_pretrained(cls, path, **kw):
        """Both files from one LOCAL directory: the lin layers (`vgg.pth` / `vgg.safetensors`, also under weights/v0.1/) and torchvision's VGG16
        (`vgg16*.pth` / `vgg16*.safetensors`)."""
        exts = (".pth", ".safetensors")
        lin = [os.path.join(path, d, "vgg" + e) for d in ("", os.path.dirname(LIN_FILE)) for e in exts]
        lin = [f for f in lin if os.path.isfile(f)]
        vgg = sorted(os.path.join(path, f) for f in os.listdir(path) if f.startswith("vgg16") and f.endswith(exts))
        if not lin or not vgg:
            raise FileNotFoundError(f"{path}: needs vgg.pth (upstream lpips' {LIN_FILE}) and vgg16*.pth (torchvision's {VGG_FILE}), as .pth or "
                                    ".safetensors; from_pretrained reads local files only")
        return cls(pretrained=True, model_path=lin[0], vgg_path=vgg[0], **kw)

    # ---- state dicts: upstream's full module form, or its two files (lin-only .pth; torchvision `features.{i}.*`, `classifier.*` ignored) ----
    def load_state_dict(self, state_dict, strict=True, assign=False):
        slice_of = {i: k + 1 for k, idx in enumerate(SLICES) for i in idx}
        sd = {}
        for key, v in state_dict.items():
            parts = key.split(".")
            if parts[0] == "classifier":
                continue
            if parts[0] == "features" and len(parts) == 3 and parts[1].isdigit() and int(parts[1]) in slice_of:
                key = f"net.slice{slice_of[int(parts[1])]}.{parts[1]}.{parts[2]}"
            sd[key] = v
        for k in range(self.L):                                     # `lin{k}` and `lins.{k}` are one module under two names
            a, b = f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight"
            if a in sd and b not in sd:
                sd[b] = sd[a]
            elif b in sd and a not in sd:
                sd[a] = sd[b]
        own = self.state_dict()
        families = {"net.": [k for k in own if k.startswith("net.")], "lin": [k for k in own if k.startswith("lin")],
                    "scaling_layer.": [k for k in own if k.startswith("scaling_layer.")]}
        if not any(k in sd for k in own):
            raise RuntimeError("LPIPS.load_state_dict: none of the keys is one of upstream lpips' (net.slice*, lin*, lins.*, scaling_layer.*) "
                               "or torchvision VGG16's (features.*)")
        for keys in families.values():                               # a file that holds one family only (the two-file form) leaves the others as they are
            if not any(k in sd for k in keys):
                sd.update({k: own[k] for k in keys})
        return super().load_state_dict(sd, strict=strict, assign=assign)

    # ---- kernel-layout copies --------------------------------------------------------------------------------------------------------------
    def packed(self):
        """([[(w [3,3,Cin,Cout], bias)] per slice], [lin weight [C]] per layer, (shift, scale)) in the kernels' layout, fp32, rebuilt when a parameter
        changes (load_state_dict) or moves (.to()); conv1_1 is padded to 16 input channels with zero rows"""
        convs = self.net.convs()
        params = [p for cs in convs for c in cs for p in (c.weight, c.bias)] + [l.model[1].weight for l in self.lins] + \
            [self.scaling_layer.shift, self.scaling_layer.scale]

        def make():
            out = []
            for cs in convs:
                row = []
                for c in cs:
                    w = ops.pack_conv_weight(c.weight)
                    if w.shape[2] == 3:
                        w = torch.cat([w, w.new_zeros(3, 3, 13, w.shape[3])], dim=2).contiguous()
                    row.append((w, c.bias.detach().float().contiguous()))
                out.append(row)
            lins = [l.model[1].weight.detach().float().reshape(-1).contiguous() for l in self.lins]
            aff = (tuple(self.scaling_layer.shift.detach().float().reshape(-1).tolist()), tuple(self.scaling_layer.scale.detach().float().reshape(-1).tolist()))
            return out, lins, aff
        return self._packed.get("all", params, make)

    # ---- forward ---------------------------------------------------------------------------------------------------------------------------
    def _check(self, *xs):
        for x in xs:
            if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
                raise ValueError(f"LPIPS: inputs are fp32 [N,3,H,W] tensors, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}"
                                 f"{' ' + str(x.dtype) if isinstance(x, torch.Tensor) else ''}")
            if x.shape != xs[0].shape:
                raise ValueError(f"LPIPS: the two inputs differ in shape: {tuple(xs[0].shape)} vs {tuple(x.shape)}")
            if x.shape[0] < 1 or min(x.shape[-2:]) < 16:
                raise ValueError(f"LPIPS: needs at least one frame of 16 x 16 pixels (four 2 x 2 pools), got {tuple(x.shape)}")
        for x in xs:
            if not x.is_cuda:
                raise RuntimeError("videogpa_amd.lpips.LPIPS runs on the GPU only (no CPU fallback)")
            if torch.is_grad_enabled() and x.requires_grad:
                raise RuntimeError("LPIPS on the device is forward only: call it under torch.no_grad()")
        if not self.lins[0].model[1].weight.is_cuda:
            raise RuntimeError("LPIPS: the module's weights are not on the GPU (no CPU fallback): call .cuda() first")

    def _stack(self, x16, convs, tap):
        """x16 [n,H,W,16] through the five slices; tap(k, pre-ReLU feature map) after each"""
        h = x16
        for k, row in enumerate(convs):
            for j, (w, b) in enumerate(row):
                h = ops.conv3x3_f32(h, w, b, relu_in=j > 0)          # a slice's first input is the scaled image or a pool's output: ReLU already applied
            tap(k, h)
            if k + 1 < len(convs):
                h = ops.maxpool2x2_f32(h, relu=True)

    def features(self, x, normalize=False):
        """the five taps (relu1_2 ... relu5_3 BEFORE their ReLU) of x [N,3,H,W] as NHWC tensors"""
        self._check(x)
        convs, _, (shift, scale) = self.packed()
        taps = []
        with torch.no_grad():
            self._stack(ops.lpips_input_f32(x.contiguous(), shift, scale, normalize), convs, lambda k, h: taps.append(h))
        return taps

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        self._check(in0, in1)
        convs, lins, (shift, scale) = self.packed()
        N, _, H, W = in0.shape
        in0, in1 = in0.contiguous(), in1.contiguous()
        layers = torch.empty(self.L, N, device=in0.device, dtype=torch.float32)
        total = torch.empty(N, device=in0.device, dtype=torch.float64)
        with torch.no_grad():
            for s in range(0, N, self.frames_chunk):
                n = min(self.frames_chunk, N - s)
                x16 = torch.empty(2 * n, H, W, 16, device=in0.device, dtype=torch.float32)
                ops.lpips_input_f32(in0[s:s + n], shift, scale, normalize, out=x16[:n])
                ops.lpips_input_f32(in1[s:s + n], shift, scale, normalize, out=x16[n:])

                def tap(k, h):
                    ops.lpips_layer_f32(h[:n], h[n:], lins[k], relu=True, total=total[s:s + n], accumulate=k > 0, out=layers[k, s:s + n])
                self._stack(x16, convs, tap)
            val = total.float().view(N, 1, 1, 1)                       # the five layers were added in layer order in fp64: one rounding
        if retPerLayer:
            return val, [layers[k].view(N, 1, 1, 1) for k in range(self.L)]
        return val
