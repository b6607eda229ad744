"""SuperPoint on the device: the drop-in for `lightglue.SuperPoint` (cvg/LightGlue: lightglue/superpoint.py, with `Extractor.extract` of
lightglue/utils.py) that the reference's LightGlueMatcher builds at metrics/epipolar.py:84.

    from videogpa_amd.superpoint import SuperPoint
    net = SuperPoint.from_pretrained(".../weights", max_num_keypoints=2048).cuda()
    feats = net.extract(image)                          # [1|3,H,W] or [B,1|3,H,W] in [0,1] -> keypoints, keypoint_scores, descriptors, image_size
    feats = net.extract_clip(frames_u8)                 # [T,H,W,3] uint8 -> T such dicts, every frame extracted once

Inference only, fp32, channels-last inside.  Nine of the ten 3x3 convolutions run on `ops.conv3x3_f32` (the exact-fp32 MFMA kernel of the VGGT heads,
which stores pre-ReLU outputs; the next convolution's `relu_in` and the pool apply the ReLU), the 1x1 descriptor head on the same kernel's 1x1 form,
the rest on csrc/superpoint.hip: the input stage with conv1a, the detector head, simple_nms, the selection and the descriptor sampling.
Weights are LOCAL files only, nothing is ever fetched.

Restated from memory and NOT pinned (neither lightglue nor kornia nor cv2 is a dependency): upstream's parameter names, its
defaults, `side_to_image_size` below and the gray weights of csrc/superpoint.hip."""
import os

import torch
import torch.nn as nn

from . import ops
from ._nn import _PackedCache, read_state_file as _read

# (name, Cin, Cout, kernel) in forward order; a 2 x 2 pool follows conv1b, conv2b and conv3b
LAYERS = (("conv1a", 1, 64, 3), ("conv1b", 64, 64, 3), ("conv2a", 64, 64, 3), ("conv2b", 64, 64, 3), ("conv3a", 64, 128, 3), ("conv3b", 128, 128, 3),
          ("conv4a", 128, 128, 3), ("conv4b", 128, 128, 3), ("convPa", 128, 256, 3), ("convPb", 256, 65, 1), ("convDa", 128, 256, 3),
          ("convDb", 256, 256, 1))
WEIGHT_FILES = ("superpoint_v1.pth", "superpoint_v1.safetensors")
DEFAULT_CONF = {"descriptor_dim": 256, "nms_radius": 4, "max_num_keypoints": None, "detection_threshold": 0.0005, "remove_borders": 4}
DEFAULT_PREPROCESS = {"resize": 1024, "side": "long"}


def side_to_image_size(size, side_size, side="long"):
    """kornia's `side_to_image_size` restated from memory (UNPINNED): (h, w) with the chosen side brought to `side_size`, the other one truncated,
    int(side_size / aspect): 480 x 720 at 1024 is 682 x 1024.  Pure Python, the only place this arithmetic lives."""
    h, w = int(size[0]), int(size[1])
    if side not in ("short", "long", "vert", "horz"):
        raise ValueError(f"side={side!r}")
    aspect = w / h
    if side == "vert" or (side in ("short", "long") and ((side == "short") ^ (aspect < 1.0))):
        return side_size, int(side_size * aspect)
    return int(side_size / aspect), side_size


class SuperPoint(nn.Module):
    def __init__(self, pretrained=True, weights_path=None, frames_chunk=4, preprocess_conf=None, **conf):
        """Upstream's configuration keywords (descriptor_dim, nms_radius, max_num_keypoints, detection_threshold, remove_borders, preprocess_conf), plus
        `weights_path` (upstream's superpoint_v1.pth, a local file) and `frames_chunk` (frames per pass through the stack in extract_clip; the result
        does not depend on it).  pretrained=False is a seeded random network (tests, benchmarks: no file at all)."""
        super().__init__()
        unknown = set(conf) - set(DEFAULT_CONF)
        if unknown:
            raise TypeError(f"SuperPoint: unknown configuration {sorted(unknown)}")
        self.conf = {**DEFAULT_CONF, **conf}
        self.preprocess_conf = {**DEFAULT_PREPROCESS, **(preprocess_conf or {})}
        if self.conf["descriptor_dim"] != 256:
            raise NotImplementedError("descriptor_dim: only upstream's 256 is implemented")
        if not 1 <= int(self.conf["nms_radius"]) <= 4:
            raise NotImplementedError("nms_radius: 1..4 (the tile of the device kernel carries a halo of five radii)")
        k = self.conf["max_num_keypoints"]
        if k is not None and not 1 <= int(k) <= ops.SP_MAX_CUT:
            raise NotImplementedError(f"max_num_keypoints: None or 1..{ops.SP_MAX_CUT}")
        if int(frames_chunk) < 1:
            raise ValueError("frames_chunk must be at least 1")
        self.frames_chunk = int(frames_chunk)
        for name, cin, cout, ks in LAYERS:
            self.add_module(name, nn.Conv2d(cin, cout, ks, stride=1, padding=ks // 2))
        self._packed = _PackedCache()
        if pretrained:
            if weights_path is None:
                raise RuntimeError(f"SuperPoint(pretrained=True) needs a local weight file and never downloads: weights_path = upstream's {WEIGHT_FILES[0]} "
                                   "(SuperPoint.from_pretrained(dir) finds it in a directory); SuperPoint(pretrained=False) is a seeded random network")
            self.load_state_dict(_read(weights_path))
        else:
            self._seeded_init()
        self.requires_grad_(False)
        self.eval()

    def _seeded_init(self, seed=0):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, cin, _, ks in LAYERS:
                c = getattr(self, name)
                c.weight.copy_(torch.randn(c.weight.shape, generator=g) * (2.0 / (ks * ks * cin)) ** 0.5)
                c.bias.copy_(0.1 * torch.randn(c.bias.shape, generator=g))

    @classmethod
    def from_pretrained(cls, path, **kw):
        """superpoint_v1.pth / superpoint_v1.safetensors from one LOCAL directory (or that file itself)"""
        path = os.fspath(path)
        if os.path.isdir(path):
            found = [os.path.join(path, f) for f in WEIGHT_FILES if os.path.isfile(os.path.join(path, f))]
            if not found:
                raise FileNotFoundError(f"{path}: needs {' or '.join(WEIGHT_FILES)}; from_pretrained reads local files only")
            path = found[0]
        elif not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: no such weight file or directory; from_pretrained reads local files only")
        return cls(pretrained=True, weights_path=path, **kw)

    # ---- kernel-layout copies --------------------------------------------------------------------------------------------------------------
    def packed(self):
        """{name: (weight, bias)} in the kernels' layout, fp32: [3,3,Cin,Cout] for the 3x3 layers, [256,65] / [256,256] for convPb / convDb"""
        params = [p for name, *_ in LAYERS for p in (getattr(self, name).weight, getattr(self, name).bias)]

        def make():
            out = {}
            for name, _, _, ks in LAYERS:
                c = getattr(self, name)
                w = ops.pack_conv_weight(c.weight)
                out[name] = (w if ks == 3 else w[0, 0].contiguous(), c.bias.detach().float().contiguous())
            out["table"] = ops.sp_gray_table(params[0].device)
            return out
        return self._packed.get("all", params, make)

    # ---- the network -----------------------------------------------------------------------------------------------------------------------
    def _check(self, x, what):
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("SuperPoint on the device is forward only: call it under torch.no_grad()")
        if not x.is_cuda:
            raise RuntimeError("videogpa_amd.superpoint.SuperPoint runs on the GPU only (no CPU fallback)")
        if not self.conv1a.weight.is_cuda:
            raise RuntimeError("SuperPoint: the module's weights are not on the GPU (no CPU fallback): call .cuda() first")
        if x.shape[0] < 1 or min(what) < 8:
            raise ValueError(f"SuperPoint: needs at least one frame of 8 x 8 pixels (three 2 x 2 pools), got {tuple(x.shape)}")

    def _maps(self, src, size=None, taps=None):
        """frames (uint8 [n,H,W,3] or fp32 [n,1|3,H,W]) -> (score image [n,8h,8w], raw descriptor map [n,h,w,256]); `taps` collects intermediates"""
        p = self.packed()
        tap = (lambda k, v: taps.__setitem__(k, v)) if taps is not None else (lambda k, v: None)
        table = p["table"] if src.dtype == torch.uint8 else None
        if taps is not None:
            h, taps["gray"] = ops.sp_input_conv1a(src, *p["conv1a"], size=size, table=table, return_gray=True)
        else:
            h = ops.sp_input_conv1a(src, *p["conv1a"], size=size, table=table)
        tap("conv1a", h)
        for name in ("conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b"):
            h = ops.conv3x3_f32(h, *p[name], relu_in=name != "conv2a" and name != "conv3a" and name != "conv4a")   # a pool's output has its ReLU already
            if name in ("conv1b", "conv2b", "conv3b"):
                h = ops.maxpool2x2_f32(h, relu=True)
        score = ops.sp_head_f32(ops.conv3x3_f32(h, *p["convPa"], relu_in=True), *p["convPb"])
        dmap = ops.conv1x1_relu_f32(ops.conv3x3_f32(h, *p["convDa"], relu_in=True), *p["convDb"])
        tap("scores", score)
        tap("dmap", dmap)
        return score, dmap

    def _detect(self, src, size=None, taps=None):
        """-> keypoints [n,K,2] (x, y) in the network's input frame, scores [n,K], descriptors [n,K,256], counts int32 [n] (on the device)"""
        score, dmap = self._maps(src, size, taps)
        nms = ops.sp_nms_f32(score, self.conf["nms_radius"], self.conf["remove_borders"])
        kp, sc, counts = ops.sp_select(nms, self.conf["detection_threshold"], self.conf["max_num_keypoints"])
        desc = ops.sp_sample_desc_f32(dmap, kp, counts)
        if taps is not None:
            taps["nms"] = nms
        return kp, sc, desc, counts

    def _image(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] not in (1, 3) or x.dtype != torch.float32:
            raise ValueError(f"SuperPoint: the image is an fp32 [B,1,H,W] or [B,3,H,W] tensor, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}"
                             f"{' ' + str(x.dtype) if isinstance(x, torch.Tensor) else ''}")
        self._check(x, x.shape[-2:])
        return x.contiguous()

    def _stacked(self, kp, sc, desc, counts):
        n = counts.tolist()
        if len(set(n)) != 1:
            raise RuntimeError(f"SuperPoint: the frames of the batch keep different numbers of keypoints {n}: they cannot be stacked (upstream's torch.stack "
                               "raises here too); extract them one by one or use extract_clip")
        return {"keypoints": kp[:, :n[0]], "keypoint_scores": sc[:, :n[0]], "descriptors": desc[:, :n[0]]}

    def forward(self, data, taps=None):
        x = self._image(data["image"])
        with torch.no_grad():
            return self._stacked(*self._detect(x, taps=taps))

    def _target(self, H, W, resize):
        """the size Extractor.extract resizes (H, W) to, and scales = (W'/W, H'/H)"""
        if resize is None:
            return (H, W), (1.0, 1.0)
        Ho, Wo = side_to_image_size((H, W), int(resize), self.preprocess_conf["side"]) if isinstance(resize, int) else tuple(resize)
        if Ho < H or Wo < W:
            raise NotImplementedError(f"SuperPoint.extract: resizing {H} x {W} to {Ho} x {Wo} shrinks the frame; upstream's down-scaling is kornia's "
                                      "antialiased form (a Gaussian pre-blur), which is not implemented")
        return (Ho, Wo), (Wo / W, Ho / H)

    def _rescaled(self, kp, scales, dev):
        return (kp + 0.5) / torch.tensor(scales, dtype=torch.float32, device=dev)[None] - 0.5

    def extract(self, img, **conf):
        """upstream's Extractor.extract: img [1|3,H,W] or [B,1|3,H,W] in [0,1]; keypoints come back in the coordinates of `img`"""
        if isinstance(img, torch.Tensor) and img.dim() == 3:
            img = img[None]
        x = self._image(img)
        H, W = x.shape[-2:]
        size, scales = self._target(H, W, {**self.preprocess_conf, **conf}["resize"])
        with torch.no_grad():
            feats = self._stacked(*self._detect(x, size=size))
            feats["image_size"] = torch.tensor([[W, H]] * x.shape[0], dtype=torch.float32, device=x.device)
            feats["keypoints"] = self._rescaled(feats["keypoints"], scales, x.device)
        return feats

    def extract_clip(self, frames_u8, resize="default", frames_chunk=None):
        """[T,H,W,3] uint8 frames (host or device) -> a list of T feature dicts as `extract` gives for the reference's `_frame2tensor(frame)`, each with a
        batch axis of 1.  Every frame goes through the network once, `frames_chunk` frames at a time; the counts are read from the device once."""
        f = torch.as_tensor(frames_u8)
        if f.dim() != 4 or f.shape[-1] != 3 or f.dtype != torch.uint8:
            raise ValueError(f"SuperPoint.extract_clip: frames are uint8 [T,H,W,3], got {f.dtype} {tuple(f.shape)}")
        if not self.conv1a.weight.is_cuda:
            raise RuntimeError("SuperPoint: the module's weights are not on the GPU (no CPU fallback): call .cuda() first")
        f = f.to(self.conv1a.weight.device).contiguous()
        T, H, W, _ = f.shape
        self._check(f, (H, W))
        size, scales = self._target(H, W, self.preprocess_conf["resize"] if resize == "default" else resize)
        chunk = self.frames_chunk if frames_chunk is None else int(frames_chunk)
        with torch.no_grad():
            parts = [self._detect(f[s:s + chunk], size=size) for s in range(0, T, chunk)]
            counts = torch.cat([p[3] for p in parts]).tolist()                     # the one host read of the clip
            image_size = torch.tensor([[W, H]], dtype=torch.float32, device=f.device)
            out = []
            for ci, (kp, sc, desc, _) in enumerate(parts):
                for j in range(kp.shape[0]):
                    n = counts[ci * chunk + j]
                    out.append({"keypoints": self._rescaled(kp[j:j + 1, :n], scales, f.device), "keypoint_scores": sc[j:j + 1, :n],
                                "descriptors": desc[j:j + 1, :n], "image_size": image_size})
        return out
