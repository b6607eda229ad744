"""A torch restatement of upstream SuperPoint (cvg/LightGlue: lightglue/superpoint.py, Extractor.extract of lightglue/utils.py) written from its
definitions: F.conv2d, F.max_pool2d, F.grid_sample, a stable descending sort for the cut.  It evaluates on the CPU in the dtype it is given (float64:
the answer; float32: the distance every fp32 evaluation is allowed).  Nothing here imports the package under test."""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = (("conv1a", 1, 64, 3), ("conv1b", 64, 64, 3), ("conv2a", 64, 64, 3), ("conv2b", 64, 64, 3), ("conv3a", 64, 128, 3), ("conv3b", 128, 128, 3),
          ("conv4a", 128, 128, 3), ("conv4b", 128, 128, 3), ("convPa", 128, 256, 3), ("convPb", 256, 65, 1), ("convDa", 128, 256, 3),
          ("convDb", 256, 256, 1))
NAMES = [f"{n}.{p}" for n, *_ in LAYERS for p in ("weight", "bias")]
GRAY = (9798, 19235, 3735, 15)            # cv2's 8-bit RGB2GRAY in 15-bit fixed point, restated from memory (unpinned)


def state(seed=1):
    """He-scaled normal weights with 0.1 * normal biases from one seeded generator"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cin, cout, ks in LAYERS:
        sd[f"{name}.weight"] = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (ks * ks * cin)) ** 0.5
        sd[f"{name}.bias"] = 0.1 * torch.randn(cout, generator=g)
    return sd


def noise_frames(T, H, W, seed):
    """uint8 [T,H,W,3] of torch.rand"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(T, H, W, 3, generator=g) * 255).round().to(torch.uint8)


def smooth_frames(T, H, W, seed):
    """uniform noise at 1/6 resolution, bicubic up, clamped, rounded to bytes"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(T, 3, max(H // 6, 2), max(W // 6, 2), generator=g)
    up = F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False).clamp(0, 1)
    return (up * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def gray_bytes(frames_u8):
    """integer numpy evaluation of the gray conversion: uint8 [T,H,W,3] -> uint8 [T,H,W]"""
    f = np.asarray(frames_u8).astype(np.int64)
    r, g, b, sh = GRAY
    return ((r * f[..., 0] + g * f[..., 1] + b * f[..., 2] + (1 << (sh - 1))) >> sh).astype(np.uint8)


def frame2tensor(frames_u8):
    """the reference's `_frame2tensor` for a stack of frames: fp32 [T,1,H,W] = (gray / 255.0).float()"""
    return torch.from_numpy(gray_bytes(frames_u8) / 255.0).float()[:, None]


def side_to_image_size(h, w, side_size):
    """long side to side_size, the other truncated"""
    aspect = w / h
    return (side_size, int(side_size * aspect)) if aspect < 1.0 else (int(side_size / aspect), side_size)


def resize(img, size):
    return F.interpolate(img, size=size, mode="bilinear", align_corners=False)


def backbone(sd, img):
    """img [T,1,H,W] -> dict of conv1a (before its ReLU), scores [T,8h,8w] (before NMS), dmap (convDb's output, [T,256,h,w]), all in img's dtype"""
    c = lambda name, x: F.conv2d(x, sd[name + ".weight"].to(img.dtype), sd[name + ".bias"].to(img.dtype), padding=sd[name + ".weight"].shape[-1] // 2)
    out = {"conv1a": c("conv1a", img)}
    x = F.relu(out["conv1a"])
    x = F.max_pool2d(F.relu(c("conv1b", x)), 2, 2)
    x = F.max_pool2d(F.relu(c("conv2b", F.relu(c("conv2a", x)))), 2, 2)
    x = F.max_pool2d(F.relu(c("conv3b", F.relu(c("conv3a", x)))), 2, 2)
    x = F.relu(c("conv4b", F.relu(c("conv4a", x))))
    s = F.softmax(c("convPb", F.relu(c("convPa", x))), 1)[:, :-1]
    b, _, h, w = s.shape
    out["scores"] = s.permute(0, 2, 3, 1).reshape(b, h, w, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, h * 8, w * 8)
    out["dmap"] = c("convDb", F.relu(c("convDa", x)))
    return out


def simple_nms(scores, radius):
    pool = lambda x: F.max_pool2d(x, kernel_size=radius * 2 + 1, stride=1, padding=radius)
    zeros = torch.zeros_like(scores)
    max_mask = scores == pool(scores)
    for _ in range(2):
        supp_mask = pool(max_mask.to(scores.dtype)) > 0
        supp_scores = torch.where(supp_mask, zeros, scores)
        new_max_mask = supp_scores == pool(supp_scores)
        max_mask = max_mask | (new_max_mask & (~supp_mask))
    return torch.where(max_mask, scores, zeros)


def nms_borders(scores, radius, border):
    s = simple_nms(scores, radius).clone()
    if border:
        s[:, :border] = -1
        s[:, :, :border] = -1
        s[:, -border:] = -1
        s[:, :, -border:] = -1
    return s


def select(nms_img, threshold, k):
    """one frame [Hs,Ws] -> (keypoints [N,2] as (x, y) in the image's dtype, scores [N]): row-major when nothing is cut, else a stable descending sort"""
    ys, xs = torch.where(nms_img > threshold)
    sc = nms_img[ys, xs]
    kp = torch.stack([xs, ys], -1)
    if k is not None and k < len(sc):
        order = torch.sort(sc, descending=True, stable=True).indices[:k]
        kp, sc = kp[order], sc[order]
    return kp.to(nms_img.dtype), sc


def sample_descriptors(kp, dmap, s=8):
    """kp [N,2], dmap [256,h,w] raw -> [N,256]: normalize, sample_descriptors, normalize"""
    d = F.normalize(dmap[None], p=2, dim=1)
    _, c, h, w = d.shape
    k = kp[None].to(d.dtype) - s / 2 + 0.5
    k = k / torch.tensor([(w * s - s / 2 - 0.5), (h * s - s / 2 - 0.5)]).to(k)[None]
    k = k * 2 - 1
    out = F.grid_sample(d, k.view(1, 1, -1, 2), mode="bilinear", align_corners=True)
    return F.normalize(out.reshape(1, c, -1), p=2, dim=1)[0].t()


def detect(sd, img, radius=4, border=4, threshold=0.0005, k=None):
    """img [T,1,H,W] -> per frame (kp, scores, descriptors), plus the backbone's maps"""
    m = backbone(sd, img)
    nms = nms_borders(m["scores"], radius, border)
    frames = []
    for t in range(img.shape[0]):
        kp, sc = select(nms[t], threshold, k)
        frames.append((kp, sc, sample_descriptors(kp, m["dmap"][t])))
    return frames, m


def nms_brute(s, radius):
    """simple_nms of one [H,W] numpy map by explicit window loops"""
    H, W = s.shape

    def pool(x):
        out = np.empty_like(x)
        for y in range(H):
            for xx in range(W):
                out[y, xx] = x[max(y - radius, 0):y + radius + 1, max(xx - radius, 0):xx + radius + 1].max()
        return out
    mask = s == pool(s)
    for _ in range(2):
        supp = pool(mask.astype(s.dtype)) > 0
        s2 = np.where(supp, 0, s)
        mask = mask | ((s2 == pool(s2)) & ~supp)
    return np.where(mask, s, 0)


def rel_err(got, want64):
    want64 = want64.double()
    return float((got.detach().cpu().double() - want64).abs().max() / want64.abs().max())


def keyset(kp):
    return {(int(x), int(y)) for x, y in kp.tolist()}


def mutual_nn(feats):
    """the stand-in matcher of the tests: mutual nearest neighbours on the descriptors, in torch"""
    d0, d1 = feats["image0"]["descriptors"][0], feats["image1"]["descriptors"][0]
    sim = d0 @ d1.t()
    a, b = sim.argmax(1), sim.argmax(0)
    i = torch.arange(len(a), device=a.device)
    keep = b[a] == i
    return {"matches": [torch.stack([i[keep], a[keep]], -1)]}
