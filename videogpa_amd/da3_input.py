"""Depth Anything 3's `InputProcessor` (depth_anything_3/utils/io/input_processor.py) with the pixels on the device: uint8 frames of any size ->
the network's input `x [1,T,3,h,w]` (ImageNet-normalised fp32, h and w multiples of 14), the transformed intrinsics, and the `processed_images`
uint8 [T,h,w,3] that api.py:_add_processed_images derives from `x` and the scorer compares against.

What stays on the host is integer arithmetic: `plan(H, W, process_res, method)` restates the sizes (`int(round(w * scale))`), the choice of
INTER_AREA when not upscaling and INTER_CUBIC when upscaling (`_resize_longest_side`, `_resize_shortest_side`, `_make_divisible_by_resize`), the
centre crop of `_make_divisible_by_crop`, and with them `_resize_ixt` / `_crop_ixt` / `_unify_batch_shapes`.  Every stage of a plan is one launch of
csrc/da3_input.hip over all frames of one size (ops.da3_resize / ops.da3_normalize); the last stage writes `x` and `processed_images` together, as the
last resize's epilogue where no crop follows it.  OpenCV is not used: the kernels restate its 8-bit INTER_AREA / INTER_CUBIC (which of its variants, and
why no build of it is pinned bit for bit, is in the header of csrc/da3_input.hip and in DESIGN.md section 5j).  No CPU fallback.

Paths and PIL images are decoded by the caller: frames arrive as uint8 arrays or tensors."""
import functools

import numpy as np
import torch

from . import ops

PATCH_SIZE = 14
METHODS = ("upper_bound_resize", "upper_bound_crop", "lower_bound_resize", "lower_bound_crop")
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


# ------------------------------------------------------------------------------------------------------------------------ host arithmetic
def _nearest_multiple(x, p):
    down = (x // p) * p
    up = down + p
    return up if abs(up - x) <= abs(x - down) else down


def plan(H, W, process_res=504, method="upper_bound_resize"):
    """-> (stages, (h, w)): what `_process_one` does to one H x W frame.  A stage is ("area" | "cubic", out_h, out_w) -- a cv2.resize with that
    interpolation -- or ("crop", top, left, h, w); (h, w) is the size the network sees.  The stages are listed as the reference runs them, a
    resize to the size the image already has included (`_resize_*_side` does not skip it; it is the identity in both modes)."""
    if method not in METHODS:
        raise ValueError(f"Unsupported process_res_method: {method}")
    H, W, process_res = int(H), int(W), int(process_res)
    if H <= 0 or W <= 0 or process_res <= 0:
        raise ValueError(f"no plan for frames of {H} x {W} at process_res {process_res}")
    stages = []
    h, w = H, W
    side = max(w, h) if method.startswith("upper_bound") else min(w, h)
    if side != process_res:                                   # _resize_longest_side / _resize_shortest_side
        scale = process_res / float(side)
        nw, nh = max(1, int(round(w * scale))), max(1, int(round(h * scale)))
        stages.append(("cubic" if scale > 1.0 else "area", nh, nw))
        h, w = nh, nw
    if method.endswith("resize"):                             # _make_divisible_by_resize
        nw, nh = max(1, _nearest_multiple(w, PATCH_SIZE)), max(1, _nearest_multiple(h, PATCH_SIZE))
        if (nw, nh) != (w, h):
            stages.append(("cubic" if (nw > w or nh > h) else "area", nh, nw))
            h, w = nh, nw
    else:                                                     # _make_divisible_by_crop
        nw, nh = (w // PATCH_SIZE) * PATCH_SIZE, (h // PATCH_SIZE) * PATCH_SIZE
        if nw <= 0 or nh <= 0:
            raise ValueError(f"{method}: a {H} x {W} frame at process_res {process_res} is {h} x {w} before the crop, smaller than one {PATCH_SIZE}-pixel patch")
        if (nw, nh) != (w, h):
            stages.append(("crop", (h - nh) // 2, (w - nw) // 2, nh, nw))
            h, w = nh, nw
    return stages, (h, w)


def resize_ixt(K, orig_w, orig_h, w, h):
    """_resize_ixt: fx, cx by the width ratio, fy, cy by the height ratio, in K's own dtype"""
    if K is None:
        return None
    K = K.copy()
    K[:1] *= w / float(orig_w)
    K[1:2] *= h / float(orig_h)
    return K


def crop_ixt(K, left, top):
    """_crop_ixt / _unify_batch_shapes: the principal point moves with the crop"""
    if K is None:
        return None
    K = K.copy()
    K[0, 2] -= left
    K[1, 2] -= top
    return K


def plan_ixt(K, H, W, stages):
    """the intrinsics of one frame behind the stages of `plan(H, W, ...)`.  `_process_one` applies `_resize_ixt` once for the boundary resize (a ratio of
    1.0 when it is skipped) and once for the divisibility resize; multiplying by 1.0 changes nothing, so one call per resize stage is the same."""
    if K is None:
        return None
    h, w = H, W
    for st in stages:
        if st[0] == "crop":
            K = crop_ixt(K, st[2], st[1])
            h, w = st[3], st[4]
        else:
            K = resize_ixt(K, w, h, st[2], st[1])
            h, w = st[1], st[2]
    return K


def processed_table():
    """uint8 [3, 256]: `processed_images` for every (channel, byte), with api.py:_add_processed_images' own expression on the fp32 normalised value:
    float32 x times float64 std plus float64 mean, clip to [0, 1], times 255, truncate.  (It is not always the byte it came from.)"""
    u = np.arange(256, dtype=np.float32)[None, :]
    mean32, std32 = np.asarray(MEAN, np.float32)[:, None], np.asarray(STD, np.float32)[:, None]
    x = (u / np.float32(255.0) - mean32) / std32                       # ToTensor, then Normalize's sub_ and div_: fp32 throughout
    assert x.dtype == np.float32
    p = x * np.array(STD)[:, None] + np.array(MEAN)[:, None]           # float64, as numpy promotes it upstream
    p = np.clip(p, 0, 1)
    return (p * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _device_table(device):
    return torch.from_numpy(processed_table()).to(device)


# ------------------------------------------------------------------------------------------------------------------------ the processor
def _as_u8(frame):
    if isinstance(frame, str):
        raise TypeError("InputProcessor takes decoded frames (uint8 [H,W,3] arrays or tensors), not paths: image and video decoding is the caller's")
    t = frame if torch.is_tensor(frame) else torch.as_tensor(np.asarray(frame))
    if t.dtype != torch.uint8 or t.ndim != 3 or t.shape[-1] != 3:
        raise ValueError(f"InputProcessor takes uint8 frames [H,W,3], got {t.dtype} {tuple(t.shape)}")
    return t


def _host_meta(a, n, name):
    if a is None:
        return None
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if len(a) != n:
        raise ValueError(f"Length of {name} must match images when provided.")
    return [k for k in a]


class InputProcessor:
    """`InputProcessor()(image, extrinsics, intrinsics, process_res, process_res_method) -> (x [1,T,3,h,w] on the device, extrinsics, intrinsics)` as
    the reference's (its batch tensor is [T,3,h,w] on the host; api.py adds the batch axis when it moves it to the device).  `process(...)` returns
    `processed_images` as a fourth value.  `image`: a list of uint8 frames [H,W,3] or one uint8 array / tensor [T,H,W,3], on the host or the device."""

    PATCH_SIZE = PATCH_SIZE

    def __init__(self, device="cuda"):
        self.device = torch.device(device)

    def __call__(self, image, extrinsics=None, intrinsics=None, process_res=504, process_res_method="upper_bound_resize"):
        return self.process(image, extrinsics, intrinsics, process_res, process_res_method)[:3]

    def _groups(self, image):
        """-> [(indices, uint8 [Tg,H,W,3] on the device)] with frames of one size together, in order of first appearance"""
        if isinstance(image, str):
            _as_u8(image)
        if not isinstance(image, (list, tuple)):
            t = image if torch.is_tensor(image) else torch.as_tensor(np.asarray(image))
            if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[-1] != 3:
                raise ValueError(f"InputProcessor takes a list of uint8 frames [H,W,3] or uint8 [T,H,W,3], got {t.dtype} {tuple(t.shape)}")
            return len(t), [(list(range(len(t))), t.to(self.device).contiguous())]
        frames = [_as_u8(f) for f in image]
        if not frames:
            raise ValueError("InputProcessor: no frames")
        by_size = {}
        for i, f in enumerate(frames):
            by_size.setdefault(tuple(f.shape[:2]), []).append(i)
        return len(frames), [(idx, torch.stack([frames[i] for i in idx]).to(self.device).contiguous()) for idx in by_size.values()]

    def process(self, image, extrinsics=None, intrinsics=None, process_res=504, process_res_method="upper_bound_resize"):
        n, groups = self._groups(image)
        exts, ixts = _host_meta(extrinsics, n, "extrinsics"), _host_meta(intrinsics, n, "intrinsics")
        plans = [plan(g.shape[1], g.shape[2], process_res, process_res_method) for _, g in groups]
        min_h, min_w = min(hw[0] for _, hw in plans), min(hw[1] for _, hw in plans)      # _unify_batch_shapes: centre crop to the smallest
        table = _device_table(self.device)
        xs, procs, order = [], [], []
        out_ixts = [None] * n
        for (idx, g), (stages, (h, w)) in zip(groups, plans):
            if (h, w) != (min_h, min_w):
                stages = stages + [("crop", (h - min_h) // 2, (w - min_w) // 2, min_h, min_w)]
            if ixts is not None:
                for i in idx:
                    out_ixts[i] = plan_ixt(ixts[i], g.shape[1], g.shape[2], stages)
            x, proc = self._run(g, stages, table)
            xs.append(x)
            procs.append(proc)
            order += idx
        x, proc = (xs[0], procs[0]) if len(xs) == 1 else (torch.cat(xs, 1), torch.cat(procs, 0))
        if order != sorted(order):
            inv = torch.tensor(order, device=self.device).argsort()
            x, proc = x.index_select(1, inv), proc.index_select(0, inv)
        out_exts = torch.from_numpy(np.asarray(exts)).float() if exts is not None else None
        out_ixts = torch.from_numpy(np.asarray(out_ixts)).float() if ixts is not None else None
        return x, out_exts, out_ixts, proc

    @staticmethod
    def _run(frames, stages, table):
        """one launch per stage over the whole group.  Crops only ever follow the resizes (the divisibility crop, then the unifying one): they fold into the
        box of the last stage"""
        box = None                                             # pending crop (top, left, h, w) of `frames`
        for k, st in enumerate(stages):
            if st[0] == "crop":
                top, left = (st[1], st[2]) if box is None else (box[0] + st[1], box[1] + st[2])
                box = (top, left, st[3], st[4])
            elif box is not None:
                raise ValueError(f"a resize behind a crop is not a plan of InputProcessor: {stages}")
            elif k == len(stages) - 1:
                return ops.da3_resize(frames, st[1], st[2], st[0], table=table)
            else:
                frames = ops.da3_resize(frames, st[1], st[2], st[0])
        return ops.da3_normalize(frames, table, box)
