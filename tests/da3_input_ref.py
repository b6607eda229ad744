"""Oracles for Depth Anything 3's input processing (videogpa_amd/da3_input.py, csrc/da3_input.hip), in numpy, written from what the operations mean
and not from the kernels:

  area_matrix / area_exact      INTER_AREA as its tap table (computeResizeAreaTab) in float64, accumulated in float64 -> a real-valued image `a`
  cubic_matrix / cubic_exact    the exact A = -0.75 cubic convolution in float64 (clamped taps), real-valued
  cubic_fixed                   the 8-bit fixed-point scheme (fp32 weights fixed to 11 bits, int accumulation, one rounding at 22 bits) in int64
  normalize / processed_images  ToTensor + Normalize in torch fp32, and api.py:_add_processed_images' numpy expression applied to the whole image
  process_one / unify           InputProcessor's sizes, interpolation choices, crop boxes and intrinsics, one frame at a time as the reference walks them

cv2 itself is not a dependency of this project and varies by build; tests/test_gpu_da3_input.py says what is asserted instead."""
import math

import numpy as np
import torch

MEAN = [0.485, 0.456, 0.406]
STD = [0.229, 0.224, 0.225]
PATCH = 14


# ------------------------------------------------------------------------------------------------------------------------ frames
def frames(T, H, W, seed):
    """T frames: even ones seeded random bytes, odd ones a smooth sinusoid pattern"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        if t % 2 == 0:
            out[t] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        else:
            for c in range(3):
                out[t, :, :, c] = np.rint(127.5 + 127.5 * np.sin(0.21 * xx * (c + 1) + 0.4 * t) * np.cos(0.17 * yy + 0.3 * c)).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------------------------------ area
def area_matrix(n_in, n_out):
    """[n_out, n_in] float64: row dx holds the weights of output sample dx"""
    assert n_out <= n_in
    scale = 1.0 / (float(n_out) / n_in)
    M = np.zeros((n_out, n_in), np.float64)
    for dx in range(n_out):
        f1 = dx * scale
        f2 = f1 + scale
        cell = min(scale, n_in - f1)
        s1, s2 = math.ceil(f1), min(math.floor(f2), n_in - 1)
        s1 = min(s1, s2)
        if s1 - f1 > 1e-3:
            M[dx, s1 - 1] += (s1 - f1) / cell
        for s in range(s1, s2):
            M[dx, s] += 1.0 / cell
        if f2 - s2 > 1e-3:
            M[dx, s2] += min(min(f2 - s2, 1.0), cell) / cell
    return M


def _separable(img, My, Mx):
    """img [T,H,W,3] -> [T,h,w,3] float64 = My applied to rows, Mx to columns"""
    return np.einsum("yh,thwc,xw->tyxc", My, img.astype(np.float64), Mx, optimize=True)


def area_exact(img, out_h, out_w):
    return _separable(img, area_matrix(img.shape[1], out_h), area_matrix(img.shape[2], out_w))


def box_sum(img, out_h, out_w):
    """integer scales: the int64 sum over each isy x isx box"""
    T, H, W, C = img.shape
    isy, isx = H // out_h, W // out_w
    assert isy * out_h == H and isx * out_w == W
    return img.astype(np.int64).reshape(T, out_h, isy, out_w, isx, C).sum(axis=(2, 4))


# ------------------------------------------------------------------------------------------------------------------------ cubic
def _keys(x, A):
    """Keys' kernel at distance |x| < 2"""
    x = abs(x)
    if x <= 1.0:
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def cubic_matrix(n_in, n_out, A=-0.75):
    scale = 1.0 / (float(n_out) / n_in)
    M = np.zeros((n_out, n_in), np.float64)
    for dx in range(n_out):
        f = (dx + 0.5) * scale - 0.5
        s = math.floor(f)
        for k in range(-1, 3):
            M[dx, min(max(s + k, 0), n_in - 1)] += _keys(f - (s + k), A)
    return M


def cubic_exact(img, out_h, out_w, A=-0.75):
    return _separable(img, cubic_matrix(img.shape[1], out_h, A), cubic_matrix(img.shape[2], out_w, A))


def cubic_fixed_table(n_in, n_out):
    """-> (index [n_out, 4] clamped, weight [n_out, 4] int64): fp32 Keys weights with A = -0.75, each fixed to rint(c * 2048)"""
    f32 = np.float32
    scale = 1.0 / (float(n_out) / n_in)
    idx, wt = np.zeros((n_out, 4), np.int64), np.zeros((n_out, 4), np.int64)
    A, one = f32(-0.75), f32(1)
    for dx in range(n_out):
        fx = f32((dx + 0.5) * scale - 0.5)
        sx = int(np.floor(fx))
        fx = f32(fx - f32(sx))
        u, v = f32(fx + one), f32(one - fx)
        c0 = f32(f32(f32(f32(f32(f32(A * u) - f32(5) * A) * u) + f32(8) * A) * u) - f32(4) * A)
        c1 = f32(f32(f32(f32(f32(A + f32(2)) * fx) - f32(A + f32(3))) * fx) * fx + one)
        c2 = f32(f32(f32(f32(f32(A + f32(2)) * v) - f32(A + f32(3))) * v) * v + one)
        c3 = f32(f32(f32(one - c0) - c1) - c2)
        for k, c in enumerate((c0, c1, c2, c3)):
            idx[dx, k] = min(max(sx - 1 + k, 0), n_in - 1)
            wt[dx, k] = int(np.rint(f32(c * f32(2048))))
    return idx, wt


def cubic_fixed(img, out_h, out_w):
    """uint8 [T,H,W,3] -> uint8 [T,out_h,out_w,3]: horizontal pass unshifted, vertical pass (acc + 2^21) >> 22, saturated; int64 throughout"""
    ix, wx = cubic_fixed_table(img.shape[2], out_w)
    iy, wy = cubic_fixed_table(img.shape[1], out_h)
    src = img.astype(np.int64)
    hor = (src[:, :, ix, :] * wx[None, None, :, :, None]).sum(axis=3)                   # [T,H,out_w,3]
    acc = (hor[:, iy, :, :] * wy[None, :, :, None, None]).sum(axis=2)                   # [T,out_h,out_w,3]
    return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------ the last stage
def normalize(u8):
    """uint8 [T,h,w,3] -> fp32 [1,T,3,h,w]: ToTensor (`.to(float32).div(255)`), then Normalize (`sub_(mean).div_(std)`), on the CPU"""
    x = torch.from_numpy(np.ascontiguousarray(u8)).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    mean, std = torch.tensor(MEAN, dtype=torch.float32).view(-1, 1, 1), torch.tensor(STD, dtype=torch.float32).view(-1, 1, 1)
    return x.sub_(mean).div_(std)[None]


def processed_images(x):
    """api.py:_add_processed_images on x fp32 [1,T,3,h,w] (a torch tensor)"""
    p = x[0].permute(0, 2, 3, 1).cpu().numpy()
    p = p * np.array(STD) + np.array(MEAN)
    p = np.clip(p, 0, 1)
    return (p * 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------ InputProcessor's host logic
def _nearest_multiple(x, p):
    down = (x // p) * p
    up = down + p
    return up if abs(up - x) <= abs(x - down) else down


def process_one(H, W, K, process_res, method):
    """one frame through `_process_one`: -> (ops, (h, w), K) with ops = [("area" | "cubic", out_h, out_w) | ("crop", top, left, h, w)] in order"""
    ops = []
    w, h = W, H
    K = None if K is None else np.array(K, copy=True)

    def scale_k(K, ow, oh, nw, nh):
        if K is None:
            return None
        K = K.copy()
        K[:1] *= nw / float(ow)
        K[1:2] *= nh / float(oh)
        return K

    side = max(w, h) if method in ("upper_bound_resize", "upper_bound_crop") else min(w, h)
    assert method in ("upper_bound_resize", "upper_bound_crop", "lower_bound_resize", "lower_bound_crop")
    if side != process_res:
        s = process_res / float(side)
        nw, nh = max(1, int(round(w * s))), max(1, int(round(h * s)))
        ops.append(("cubic" if s > 1.0 else "area", nh, nw))
        w, h = nw, nh
    K = scale_k(K, W, H, w, h)
    if method.endswith("resize"):
        nw, nh = max(1, _nearest_multiple(w, PATCH)), max(1, _nearest_multiple(h, PATCH))
        if (nw, nh) != (w, h):
            ops.append(("cubic" if (nw > w) or (nh > h) else "area", nh, nw))
        K = scale_k(K, w, h, nw, nh)
    else:
        nw, nh = (w // PATCH) * PATCH, (h // PATCH) * PATCH
        left, top = (w - nw) // 2, (h - nh) // 2
        if (nw, nh) != (w, h):
            ops.append(("crop", top, left, nh, nw))
        if K is not None:
            K = K.copy()
            K[0, 2] -= left
            K[1, 2] -= top
    return ops, (nh, nw), K


def unify(sizes, Ks):
    """`_unify_batch_shapes`: -> (per-frame crop (top, left), (min_h, min_w), Ks)"""
    if len(set(sizes)) <= 1:
        return [(0, 0)] * len(sizes), sizes[0], Ks
    mh, mw = min(h for h, _ in sizes), min(w for _, w in sizes)
    crops, out = [], []
    for (h, w), K in zip(sizes, Ks):
        top, left = max(0, (h - mh) // 2), max(0, (w - mw) // 2)
        crops.append((top, left))
        if K is not None:
            K = K.copy()
            K[0, 2] -= left
            K[1, 2] -= top
        out.append(K)
    return crops, (mh, mw), out
