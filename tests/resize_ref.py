"""TEST INFRASTRUCTURE -- numpy restatement of PIL `Image.resize(size, BICUBIC | LANCZOS)` for 8-bit RGB images, written from Pillow's published
algorithm (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc) and independent of
videogpa_amd/csrc/preprocess.hip.  tests/test_i2v_host.py pins it against PIL itself byte for byte; tests/test_gpu_i2v.py holds the device to it.

    filter      support  kernel
    bicubic     2        a = -0.5 Keys cubic
    lanczos     3        sinc(x) sinc(x / 3) on [-3, 3),  sinc(x) = sin(pi x) / (pi x)
Per output sample: scale = in / out, filterscale = max(scale, 1), the taps cover [center - support filterscale, center + support filterscale) cut to the
image, weights filter((x - center + 0.5) / filterscale) normalised by their sum in double, fixed to 22 fractional bits rounding half away from zero; a
pass accumulates in integers from 1 << 21, shifts by 22 and clips to [0, 255].  Horizontal pass first, vertical second, a pass whose size does not change
is skipped, and so the image between the passes is uint8."""
import math

import numpy as np

BITS = 22
SUPPORT = {"bicubic": 2.0, "lanczos": 3.0}

# the four cases of the issue as (H, W) -> (out_h, out_w), and a 1-pixel-wide source
SIZES = [((720, 1080), (480, 720)), ((37, 53), (48, 64)), ((200, 310), (40, 62)), ((9, 1), (12, 7))]


def _cubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


FILTER = {"bicubic": _cubic, "lanczos": _lanczos}


def coefficients(in_size, out_size, filter):
    """-> list of (first input sample, int weights) per output sample"""
    f, scale = FILTER[filter], in_size / out_size
    fscale = max(scale, 1.0)
    support = SUPPORT[filter] * fscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = [f((x - center + 0.5) * (1.0 / fscale)) for x in range(lo, hi)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        out.append((lo, np.array([int(-0.5 + v * (1 << BITS)) if v < 0 else int(0.5 + v * (1 << BITS)) for v in w], np.int64)))
    return out


def _one_pass(img, out_size, filter, axis):
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    rows = [np.clip((np.tensordot(k, src[lo:lo + len(k)], axes=(0, 0)) + (1 << (BITS - 1))) >> BITS, 0, 255)
            for lo, k in coefficients(src.shape[0], out_size, filter)]
    return np.moveaxis(np.stack(rows).astype(np.uint8), 0, axis)


def resize(img, out_h, out_w, filter):
    """uint8 [H, W, 3] -> uint8 [out_h, out_w, 3]"""
    if img.shape[1] != out_w:
        img = _one_pass(img, out_w, filter, 1)
    if img.shape[0] != out_h:
        img = _one_pass(img, out_h, filter, 0)
    return img


def test_image(H, W, seed=0):
    """uint8 [H, W, 3]: smooth gradients plus noise plus saturated blocks (both clips after a pass are reached next to their edges)"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([127 + 120 * np.sin(0.07 * x + 0.03 * y), 255.0 * x / max(W - 1, 1), 255.0 * y / max(H - 1, 1)], -1) + rng.normal(0, 25, (H, W, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    img[: max(H // 5, 1), : max(W // 4, 1)] = 255
    img[H // 2: H // 2 + max(H // 6, 1), W // 3: W // 3 + max(W // 5, 1)] = 0
    return img
