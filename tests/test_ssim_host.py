"""SSIMMetric without a GPU: the public surface, the C-ABI entries, the loud failure, and the restatement of piq.ssim the GPU tests compare against
(tests/test_gpu_ssim.py imports it from here).

`piq` is not vendored, so the contract is restated (unpinned) from piq.ssim as metrics/mse.py:101-110 calls it: kernel_size=11, kernel_sigma=1.5,
data_range=1.0, reduction="mean", full=False, downsample=True, k1=0.01, k2=0.03."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the restatement
def ssim_factor(H, W):
    return max(1, round(min(H, W) / 256))                      # Python's round: half to even


def to_tensor_01(x, dtype=torch.float64):
    """_to_tensor_01, metrics/mse.py:112-134 -> [T,C,H,W] in [0,1]"""
    is_tensor = isinstance(x, torch.Tensor)
    t = (x if is_tensor else torch.from_numpy(np.ascontiguousarray(x))).to(dtype)
    if t.ndim == 3:
        t = t.unsqueeze(0)
    if t.shape[-1] == 3:
        t = t.permute(0, 3, 1, 2)
    if is_tensor and t.min() < 0:
        t = (t + 1.0) / 2.0
    elif t.max() > 1.0:
        t = t / 255.0
    return t.contiguous()


def ssim_restated(gt, rep, downsample=True, dtype=torch.float64, sigma=1.5, size=11, k1=0.01, k2=0.03):
    """-> per-frame SSIM [T] in `dtype`, computed on the CPU with plain avg_pool2d / conv2d(groups=C)."""
    x, y = to_tensor_01(gt, dtype), to_tensor_01(rep, dtype)
    C = x.shape[1]
    f = ssim_factor(x.shape[-2], x.shape[-1]) if downsample else 1
    if f > 1:
        x, y = F.avg_pool2d(x, kernel_size=f), F.avg_pool2d(y, kernel_size=f)
    c = torch.arange(size, dtype=dtype) - (size - 1) / 2.0
    g = torch.exp(-(c[:, None] ** 2 + c[None, :] ** 2) / (2 * sigma ** 2))
    g = (g / g.sum()).expand(C, 1, size, size).contiguous()
    c1, c2 = k1 ** 2, k2 ** 2
    mu_x, mu_y = F.conv2d(x, g, groups=C), F.conv2d(y, g, groups=C)
    mu_xx, mu_yy, mu_xy = mu_x * mu_x, mu_y * mu_y, mu_x * mu_y
    s_xx = F.conv2d(x * x, g, groups=C) - mu_xx
    s_yy = F.conv2d(y * y, g, groups=C) - mu_yy
    s_xy = F.conv2d(x * y, g, groups=C) - mu_xy
    cs = (2.0 * s_xy + c2) / (s_xx + s_yy + c2)
    ss = (2.0 * mu_xy + c1) / (mu_xx + mu_yy + c1) * cs
    return ss.mean(dim=(-1, -2)).mean(dim=1)


def smooth_pair(T, C, H, W, seed):
    """gt: a smooth random image in [0,1]; rep: the same plus noise with ~10 % of the pixels zeroed (a reprojection with holes)."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(T, C, max(2, H // 8 + 1), max(2, W // 8 + 1), generator=g)
    gt = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True).clamp(0, 1)
    rep = (gt + 0.03 * torch.randn(T, C, H, W, generator=g)).clamp(0, 1)
    rep = rep * (torch.rand(T, 1, H, W, generator=g) > 0.10)
    return gt.contiguous(), rep.contiguous()


# ---------------------------------------------------------------- tests
def test_public_surface():
    from videogpa_amd.scorer import Metric, SSIMMetric, ssim
    m = SSIMMetric()
    assert m.name == "ssim" and isinstance(m, Metric) and callable(ssim)
    assert SSIMMetric(device="cuda").device == "cuda"
    assert hasattr(m, "compute_device")


def test_cabi_declares_ssim_entries():
    from videogpa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "videogpa_hip.h")).read()
    for name in ("vgpa_frame_ssim", "vgpa_frame_ssim_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["vgpa_frame_ssim"][1]) == 18
    # host-only query: one fp64 partial per (frame, channel, 32 x 24 tile) at full resolution + the four range words
    assert _lib.query("vgpa_frame_ssim_workspace_bytes", 10, 3, 518, 518) == 10 * 3 * 16 * 22 * 8 + 16
    assert _lib.query("vgpa_frame_ssim_workspace_bytes", 1, 1, 11, 11) == 8 + 16


def test_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from videogpa_amd.scorer import SSIMMetric, ssim
    a = torch.rand(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SSIMMetric().compute(gt=a, rep=a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ssim(a.numpy(), a.numpy(), reduction="none")


def test_restatement_downsample_factor_is_half_to_even():
    table = {256: 1, 294: 1, 383: 1, 384: 2, 518: 2, 640: 2, 641: 3}
    for side, f in table.items():
        assert ssim_factor(side, side + 100) == f and ssim_factor(side + 7, side) == f, side


def test_restatement_identical_images_give_exactly_one():
    gt, _ = smooth_pair(2, 3, 40, 52, seed=0)
    for dt in (torch.float64, torch.float32):
        assert torch.equal(ssim_restated(gt, gt.clone(), dtype=dt), torch.ones(2, dtype=dt))
    u8 = (gt * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(ssim_restated(u8, u8.numpy()), torch.ones(2, dtype=torch.float64))


def test_restatement_inputs_do_not_saturate_and_forms_agree():
    gt, rep = smooth_pair(2, 3, 64, 80, seed=1)
    v = ssim_restated(gt, rep)
    assert v.shape == (2,) and 0.35 < float(v.min()) and float(v.max()) < 0.78, v
    # the same pictures through the other input forms of _to_tensor_01
    assert torch.allclose(ssim_restated(gt * 2 - 1, rep * 2 - 1), v, atol=1e-12)
    assert torch.allclose(ssim_restated(gt.permute(0, 2, 3, 1).numpy(), rep), v, atol=1e-6)
    assert torch.allclose(ssim_restated(gt[0], rep[0]), v[:1], atol=1e-12)
    # fp32 against float64: the yardstick of the GPU tolerance
    assert float((ssim_restated(gt, rep, dtype=torch.float32).double() - v).abs().max()) < 5e-6
