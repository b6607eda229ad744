"""SSIMMetric / scorer.ssim (csrc/scorer_ssim.hip) against the float64 restatement of piq.ssim in tests/test_ssim_host.py, run on the CPU.  -m gpu only.

Tolerance.  The yardstick is the distance d between the fp32 and the float64 run of the restatement on the same inputs (both on the CPU): the kernel is fp32 too
but sums the same terms in another order (separable window, pooling on load), so per case it gets FACTOR x d with an absolute floor of 4 fp32 ulps of 1.0
(4.8e-7).  FACTOR = 2, chosen from the first run on an MI355X: over the 35 comparisons below d was 1.3e-7 .. 2.8e-6 (largest for uint8 inputs and for the single
11 x 11 window, where nothing averages out) and the kernel's error 1.7e-9 .. 6.9e-7, at most 0.77 d (the single window; 0.25 d or less everywhere else) -- the
kernel is closer to float64 than the fp32 composition is, and 2 d leaves room for a different summation order without admitting anything else.  An error of the
semantics (window, pooling, constants, padding) shows up at 8e-4 or more on these inputs; every bound is asserted to stay below 1e-4."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import scorer as osc
from test_ssim_host import smooth_pair, ssim_restated

FACTOR = 2.0
FLOOR = 4 * 2.0 ** -23


@pytest.fixture(scope="module")
def sc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import scorer
    return scorer


def _tol(gt, rep, downsample=True):
    """-> (float64 per-frame reference, per-case bound)"""
    ref = ssim_restated(gt, rep, downsample=downsample)
    d = float((ssim_restated(gt, rep, downsample=downsample, dtype=torch.float32).double() - ref).abs().max())
    tol = max(FACTOR * d, FLOOR)
    assert tol < 1e-4, (d, tol)
    return ref, tol


def _check(sc, gt, rep, label, downsample=True):
    ref, tol = _tol(gt, rep, downsample)
    got = sc.ssim(gt, rep, downsample=downsample, reduction="none")
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
    err = float((got.double().cpu() - ref).abs().max())
    print(f"ssim[{label}] ref {float(ref.min()):.4f}..{float(ref.max()):.4f}  |err| {err:.3e}  bound {tol:.3e}  (fp32-fp64 distance {tol / FACTOR:.3e})")
    assert err <= tol, (label, err, tol, got.tolist(), ref.tolist())
    mean = sc.ssim(gt, rep, downsample=downsample)
    assert mean.dim() == 0 and abs(float(mean) - float(got.double().mean())) <= 2.0 ** -23, (float(mean), float(got.double().mean()))
    return got, ref


SHAPES = [(10, 3, 518, 518), (3, 3, 294, 518), (2, 3, 64, 80), (1, 3, 11, 11), (2, 3, 385, 385), (2, 1, 96, 120)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_vs_restatement(sc, shape):
    """the scorer's 10 x 518 x 518, no pooling + non-square, small, a single window, pooling that drops a trailing row / column, one channel"""
    T, C, H, W = shape
    gt, rep = smooth_pair(T, C, H, W, seed=H)
    got, ref = _check(sc, gt, rep, "x".join(map(str, shape)))
    assert 0.1 < float(ref.min()) and float(ref.max()) < 0.9                      # neither side saturates
    again = sc.ssim(gt, rep, reduction="none")
    assert torch.equal(got, again), "two runs on the same input differ"            # fixed-order reduction: bit-identical
    assert float(sc.ssim(gt, rep)) == float(sc.ssim(gt.cuda(), rep.cuda()))


@pytest.mark.parametrize("hw", [(64, 80), (390, 402)], ids=["64x80", "390x402_pooled"])
def test_every_input_form(sc, hw):
    """_to_tensor_01 (metrics/mse.py:112-134): f32 NCHW in [0,1] / [-1,1] / [0,255], uint8 NHWC tensor and numpy, a 3-D single frame, mixed pairs"""
    H, W = hw
    gt, rep = smooth_pair(2, 3, H, W, seed=7)
    gt8, rep8 = (gt * 255).round().to(torch.uint8), (rep * 255).round().to(torch.uint8)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    forms = {
        "f32_01": (gt, rep),
        "f32_pm1": (gt * 2 - 1, rep * 2 - 1),
        "f32_255": (gt * 255, rep * 255),
        "u8_nhwc_tensor": (nhwc(gt8), nhwc(rep8)),
        "u8_nhwc_numpy": (nhwc(gt8).numpy(), nhwc(rep8).numpy()),
        "f32_nhwc_numpy_01": (nhwc(gt).numpy(), nhwc(rep).numpy()),
        "single_frame_chw": (gt[0], rep[0]),
        "single_frame_hwc_u8": (nhwc(gt8)[0].numpy(), nhwc(rep8)[0].numpy()),
        "mixed_u8numpy_vs_pm1": (nhwc(gt8).numpy(), rep * 2 - 1),                      # what VideoProcessor passes: sampled frames vs reprojection
        "mixed_01_vs_u8tensor": (gt, nhwc(rep8)),
        "mixed_255_vs_u8_nchw": (gt * 255, rep8),
    }
    for name, (a, b) in forms.items():
        _check(sc, a, b, f"{H}x{W}:{name}")
    assert float(sc.SSIMMetric().compute(gt=nhwc(gt8).numpy(), rep=rep * 2 - 1)) == float(sc.ssim(nhwc(gt8).numpy(), rep * 2 - 1))


def test_downsample_switch(sc):
    gt, rep = smooth_pair(2, 3, 518, 518, seed=11)
    pooled, _ = _check(sc, gt, rep, "518:downsample")
    full, _ = _check(sc, gt, rep, "518:no_downsample", downsample=False)
    assert float((pooled - full).abs().min()) > 0.1                                 # pooling left out moves these inputs by ~0.4


def test_identical_inputs_and_metric_class(sc):
    gt, rep = smooth_pair(3, 3, 300, 280, seed=3)
    m = sc.SSIMMetric(device="cuda")
    assert isinstance(m, sc.Metric) and m.name == "ssim"
    assert abs(m.compute(gt=gt, rep=gt.clone()) - 1.0) <= FLOOR
    u8 = (gt * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert abs(m(gt=u8, rep=u8.numpy()) - 1.0) <= FLOOR
    dev = m.compute_device(gt=gt, rep=rep)
    assert dev.is_cuda and dev.dim() == 0
    v = m.compute(gt=gt, rep=rep, extrinsics=None)                                   # extra keywords are ignored, as in the reference
    assert isinstance(v, float) and v == float(dev)
    ref, tol = _tol(gt, rep)
    assert abs(v - float(ref.mean())) <= tol


def test_value_errors(sc):
    a = torch.rand(2, 3, 40, 48)
    with pytest.raises(ValueError):
        sc.ssim(a, torch.rand(2, 3, 40, 50))                                         # SSIM does not resize
    with pytest.raises(ValueError):
        sc.ssim(a, torch.rand(2, 3, 20, 24))
    with pytest.raises(ValueError):
        sc.ssim(a, torch.rand(3, 3, 40, 48))
    with pytest.raises(ValueError):
        sc.ssim(a, torch.rand(2, 1, 40, 48))
    with pytest.raises(ValueError):
        sc.ssim(torch.rand(1, 3, 10, 48), torch.rand(1, 3, 10, 48))                  # smaller than one window
    with pytest.raises(ValueError):
        sc.ssim(torch.rand(1, 1, 600, 10), torch.rand(1, 1, 600, 10), downsample=False)
    assert sc.ssim(torch.rand(1, 1, 600, 11), torch.rand(1, 1, 600, 11)).dim() == 0   # the factor comes from the SHORT side: no pooling here
    with pytest.raises(ValueError):
        sc.ssim(a, a, reduction="sum")
    with pytest.raises(ValueError):
        sc.SSIMMetric().compute(gt=a, rep=torch.rand(2, 3, 48, 40))


def _synthetic_predictions():
    """the stand-in backbone output of tests/test_gpu_scorer.py::test_video_processor_dispatch_matches_oracle_chain"""
    rng = np.random.default_rng(5)
    T, H, W = 4, 28, 36
    frames = (rng.random((T, H, W, 3)) * 255).astype(np.uint8)
    K = np.stack([np.array([[40.0 + t, 0, W / 2], [0, 42.0, H / 2], [0, 0, 1]], np.float32) for t in range(T)])
    E = np.stack([np.eye(4, dtype=np.float32) for _ in range(T)])
    for t in range(T):
        a = 0.03 * t
        E[t, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        E[t, :3, 3] = [0.05 * t, 0.0, 0.02 * t]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    depth = np.stack([2.0 + 0.3 * np.sin(xs / W * 3 + 0.2 * t) + 0.01 * rng.normal(size=(H, W)) for t in range(T)]).astype(np.float32)
    conf = (rng.random((T, H, W)) * 5).astype(np.float32)
    conf[0, 0, :4] = np.nan
    return T, H, W, frames, K, E, depth, conf


def test_video_processor_reports_ssim(sc):
    """SSIMMetric goes through the `else` branch of VideoProcessor.compute_metrics (pipelines/process_video.py:168-196) next to PSNR"""
    from types import SimpleNamespace
    from videogpa_amd.process_video import VideoProcessor
    T, H, W, frames, K, E, depth, conf = _synthetic_predictions()
    metrics = {"SSIM": sc.SSIMMetric(), "PSNR": sc.PSNRMetric()}
    world = osc.unproject_depth(depth, K, osc.affine_inverse(E)).numpy()
    images01 = torch.from_numpy(frames).float().div(255).permute(0, 3, 1, 2).contiguous()

    def expect(gt, th):
        v, c = osc.pointcloud_filter(world, conf, images01, th)
        rep = torch.from_numpy(osc.batch_reproject(v.numpy(), c.numpy(), K, E[:, :3], H, W))
        ref, tol = _tol(gt, rep)
        return float(ref.mean()), tol, osc.psnr(gt, rep)

    da3 = VideoProcessor(metrics, backbone_fn=lambda fl: SimpleNamespace(processed_images=frames, extrinsics=E[:, :3], intrinsics=K, depth=depth, conf=conf),
                         frame_sampler=lambda p, n: frames, backbone="da3")
    res = da3.process("video.mp4", thresholds=[0, 40], num_frames=T)
    preds = {"images": images01, "world_points_from_depth": torch.from_numpy(world), "depth_conf": torch.from_numpy(conf),
             "extrinsic": torch.from_numpy(E[:, :3]), "intrinsic": torch.from_numpy(K), "depth": torch.from_numpy(depth)}
    res2 = VideoProcessor(metrics, backbone_fn=lambda fr: preds, backbone="vggt").process(frames, thresholds=[0, 40], num_frames=T)
    for label, r, gt in (("da3", res, images01), ("vggt", res2, frames)):
        for th in (0, 40):
            assert set(r[th]) == {"SSIM", "PSNR"}
            want, tol, want_psnr = expect(gt, th)
            print(f"processor[{label}, thr {th}] SSIM {r[th]['SSIM']:.6f} ref {want:.6f} |err| {abs(r[th]['SSIM'] - want):.3e} bound {tol:.3e}")
            assert abs(r[th]["SSIM"] - want) <= tol, (label, th, r[th]["SSIM"], want)
            assert abs(r[th]["PSNR"] - float(want_psnr)) <= 2e-5 * max(1.0, abs(float(want_psnr)))
