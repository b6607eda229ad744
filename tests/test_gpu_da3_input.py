"""Depth Anything 3's input processing on the device (csrc/da3_input.hip, videogpa_amd/da3_input.py, da3.DepthAnything3).  -m gpu only.

cv2 is not a dependency of this project and its 8-bit result varies by build, so nothing below compares against it.  The kernels are bounded against what the
operations mean, with the oracles of tests/da3_input_ref.py (numpy float64 / int64, written from the definitions, not from the kernels):

  area, general path   with `a` the float64 evaluation of the tap table: the output equals rint(a) wherever |frac(a) - 0.5| > 1e-3 and lies in
                       {floor(a), ceil(a)} elsewhere.  1e-3: at most 32 fp32 products of values <= 255 err by less than 255 * 32 * 2^-24 ~ 5e-4.  The
                       samples given that latitude may be at most 5 % (40x60 and 56x90 -> 28x42), 1 % (37x53) and none (30x42): at ratio 10/7 the exact
                       values are multiples of 1/100, so exact ties are real there (observed on an MI355X: 3.1 %, 0.18 %, 3.3 %, 0; nothing wrong anywhere).
  area, integer path   exact: (sum + 2) >> 2 for 2 x 2, rint(sum / 9) for 3 x 3 (no tie exists at ninths).
  cubic                exactly the int64 restatement of the fixed-point scheme, AND within CUBIC_BOUND of the exact float64 A = -0.75 cubic
                       convolution (clipped to [0, 255]): eight weights (four per axis) each off by at most 2^-12 after fixing to 11 bits, times 255,
                       plus the 0.5 of the final rounding = 0.998 grey levels (observed 0.60-0.72).  A = -0.5 is 12-20 grey levels away on the random frame.
  last stage           x bit-identical to torch's ToTensor + Normalize in fp32; processed_images identical to the table lookup.
Every check prints its figures before it asserts.  The whole file takes a few seconds."""
import types

import numpy as np
import pytest
import torch

import da3_input_ref as R

pytestmark = pytest.mark.gpu
T = 3
TIE = 1e-3
CUBIC_BOUND = 8 * 2.0 ** -12 * 255 + 0.5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops
    return ops


@pytest.fixture(scope="module")
def table(ops):
    from videogpa_amd import da3_input
    return torch.from_numpy(da3_input.processed_table()).cuda()


_FRAMES = {}


def frames(H, W):
    if (H, W) not in _FRAMES:
        _FRAMES[H, W] = R.frames(T, H, W, seed=H * 1000 + W)
    return _FRAMES[H, W]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_area(name, got, a, max_share):
    """got uint8, a float64 of the same shape -> the share of samples within TIE of a tie"""
    got = got.astype(np.float64)
    lat = np.abs(a - np.floor(a) - 0.5) <= TIE
    strict_bad = int((got[~lat] != np.rint(a[~lat])).sum())
    lat_bad = int(((got[lat] != np.floor(a[lat])) & (got[lat] != np.ceil(a[lat]))).sum())
    share = float(lat.mean())
    print(f"{name}: max |out - a| {np.abs(got - a).max():.4f}, {share:.2%} of samples within {TIE} of a tie (limit {max_share:.0%}), "
          f"{strict_bad} wrong away from ties, {lat_bad} wrong at ties")
    assert strict_bad == 0 and lat_bad == 0 and share <= max_share, name
    return share


def check_cubic(name, got, src, out_h, out_w):
    fixed, exact = R.cubic_fixed(src, out_h, out_w), np.clip(R.cubic_exact(src, out_h, out_w), 0, 255)
    err = float(np.abs(got.astype(np.float64) - exact).max())
    off = float(np.abs(got[:1].astype(np.float64) - np.clip(R.cubic_exact(src[:1], out_h, out_w, A=-0.5), 0, 255)).max())       # frame 0 is the random one
    print(f"{name}: {int((got != fixed).sum())} samples differ from the int64 restatement; max distance from the float64 cubic {err:.4f} "
          f"(bound {CUBIC_BOUND:.4f}); from an A = -0.5 cubic on the random frame {off:.1f}")
    assert np.array_equal(got, fixed) and err <= CUBIC_BOUND, name
    return off


# ------------------------------------------------------------------------------------------------------------------------ 1. area
@pytest.mark.parametrize("src,share", [((40, 60), 0.05), ((37, 53), 0.01), ((56, 90), 0.05), ((30, 42), 0.0)])
def test_area_general_path(ops, src, share):
    f = frames(*src)
    got = ops.da3_resize(dev(f), 28, 42, "area").cpu().numpy()
    assert got.shape == (T, 28, 42, 3) and got.dtype == np.uint8
    check_area(f"area {src} -> (28, 42)", got, R.area_exact(f, 28, 42), share)


def test_area_integer_path(ops):
    f = frames(56, 84)
    got = ops.da3_resize(dev(f), 28, 42, "area").cpu().numpy()
    want = (R.box_sum(f, 28, 42) + 2) >> 2
    print(f"area 2 x 2: {int((got != want).sum())} samples differ from (sum + 2) >> 2")
    assert np.array_equal(got, want)
    f = frames(84, 126)
    got = ops.da3_resize(dev(f), 28, 42, "area").cpu().numpy()
    want = np.rint(R.box_sum(f, 28, 42) / 9.0)
    print(f"area 3 x 3: {int((got != want).sum())} samples differ from rint(sum / 9)")
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------------ 2. cubic
@pytest.mark.parametrize("src,dst", [((27, 50), (28, 50)), ((20, 31), (28, 42))])
def test_cubic(ops, src, dst):
    f = frames(*src)
    got = ops.da3_resize(dev(f), dst[0], dst[1], "cubic").cpu().numpy()
    assert got.shape == (T, dst[0], dst[1], 3)
    off = check_cubic(f"cubic {src} -> {dst}", got, f, *dst)
    assert off > 10 * CUBIC_BOUND                      # the bound has teeth: another A does not pass it


# ------------------------------------------------------------------------------------------------------------------------ 3. other kernel checks
def test_constant_frames_stay_constant_and_area_refuses_to_upscale(ops):
    for H, W, oh, ow, mode in ((40, 60, 28, 42, "area"), (37, 53, 28, 42, "area"), (56, 84, 28, 42, "area"), (84, 126, 28, 42, "area"),
                               (20, 31, 28, 42, "cubic"), (27, 50, 28, 50, "cubic"), (40, 60, 28, 42, "cubic")):
        f = np.zeros((2, H, W, 3), np.uint8)
        f[0] = 255
        got = ops.da3_resize(dev(f), oh, ow, mode).cpu().numpy()
        assert (got[0] == 255).all() and (got[1] == 0).all(), (H, W, oh, ow, mode)
    x = dev(frames(40, 60))
    for oh, ow in ((41, 60), (40, 61), (28, 61)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.da3_resize(x, oh, ow, "area")
    with pytest.raises(RuntimeError, match="mode is one of"):
        ops.da3_resize(x, 28, 42, "linear")


def lookup(table, u8):
    """processed_images by the table: u8 numpy [T,h,w,3]"""
    t = table.cpu().numpy()
    return np.stack([t[c][u8[..., c]] for c in range(3)], axis=-1)


@pytest.mark.parametrize("box", [None, (3, 5, 28, 42), (0, 0, 14, 14), (12, 18, 28, 42)])
def test_fused_last_stage(ops, table, box):
    f = frames(40, 60)
    x, proc = ops.da3_normalize(dev(f), table, box)
    top, left, h, w = box or (0, 0, 40, 60)
    crop = f[:, top:top + h, left:left + w]
    want = R.normalize(crop)
    assert x.shape == (1, T, 3, h, w) and x.dtype == torch.float32 and proc.shape == (T, h, w, 3) and proc.dtype == torch.uint8
    print(f"last stage box {box}: {int((x.cpu() != want).sum())} values of x differ from torch's ToTensor + Normalize, "
          f"{int((proc.cpu().numpy() != lookup(table, crop)).sum())} of processed_images from the table")
    assert torch.equal(x.cpu(), want)
    assert np.array_equal(proc.cpu().numpy(), lookup(table, crop)) and np.array_equal(proc.cpu().numpy(), R.processed_images(want))
    if box is not None:
        for bad in ((-1, 0, 10, 10), (0, 0, 41, 60), (0, 30, 40, 31)):
            with pytest.raises(RuntimeError, match="invalid argument"):
                ops.da3_normalize(dev(f), table, bad)


@pytest.mark.parametrize("src,dst,mode", [((40, 60), (28, 42), "area"), ((56, 84), (28, 42), "area"), ((84, 126), (28, 42), "area"),
                                          ((20, 31), (28, 42), "cubic")])
def test_last_stage_as_the_resize_epilogue(ops, table, src, dst, mode):
    f = dev(frames(*src))
    u8 = ops.da3_resize(f, dst[0], dst[1], mode).cpu().numpy()
    x, proc = ops.da3_resize(f, dst[0], dst[1], mode, table=table)
    assert x.shape == (1, T, 3) + dst and torch.equal(x.cpu(), R.normalize(u8)) and np.array_equal(proc.cpu().numpy(), lookup(table, u8))


# ------------------------------------------------------------------------------------------------------------------------ 4. InputProcessor
def check_stage(ops, name, cur, st):
    """one resize stage of the reference's walk on the device's own previous image -> the device's next image (numpy), checked against the oracles"""
    got = ops.da3_resize(dev(cur), st[1], st[2], st[0]).cpu().numpy()
    if st[0] == "area":
        check_area(name, got, R.area_exact(cur, st[1], st[2]), 0.05)
    else:
        check_cubic(name, got, cur, st[1], st[2])
    return got


@pytest.mark.parametrize("method", ["upper_bound_resize", "upper_bound_crop", "lower_bound_resize", "lower_bound_crop"])
@pytest.mark.parametrize("size", [(50, 75), (75, 50)])
def test_input_processor(ops, table, size, method):
    from videogpa_amd.da3_input import InputProcessor
    H, W = size
    f = frames(H, W)
    K = np.stack([np.array([[90.0 + i, 0, W / 2.0], [0, 80.0, H / 2.0 + i], [0, 0, 1]], np.float32) for i in range(T)])
    E = np.stack([np.eye(4, dtype=np.float32) * (i + 1) for i in range(T)])
    x, ext, ixt, proc = InputProcessor().process(list(f), E, K, 56, method)
    stages, (h, w), _ = R.process_one(H, W, None, 56, method)
    cur = f
    for k, st in enumerate(stages):
        cur = cur[:, st[1]:st[1] + st[3], st[2]:st[2] + st[4]] if st[0] == "crop" else check_stage(ops, f"{size} {method} stage {k} {st}", cur, st)
    assert cur.shape == (T, h, w, 3) and h % 14 == 0 and w % 14 == 0 and x.shape == (1, T, 3, h, w) and x.is_cuda and proc.shape == (T, h, w, 3)
    assert torch.equal(x.cpu(), R.normalize(cur)) and np.array_equal(proc.cpu().numpy(), lookup(table, cur))
    want_k = np.stack([R.process_one(H, W, K[i], 56, method)[2] for i in range(T)])
    assert ixt.dtype == torch.float32 and np.array_equal(ixt.numpy(), want_k) and np.array_equal(ext.numpy(), E)
    x2, e2, k2 = InputProcessor()(dev(f), process_res=56, process_res_method=method)                # one device tensor, no cameras: the same pixels
    assert torch.equal(x2, x) and e2 is None and k2 is None


def test_input_processor_groups_mixed_sizes(ops, table):
    """frames of two sizes in one call: grouped by size, one batch of launches each, then `_unify_batch_shapes`' centre crop to the smallest"""
    from videogpa_amd.da3_input import InputProcessor
    a, b = frames(50, 75), frames(75, 50)
    K = np.stack([np.array([[90.0, 0, 30.0 + i], [0, 80.0, 20.0], [0, 0, 1]], np.float32) for i in range(4)])
    clip, sizes = [a[0], b[0], a[1], b[1]], [(50, 75), (75, 50), (50, 75), (75, 50)]
    x, _, ixt, proc = InputProcessor().process(clip, None, K, 56, "upper_bound_resize")
    ones = [R.process_one(h, w, K[i], 56, "upper_bound_resize") for i, (h, w) in enumerate(sizes)]
    crops, (mh, mw), want_k = R.unify([o[1] for o in ones], [o[2] for o in ones])
    assert (mh, mw) == (42, 42) and x.shape == (1, 4, 3, 42, 42) and np.array_equal(ixt.numpy(), np.stack(want_k))
    xa, _, _, pa = InputProcessor().process(a[:2], None, None, 56, "upper_bound_resize")           # each size alone, cropped by hand
    xb, _, _, pb = InputProcessor().process(b[:2], None, None, 56, "upper_bound_resize")
    for i, (src, pr, j) in enumerate(((xa, pa, 0), (xb, pb, 0), (xa, pa, 1), (xb, pb, 1))):
        top, left = crops[i]
        assert torch.equal(x[0, i], src[0, j, :, top:top + 42, left:left + 42]) and torch.equal(proc[i], pr[j, top:top + 42, left:left + 42])


# ------------------------------------------------------------------------------------------------------------------------ 5. end to end
def api_model(**kw):
    from test_gpu_dualdpt import small_net
    from videogpa_amd.da3 import DepthAnything3
    return DepthAnything3(model=small_net(), **kw)


def test_inference_takes_frames_of_any_size(ops, table):
    api = api_model()
    f = R.frames(4, 40, 60, seed=11)
    pred = api.inference([f[i] for i in range(4)], process_res=42)
    u8 = ops.da3_resize(dev(f), 28, 42, "area").cpu().numpy()
    assert pred.depth.shape == pred.conf.shape == (4, 28, 42) and pred.depth.is_cuda and pred.extrinsics.shape == (4, 3, 4) and pred.intrinsics.shape == (4, 3, 3)
    assert bool(torch.isfinite(pred.depth).all()) and bool(torch.isfinite(pred.conf).all()) and bool((pred.depth > 0).all())
    assert pred.processed_images.dtype == torch.uint8 and np.array_equal(pred.processed_images.cpu().numpy(), lookup(table, u8))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = api.model(R.normalize(u8).cuda(), aux=False)                                          # the bare network on the hand-normalised frames
    assert torch.equal(out["depth"][0], pred.depth) and torch.equal(out["depth_conf"][0], pred.conf) and torch.equal(out["extrinsics"][0], pred.extrinsics)
    again = api.inference(dev(f), process_res=42, process_res_method="upper_bound_crop")            # a device tensor; the same plan by another method
    assert torch.equal(again.depth, pred.depth)


def test_video_processor_scores_frames_of_any_size(ops, table):
    from videogpa_amd import scorer as sc
    from videogpa_amd.process_video import VideoProcessor
    api = api_model(process_res=42)                  # VideoProcessor calls inference(frames) bare, as upstream: the processing size is the instance's
    f = R.frames(4, 40, 60, seed=11)
    metrics = {"mse": sc.MSEMetric(), "MVCS": sc.MVCSMetric()}
    res = VideoProcessor(metrics, backbone="da3", da3_model=api).process(f, thresholds=[0, 40], num_frames=4)
    # the same clip resized with ops, normalised by hand and run through the bare network, scored through the existing backbone_fn path
    u8 = ops.da3_resize(dev(f), 28, 42, "area").cpu().numpy()
    x = R.normalize(u8)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = api.model(x.cuda(), aux=False)
    pred = types.SimpleNamespace(processed_images=R.processed_images(x), depth=out["depth"][0], conf=out["depth_conf"][0],
                                 extrinsics=out["extrinsics"][0], intrinsics=out["intrinsics"][0])
    ref = VideoProcessor(metrics, backbone="da3", backbone_fn=lambda fl: pred).process(f, thresholds=[0, 40], num_frames=4)
    assert set(res) == {0, 40, "_extrinsic"} and res["_extrinsic"] == ref["_extrinsic"]
    for th in (0, 40):
        print(f"VideoProcessor(DepthAnything3) on 40 x 60 frames, threshold {th}: {res[th]}; bare network on the pre-resized frames: {ref[th]}")
        assert set(res[th]) == {"mse", "MVCS"} and all(isinstance(v, float) and np.isfinite(v) for v in res[th].values()) and res[th] == ref[th]
    with pytest.raises(ValueError, match="multiples of 14.*DepthAnything3"):                        # the bare network keeps its path and its refusal
        VideoProcessor(metrics, backbone="da3", da3_model=api.model).process(f, thresholds=[0], num_frames=4)
