"""LPIPS-VGG on the device: the kernels of csrc/lpips.hip, videogpa_amd.lpips.LPIPS and its place in the scorer.  -m gpu only.

The accuracy convention is tests/test_gpu_vggt_heads.py's: error = max-abs difference over max-abs of the float64 answer (tests/lpips_ref.py, a
restatement of upstream lpips 0.1), bound 8 x d32 with d32 that same distance for the fp32 torch evaluation on the CPU.  A scalar output (per-layer values,
totals, metric values) is one fp32 number, so half an ulp is its own floor: its bound is max(8 d32, 8 * 2^-24).  Every check prints `name err d32 ratio`
before it asserts.  Max pooling, ReLU, the zero channels and every determinism statement are exact (torch.equal).  The layer kernel's known answers
(2, 0, exactly 0) do not rest on the restatement."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R

pytestmark = pytest.mark.gpu
MARGIN = 8.0
FLOOR = 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops
    return ops


@pytest.fixture(scope="module")
def net(ops):
    from videogpa_amd.lpips import LPIPS
    m = LPIPS(net="vgg", pretrained=False, pnet_rand=True, frames_chunk=3)
    m.load_state_dict(R.state())
    return m.cuda()


def check(name, got, want64, ref32, scalar=False):
    err, d32 = R.rel_err(got, want64), R.rel_err(ref32, want64)
    bound = max(MARGIN * d32, FLOOR) if scalar else MARGIN * d32
    print(f"{name}: err {err:.3e} d32 {d32:.3e} ratio {err / d32 if d32 > 0 else float('nan'):.2f}{' (floor 4.8e-07)' if scalar else ''}")
    assert np.isfinite(err) and err <= bound, (name, err, d32)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------- input kernel
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 3, 37, 41)])
def test_input_scaling_and_layout(ops, shape):
    g = torch.Generator().manual_seed(shape[2])
    x = torch.rand(shape, generator=g) * 2 - 1
    shift, scale = torch.tensor(ops.LPIPS_SHIFT)[None, :, None, None], torch.tensor(ops.LPIPS_SCALE)[None, :, None, None]
    got = ops.lpips_input_f32(x.cuda())
    assert got.shape == (shape[0], shape[2], shape[3], 16)
    assert float(got[..., 3:].abs().max()) == 0.0                                          # the padding channels are exactly zero
    check(f"lpips_input {shape}", got[..., :3].permute(0, 3, 1, 2), (x.double() - shift.double()) / scale.double(), (x - shift) / scale)
    x01 = torch.rand(shape, generator=g)
    got = ops.lpips_input_f32(x01.cuda(), normalize=True)
    check(f"lpips_input normalize {shape}", got[..., :3].permute(0, 3, 1, 2), (2 * x01.double() - 1 - shift.double()) / scale.double(),
          (2 * x01 - 1 - shift) / scale)
    half = torch.full((2 * shape[0], shape[2], shape[3], 16), 7.0, device="cuda")          # the two halves of one batch
    ops.lpips_input_f32(x.cuda(), out=half[shape[0]:])
    assert torch.equal(half[shape[0]:], ops.lpips_input_f32(x.cuda())) and float((half[:shape[0]] - 7).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 7, 64), (1, 2, 2, 16), (2, 37, 41, 128)])
def test_maxpool_is_exact(ops, shape, relu):
    N, H, W, C = shape
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(H + C))
    want = F.max_pool2d(F.relu(x) if relu else x, 2, 2)                                    # odd sizes: the last row / column is dropped
    got = ops.maxpool2x2_f32(nhwc(x).cuda(), relu=relu)
    assert got.shape == (N, H // 2, W // 2, C)
    assert torch.equal(got.cpu(), nhwc(want))


# ---------------------------------------------------------------------------------------------------------------- layer kernel
def test_layer_known_answers(ops):
    C = 64
    e0, e1 = torch.zeros(1, 2, 2, C), torch.zeros(1, 2, 2, C)
    e0[..., 0], e1[..., 1] = 1.0, 1.0
    one = torch.ones(C)
    v = float(ops.lpips_layer_f32(e0.cuda(), e1.cuda(), one.cuda())[0])                    # orthogonal unit vectors: |e0 - e1|^2 = 2
    print(f"lpips_layer e0 vs e1: {v!r}")
    assert abs(v - 2.0) <= 2.0 ** -22                                                      # one ulp of 2
    v = float(ops.lpips_layer_f32((3 * e0).cuda(), (4 * e0).cuda(), one.cuda())[0])        # scale invariance
    print(f"lpips_layer 3 e0 vs 4 e0: {v!r}")
    assert abs(v) <= 1e-9
    g = torch.Generator().manual_seed(0)
    for shape in ((2, 3, 5, 128), (1, 33, 31, 256)):
        f = torch.randn(shape, generator=g).cuda()
        w = torch.rand(shape[-1], generator=g).cuda()
        for relu in (False, True):
            assert float(ops.lpips_layer_f32(f, f.clone(), w, relu=relu).abs().max()) == 0.0   # identical maps: exactly 0.0


def test_layer_all_negative_pixels_contribute_zero(ops):
    g = torch.Generator().manual_seed(1)
    f0, f1 = torch.randn(2, 3, 5, 128, generator=g), torch.randn(2, 3, 5, 128, generator=g)
    w = torch.rand(128, generator=g)
    f0[0, 1, 2], f1[0, 1, 2] = -f0[0, 1, 2].abs() - 0.1, -f1[0, 1, 2].abs() - 0.1           # all negative in both maps: zero after the ReLU
    z0, z1 = f0.clone(), f1.clone()
    z0[0, 1, 2], z1[0, 1, 2] = 0.0, 0.0
    got = ops.lpips_layer_f32(f0.cuda(), f1.cuda(), w.cuda(), relu=True)
    assert bool(torch.isfinite(got).all()) and float(got.min()) > 0
    assert torch.equal(got, ops.lpips_layer_f32(z0.cuda(), z1.cuda(), w.cuda(), relu=True))
    neg = -torch.rand(1, 4, 4, 64, generator=g) - 0.1
    assert float(ops.lpips_layer_f32(neg.cuda(), (2 * neg).cuda(), w[:64].cuda(), relu=True)[0]) == 0.0   # 0 / (0 + 1e-10) = 0, not NaN


# (1,300,301,64): 353 workgroups, a pixel count that is no multiple of any tile (256 pixels per workgroup at C = 64)
@pytest.mark.parametrize("shape", [(2, 1, 1, 64), (2, 3, 5, 128), (3, 9, 7, 512), (1, 33, 31, 256), (1, 300, 301, 64)])
def test_layer_random_maps(ops, shape):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(H * W + C)
    f0, f1 = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
    w = 0.01 * torch.rand(1, C, 1, 1, generator=g)
    a, b, wd = nhwc(f0).cuda(), nhwc(f1).cuda(), w.reshape(-1).cuda()
    total = torch.full((N,), 5.0, dtype=torch.float64, device="cuda")
    got = ops.lpips_layer_f32(a, b, wd, relu=True, total=total)
    want64 = R.layer(F.relu(f0.double()), F.relu(f1.double()), w)
    check(f"lpips_layer {shape}", got, want64, R.layer(F.relu(f0), F.relu(f1), w), scalar=True)
    assert torch.equal(total.float(), got)                                                 # `total` is the same value before its rounding ...
    first = total.clone()
    ops.lpips_layer_f32(a, b, wd, relu=True, total=total, accumulate=True)
    assert torch.equal(total, 2 * first)                                                   # ... and accumulates in fp64 (x + x is exact)
    assert torch.equal(got, ops.lpips_layer_f32(a, b, wd, relu=True))                      # run to run
    if N > 1:                                                                              # a frame's value does not depend on N
        each = torch.cat([ops.lpips_layer_f32(a[i:i + 1], b[i:i + 1], wd, relu=True) for i in range(N)])
        assert torch.equal(got, each)


# ---------------------------------------------------------------------------------------------------------------- whole network
# (3,3,16,16): 1 x 1 at slice 5; (2,3,35,29): odd at every pooling level; (2,3,70,61): 134 convolution workgroups at slice 1
@pytest.mark.parametrize("shape", R.NET_CASES)
def test_network_against_float64(net, shape):
    c = R.net_case(shape)
    gt, rep = c["gt"].cuda(), c["rep"].cuda()
    feats = net.features(gt)
    for k, f in enumerate(feats):
        assert f.shape == nhwc(c["feat64"][k]).shape
        check(f"LPIPS features {shape} slice {k + 1}", f.permute(0, 3, 1, 2), c["feat64"][k], c["feat32"][k])
    val, per = net(gt, rep, retPerLayer=True)
    assert val.shape == (shape[0], 1, 1, 1) and val.dtype == torch.float32 and len(per) == 5 and all(p.shape == (shape[0], 1, 1, 1) for p in per)
    check(f"LPIPS per-layer {shape}", torch.stack([p.reshape(-1) for p in per], dim=1), torch.stack(c["per64"], dim=1), torch.stack(c["per32"], dim=1),
          scalar=True)
    check(f"LPIPS total {shape}", val.reshape(-1), c["val64"], c["val32"], scalar=True)
    assert torch.equal(net(gt, rep), val)


@pytest.mark.parametrize("shape", R.NET_CASES)
def test_network_exact_properties(net, shape):
    c = R.net_case(shape)
    gt, rep = c["gt"].cuda(), c["rep"].cuda()
    assert net.frames_chunk == 3
    val3, per3 = net(gt, rep, retPerLayer=True)
    try:
        net.frames_chunk = 1
        val1, per1 = net(gt, rep, retPerLayer=True)
    finally:
        net.frames_chunk = 3
    assert torch.equal(val1, val3) and all(torch.equal(a, b) for a, b in zip(per1, per3))  # bit-equal for every frames_chunk
    assert float(net(gt, gt).abs().max()) == 0.0                                           # LPIPS(x, x) == 0 exactly
    # normalize=True maps [0,1] to [-1,1] by 2 x - 1.  On inputs on a 2^-8 grid (x + 1) / 2 and 2 y - 1 are exact in fp32, so both calls see the same numbers;
    # off such a grid (x + 1) / 2 itself rounds and the two calls legitimately see different inputs.
    q0, q1 = torch.round(gt * 256) / 256, torch.round(rep * 256) / 256
    assert torch.equal(net((q0 + 1) / 2, (q1 + 1) / 2, normalize=True), net(q0, q1))
    with pytest.raises(ValueError):
        net(gt, rep[:, :, :-1])
    with pytest.raises(RuntimeError, match="forward only"):
        net(gt.clone().requires_grad_(True), rep)


# ---------------------------------------------------------------------------------------------------------------- scorer
def test_scorer_metrics_with_the_native_network(net):
    """LPIPSMetric / Consistency_Score with the native network against oracle.scorer.lpips_metric / consistency_score around the restatement: uint8 NHWC numpy
    frames and a float NCHW `rep` of half the size, so the device resize runs and the network sees 20 x 24 pixels."""
    from oracle import scorer as osc
    from videogpa_amd import scorer as sc
    rng = np.random.default_rng(5)
    gt = rng.integers(0, 256, size=(3, 20, 24, 3), dtype=np.uint8)
    rep = torch.rand(3, 3, 10, 12, generator=torch.Generator().manual_seed(6))
    E = np.zeros((3, 3, 4), np.float32)
    for i in range(3):
        a = 0.1 * i
        E[i, :3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        E[i, :, 3] = [0.2 * i, -0.1 * i, 0.05 * i * i]
    n64, n32 = R.Net(R.state(), torch.float64), R.Net(R.state(), torch.float32)

    def scalar(name, got, want, ref32):
        err, d32 = abs(got - want) / abs(want), abs(ref32 - want) / abs(want)
        print(f"{name}: got {got!r} want {want!r} err {err:.3e} d32 {d32:.3e} ratio {err / d32 if d32 > 0 else float('nan'):.2f} (floor 4.8e-07)")
        assert np.isfinite(err) and err <= max(MARGIN * d32, FLOOR), (name, got, want, err, d32)
    with torch.no_grad():
        scalar("LPIPSMetric", sc.LPIPSMetric(device="cuda", lpips_net=net).compute(gt=gt, rep=rep), osc.lpips_metric(gt, rep, n64), osc.lpips_metric(gt, rep, n32))
        cs = sc.Consistency_Score(net, device="cuda")
        for ratio in (1, 0):
            got, motion = cs.compute(gt=gt, rep=rep, extrinsics=E, ratio=ratio)
            want, want_motion = osc.consistency_score(gt, rep, E, n64, ratio=ratio)
            scalar(f"Consistency_Score ratio={ratio}", got, want, osc.consistency_score(gt, rep, E, n32, ratio=ratio)[0])
            assert abs(motion - want_motion) <= 2e-6 * max(1.0, abs(want_motion))
