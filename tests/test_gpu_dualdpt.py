"""Depth Anything 3's DualDPT head and the whole DepthAnything3Net on the device (videogpa_amd/da3.py, csrc/dualdpt.hip).  -m gpu only.

Every accuracy bound is the one of tests/test_gpu_vggt_heads.py: err <= 8 x d32.  Error = max-abs difference over max-abs of the float64 answer; d32 =
that same distance for the fp32 torch evaluation of the same output (the restatement of tests/dualdpt_ref.py on the CPU, or the fp32 golden of the
reference module).  The arithmetic is of the same class (fp32 products, fp32 sums; the fp32 MFMA is a k-ordered fmaf chain) while the summation
order differs and the embedding / LayerNorm are fused.  Every test prints `name err d32 ratio` before it asserts.  What must be bit for bit is: the
result whatever the chunking, depth / depth_conf with and without the auxiliary branch, the network against its parts, and the cameras against
DA3Cameras'.

Observed err / d32 on an MI355X (also in DESIGN.md section 5e): auxiliary tail 0.38-1.22 at C = 16, 1.67-3.38 at C = 128; zero-variance pixels within 4e-8 of the
LayerNorm-bias path on the rays and 1.5e-7 on the confidence logit (bounds 2-4e-6); head against golden (A) 0.44-0.99, (B) 1.06-1.36; without embedding, patch_start_idx = 2:
0.87-1.56; full width 1.36 / 2.20 / 2.12 / 1.86 (depth, depth_conf, ray, ray_conf); head on backbone features 0.35-1.02.  The whole file takes 4 s."""
import os

import numpy as np
import pytest
import torch

import da3_ref as D
import dinov2_ref
import dualdpt_ref as R
from test_dualdpt_host import GOLDEN, load_case, load_golden

pytestmark = pytest.mark.gpu
MARGIN = 8.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops
    return ops


def check(name, got, want64, ref32):
    err, d32 = R.rel(got, want64), R.rel(ref32, want64)
    ratio = err / d32 if d32 > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{name}: err {err:.3e} d32 {d32:.3e} ratio {ratio:.2f}")
    assert np.isfinite(err) and err <= MARGIN * d32, (name, err, d32)
    return ratio


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------------------------------ 1. the auxiliary tail
def tail_state(C, od, seed, const_b1=None):
    g = torch.Generator().manual_seed(seed)
    p = "t.0"
    return {p + ".0.weight": torch.randn(32, C, 3, 3, generator=g) / (9 * C) ** 0.5,
            p + ".0.bias": torch.randn(32, generator=g) if const_b1 is None else torch.full((32,), const_b1),
            p + ".2.weight": 1.0 + 0.2 * torch.randn(32, generator=g), p + ".2.bias": 0.3 * torch.randn(32, generator=g),
            p + ".5.weight": torch.randn(od, 32, 1, 1, generator=g) * 0.4, p + ".5.bias": torch.randn(od, generator=g)}


def run_tail(ops, sd, x, aspect, embed):
    """x NCHW on the CPU -> (preds, conf) of the kernel"""
    N, C, h, w = x.shape
    with torch.no_grad():
        return ops.dualdpt_aux_tail_f32(nhwc(x).cuda(), ops.pack_conv_weight(sd["t.0.0.weight"]).cuda(), sd["t.0.0.bias"].cuda(), sd["t.0.2.weight"].cuda(),
                                        sd["t.0.2.bias"].cuda(), 1e-5, sd["t.0.5.weight"].flatten(1).contiguous().cuda(), sd["t.0.5.bias"].cuda(),
                                        tabs=ops.uv_embed_tables(w, h, C, aspect, "cuda", f32_angles=True) if embed else None)


@pytest.mark.parametrize("embed", [False, True])
@pytest.mark.parametrize("hw", [(5, 7), (24, 32)])            # 70 pixels: one partial 128-pixel tile; 1536 pixels: twelve full tiles over two frames
@pytest.mark.parametrize("C", [16, 128])
def test_aux_tail_vs_restatement(ops, C, hw, embed):
    N, od, aspect = 2, 7, 56 / 42
    x = torch.randn(N, C, *hw, generator=torch.Generator().manual_seed(C + hw[0]))
    sd = tail_state(C, od, seed=C + hw[1])
    ref = lambda dt: R.aux_tail({k: v.to(dt) for k, v in sd.items()}, x.to(dt), aspect, level=0, pos_embed=embed, prefix="t.")
    (p64, c64), (p32, c32) = ref(torch.float64), ref(torch.float32)
    p, c = run_tail(ops, sd, x, aspect, embed)
    assert p.shape == (N, *hw, od - 1) and c.shape == (N, *hw) and p.dtype == c.dtype == torch.float32
    check(f"aux tail C={C} {hw} embed={embed} preds", p, p64, p32)
    check(f"aux tail C={C} {hw} embed={embed} conf", c, c64, c32)


def test_aux_tail_zero_variance_pixels(ops):
    """frame 0 is zero and there is no embedding, so its hidden values are the constant bias in all 32 channels: variance 0.  The kernel sums pairwise, so
    the mean is exact, the centred values are 0 and the output is w2 . relu(ln_b) + b2 at every pixel: finite, identical across the frame, and within
    the rounding of a 32-term fp32 dot product (32 x 2^-24 x sum |terms|) of the float64 value.  Frame 1 is ordinary and checked as above."""
    C, od, hw = 32, 7, (9, 11)
    x = torch.randn(2, C, *hw, generator=torch.Generator().manual_seed(3))
    x[0] = 0
    sd = tail_state(C, od, seed=4, const_b1=0.3)
    p, c = run_tail(ops, sd, x, 1.0, embed=False)
    p, c = p.cpu(), c.cpu()
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(c).all())
    w2, b2, hidden = sd["t.0.5.weight"].flatten(1).double(), sd["t.0.5.bias"].double(), torch.relu(sd["t.0.2.bias"].double())
    want = w2 @ hidden + b2
    bound = 32 * 2.0 ** -24 * ((w2.abs() @ hidden) + b2.abs())
    got = torch.cat([p[0, 4, 5], (c[0, 4, 5] - 1).log()[None]]).double()
    print("zero-variance pixel: |got - bias path|", (got - want).abs().tolist(), "bound", bound.tolist())
    assert bool(((got[:-1] - want[:-1]).abs() <= bound[:-1]).all())
    assert abs(float(c[0, 4, 5]) - float(1 + want[-1].exp())) <= float((1 + want[-1].exp()) * (bound[-1] + 2.0 ** -22))
    assert bool((p[0] == p[0, 4, 5]).all()) and bool((c[0] == c[0, 4, 5]).all())
    ref = lambda dt: R.aux_tail({k: v.to(dt) for k, v in sd.items()}, x.to(dt), 1.0, level=0, pos_embed=False, prefix="t.")
    (p64, c64), (p32, c32) = ref(torch.float64), ref(torch.float32)
    check("aux tail zero-variance frame + ordinary frame preds", p, p64, p32)
    check("aux tail zero-variance frame + ordinary frame conf", c, c64, c32)


def test_aux_tail_refusals(ops):
    z = lambda *s: torch.zeros(*s, device="cuda")
    good = dict(x=z(1, 5, 7, 16), w1_packed=z(3, 3, 16, 32), b1=z(32), ln_w=z(32), ln_b=z(32), eps=1e-5, w2=z(7, 32), b2=z(7))
    ops.dualdpt_aux_tail_f32(**good)
    for bad in (dict(w1_packed=z(3, 3, 16, 16)), dict(w2=z(7, 16)), dict(ln_w=z(16)), dict(b2=z(6)), dict(w2=z(9, 32), b2=z(9)),
                dict(tabs=(z(7, 8), z(6, 8))), dict(x=z(1, 5, 7, 24), w1_packed=z(3, 3, 24, 32))):
        with pytest.raises(RuntimeError, match="do not fit"):
            ops.dualdpt_aux_tail_f32(**{**good, **bad})


# ------------------------------------------------------------------------------------------------------------------------ 2. the head
_HEAD = {}


def golden_head():
    if "head" not in _HEAD:
        from videogpa_amd.da3 import DualDPT
        _, state = load_golden()
        head = DualDPT(**R.CFG)
        head.load_state_dict(state, strict=True)
        _HEAD["head"] = head.cuda().eval()
    return _HEAD["head"]


@pytest.mark.parametrize("name", list(R.CASES))
def test_head_matches_the_reference_goldens(ops, name):
    head, c = golden_head(), load_case(name)
    H, W = c["hw"]
    B, S = R.CASES[name][:2]
    feats = [(f.cuda(), None) for f in c["feats"]]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):           # the head computes in fp32 whatever autocast says
        out = head(feats, H, W, patch_start_idx=0)
        chunk2 = head(feats, H, W, patch_start_idx=0, chunk_size=2)
        chunk1 = head(feats, H, W, patch_start_idx=0, chunk_size=1)
        main = head(feats, H, W, patch_start_idx=0, aux=False)
    assert tuple(out) == R.OUTPUTS and out.depth is out["depth"]
    for k in R.OUTPUTS:
        assert out[k].shape == c["out64"][k].shape and out[k].dtype == torch.float32
        check(f"DualDPT golden {name} {k}", out[k], c["out64"][k], c["out32"][k])
        assert torch.equal(chunk2[k], out[k]) and torch.equal(chunk1[k], out[k]), k           # the result does not depend on the chunking
    assert tuple(main) == ("depth", "depth_conf")
    assert torch.equal(main["depth"], out["depth"]) and torch.equal(main["depth_conf"], out["depth_conf"])
    with pytest.raises(RuntimeError, match="forward only"):
        head(feats, H, W, patch_start_idx=0)


def test_head_with_leading_tokens_and_without_embedding(ops):
    """patch_start_idx > 0 drops the leading tokens; pos_embed=False takes the table-less path of every kernel"""
    from videogpa_amd.da3 import DualDPT
    _, state = load_golden()
    head = DualDPT(**R.CFG, pos_embed=False)
    head.load_state_dict(state, strict=True)
    head = head.cuda().eval()
    c = load_case("B")
    H, W = c["hw"]
    g = torch.Generator().manual_seed(8)
    feats = [torch.cat([torch.randn(*f.shape[:2], 2, f.shape[-1], generator=g), f], dim=2) for f in c["feats"]]
    with torch.no_grad():
        out = head([(f.cuda(), None) for f in feats], H, W, patch_start_idx=2)
        o64 = R.head({k: v.double() for k, v in state.items()}, [f.double() for f in feats], H, W, patch_start_idx=2, pos_embed=False)
        o32 = R.head(state, feats, H, W, patch_start_idx=2, pos_embed=False)
    for k in R.OUTPUTS:
        check(f"DualDPT no embedding, patch_start_idx=2 {k}", out[k], o64[k], o32[k])


def test_head_full_width(ops):
    """dim_in = 2048 and the default channels (DA3-Large's head) on one frame of 28 x 42: K = 9 x 1024 in resize_layers.3 / layer4_rn and the 2048-wide
    projection, against the float64 restatement"""
    from videogpa_amd.da3 import DualDPT
    head = DualDPT(2048)
    state = R.seeded_state({k: v.shape for k, v in head.state_dict().items()}, seed=31)
    head.load_state_dict(state, strict=True)
    head = head.cuda().eval()
    H, W = 28, 42
    feats = [torch.randn(1, 1, 6, 2048, generator=torch.Generator().manual_seed(40 + i)) for i in range(4)]
    with torch.no_grad():
        out = head([(f.cuda(), None) for f in feats], H, W, patch_start_idx=0)
        o32 = R.head(state, feats, H, W)
        o64 = R.head({k: v.double() for k, v in state.items()}, [f.double() for f in feats], H, W)
    assert out["depth"].shape == (1, 1, 28, 42) and out["ray"].shape == (1, 1, 16, 24, 6)
    for k in R.OUTPUTS:
        check(f"DualDPT full width {k}", out[k], o64[k], o32[k])


# ------------------------------------------------------------------------------------------------------------------------ 3. the network
def small_net():
    """da3_ref's configuration (a) with its seeded backbone and camera decoder (checked against the golden's sums), all four blocks tapped, and a seeded
    head of dim_in = 128, features = 32"""
    if "net" not in _HEAD:
        from test_dualdpt_host import small_net as build
        g = torch.load(os.path.join(GOLDEN, "da3_a.pt"))
        state, dec_state = D.seeded_state(g["shapes"], g["cfg"]["seed"]), D.cam_dec_state(g["cam_dec_shapes"], g["cfg"]["seed"])
        dinov2_ref.check_state_sums(state, g["sums"])
        dinov2_ref.check_state_sums(dec_state, g["cam_dec_sums"])
        net = build()
        net.backbone.pretrained.load_state_dict(state, strict=True)
        net.cam_dec.load_state_dict(dec_state, strict=True)
        net.head.load_state_dict(R.seeded_state({k: v.shape for k, v in net.head.state_dict().items()}, seed=32), strict=True)
        _HEAD["net"] = net.cuda().eval()
    return _HEAD["net"]


def test_network_is_its_parts(ops):
    from videogpa_amd.da3 import DA3Cameras
    net = small_net()
    x = D.images(100, 1, 4, (42, 56)).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = net(x)
        feats, _ = net.backbone(x)
        parts = net.head(feats, 42, 56, patch_start_idx=0)
        cams = DA3Cameras(net.backbone, net.cam_dec)(x)
        main = net(x, aux=False)
    assert set(out) == set(R.OUTPUTS) | {"extrinsics", "intrinsics"} and set(main) == {"depth", "depth_conf", "extrinsics", "intrinsics"}
    assert out.depth.shape == (1, 4, 42, 56) and out.ray.shape == (1, 4, 24, 32, 6) and out.extrinsics.shape == (1, 4, 3, 4) and out.intrinsics.shape == (1, 4, 3, 3)
    for k in R.OUTPUTS:
        assert out[k].dtype == torch.float32 and bool(torch.isfinite(out[k]).all()) and torch.equal(out[k], parts[k]), k
    for k in ("extrinsics", "intrinsics"):
        assert torch.equal(out[k], cams[k]) and torch.equal(main[k], cams[k]), k
    assert torch.equal(main["depth"], out["depth"]) and torch.equal(main["depth_conf"], out["depth_conf"])
    with torch.no_grad():
        o64 = R.head({k: v.double().cpu() for k, v in net.head.state_dict().items()}, [f.double().cpu() for f, _ in feats], 42, 56)
        o32 = R.head({k: v.cpu() for k, v in net.head.state_dict().items()}, [f.cpu() for f, _ in feats], 42, 56)
    for k in R.OUTPUTS:                                                           # the head on real backbone features (dim_in = 128), against the restatement
        check(f"DepthAnything3Net head on backbone features {k}", out[k], o64[k], o32[k])


def test_video_processor_scores_a_clip_with_da3_model(ops):
    from videogpa_amd import scorer as sc
    from videogpa_amd.process_video import VideoProcessor
    net = small_net()
    frames = (torch.rand(3, 42, 56, 3, generator=torch.Generator().manual_seed(6)) * 255).to(torch.uint8).numpy()
    metrics = {"mse": sc.MSEMetric()}
    vp = VideoProcessor(metrics, backbone="da3", da3_model=net)
    res = vp.process(frames, thresholds=[0, 40], num_frames=3)
    pred = vp._run_da3(net, [frames[i] for i in range(3)])
    assert pred.depth.shape == pred.conf.shape == (3, 42, 56) and pred.extrinsics.shape == (3, 3, 4) and pred.intrinsics.shape == (3, 3, 3)
    assert pred.depth.is_cuda and pred.processed_images.shape == (3, 42, 56, 3) and bool((pred.conf > 1).all()) and bool((pred.depth > 0).all())
    ref = VideoProcessor(metrics, backbone="da3", backbone_fn=lambda fl: pred).process(frames, thresholds=[0, 40], num_frames=3)
    assert set(res) == {0, 40, "_extrinsic"} and res["_extrinsic"] == ref["_extrinsic"] == pred.extrinsics.cpu().tolist()
    for th in (0, 40):
        print(f"VideoProcessor(da3_model) threshold {th}: {res[th]} backbone_fn path: {ref[th]}")
        assert isinstance(res[th]["mse"], float) and np.isfinite(res[th]["mse"]) and res[th] == ref[th]
    with pytest.raises(ValueError, match="multiples of 14"):
        vp.process(np.zeros((3, 43, 56, 3), np.uint8), thresholds=[0], num_frames=3)
