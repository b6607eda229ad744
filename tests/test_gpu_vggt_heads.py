"""The VGGT head kernels and modules on the device.  -m gpu only.

Every accuracy bound is 8 x d32.  Error = max-abs difference over max-abs of the float64 answer; d32 = that same distance for the fp32 torch
evaluation of the same output (F.conv2d on the CPU, the restatement of tests/vggt_heads_ref.py, or the fp32 golden of the reference module).
The margin is there because the arithmetic is of the same class (fp32 products, fp32 sums; the fp32 MFMA is a k-ordered fmaf chain) while
the summation order differs and the interpolation / positional embedding are fused.  Every test prints `name err d32 ratio` before it asserts.

Observed err / d32 on an MI355X (also in DESIGN.md section 5b): convolution 1.0-4.6 (largest at K = 9 x 1024), 1x1 with K = 2048 5.9, stride 2 3.8; upsample
0.1-1.0; tail 0.5-1.5; small attention 0.75-1.0; depth / point heads against the goldens 0.4-1.2; camera head 1.03; full-width head 1.10 / 0.75.  The tail call
raises the peak allocation by 17 MB over its inputs."""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vggt_heads_ref as R
from test_vggt_heads_host import DPT_CFG, load_goldens

pytestmark = pytest.mark.gpu
MARGIN = 8.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops
    return ops


def check(name, got, want64, ref32):
    err, d32 = R.rel_err(got, want64), R.rel_err(ref32, want64)
    ratio = err / d32 if d32 > 0 else (0.0 if err == 0 else float("inf"))       # an exact fp32 reference (identity resize) asks for an exact result
    print(f"{name}: err {err:.3e} d32 {d32:.3e} ratio {ratio:.2f}")
    assert np.isfinite(err) and err <= MARGIN * d32, (name, err, d32)
    return ratio


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def run_conv(ops, N, H, W, Cin, Cout, relu_in, bias, res_mode, stride, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    b = torch.randn(Cout, generator=g) if bias else None
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = torch.randn(N, Cout, Ho, Wo, generator=g) if res_mode else None
    res2 = torch.randn(N, Cout, Ho, Wo, generator=g) if res_mode == 3 else None

    def ref(dt):
        y = F.conv2d(F.relu(x.to(dt)) if relu_in else x.to(dt), w.to(dt), None if b is None else b.to(dt), stride=stride, padding=1)
        if res is not None:
            y = y + (F.relu(res.to(dt)) if res_mode >= 2 else res.to(dt))
        if res2 is not None:
            y = y + res2.to(dt)
        return y
    with torch.no_grad():
        got = ops.conv3x3_f32(nhwc(x).cuda(), ops.pack_conv_weight(w).cuda(), None if b is None else b.cuda(), None if res is None else nhwc(res).cuda(),
                              None if res2 is None else nhwc(res2).cuda(), relu_in=relu_in, relu_res=res_mode >= 2, stride=stride)
    assert got.shape == (N, Ho, Wo, Cout)
    return check(f"conv3x3 {N}x{H}x{W} {Cin}->{Cout} relu_in={relu_in} bias={bias} res={res_mode} stride={stride}", got.permute(0, 3, 1, 2),
                 ref(torch.float64), ref(torch.float32))


# res_mode: 0 none, 1 res, 2 relu(res), 3 relu(res) + res2
@pytest.mark.parametrize("relu_in,bias,res_mode", list(itertools.product((False, True), (False, True), (0, 1, 2, 3))))
def test_conv3x3_every_flag_combination(ops, relu_in, bias, res_mode):
    run_conv(ops, 2, 19, 19, 32, 48, relu_in, bias, res_mode, 1, seed=res_mode + 4 * bias + 8 * relu_in)


@pytest.mark.parametrize("hw", [(5, 7), (19, 19), (37, 37), (148, 148)])
@pytest.mark.parametrize("cin,cout", [(16, 16), (32, 32), (128, 128), (256, 256), (1024, 256)])
def test_conv3x3_channels_and_sizes(ops, hw, cin, cout):
    run_conv(ops, 2 if hw[0] < 100 else 1, hw[0], hw[1], cin, cout, True, True, 3, 1, seed=cin + hw[0])


def test_conv3x3_stride2_and_conv1x1(ops):
    run_conv(ops, 2, 19, 19, 128, 128, False, True, 0, 2, seed=5)
    run_conv(ops, 3, 6, 8, 32, 32, False, True, 0, 2, seed=6)
    g = torch.Generator().manual_seed(7)
    x, w, b = torch.randn(3, 37, 2048, generator=g), torch.randn(256, 2048, generator=g) / 2048 ** 0.5, torch.randn(256, generator=g)
    with torch.no_grad():
        got = ops.conv1x1_f32(x.cuda(), w.t().contiguous().cuda(), b.cuda())
        rows = ops.conv1x1_f32(x[1:2].cuda(), w.t().contiguous().cuda(), b.cuda())
    check("conv1x1 2048->256", got, F.linear(x.double(), w.double(), b.double()), F.linear(x, w, b))
    assert torch.equal(rows, got[1:2])                                           # the summation order does not depend on the row count


@pytest.mark.parametrize("shape", [(2, 5, 7, 16, 10, 14), (2, 24, 32, 32, 42, 56), (1, 19, 19, 256, 37, 37), (2, 9, 12, 32, 9, 12)])
@pytest.mark.parametrize("embed", [False, True])
def test_upsample_vs_restatement(ops, shape, embed):
    N, h, w, C, H, W = shape
    x = torch.randn(N, C, h, w, generator=torch.Generator().manual_seed(h))

    def ref(dt):
        y = F.interpolate(x.to(dt), size=(H, W), mode="bilinear", align_corners=True)
        return y + R.uv_embed(W, H, C, 1.3, dt)[None] if embed else y
    with torch.no_grad():
        got = ops.upsample_bilinear_ac_f32(nhwc(x).cuda(), H, W, ops.uv_embed_tables(W, H, C, 1.3, "cuda") if embed else None)
    check(f"upsample {shape} embed={embed}", got.permute(0, 3, 1, 2), ref(torch.float64), ref(torch.float32))


@pytest.mark.parametrize("act,od", [("exp", 2), ("inv_log", 4)])
@pytest.mark.parametrize("embed", [False, True])
@pytest.mark.parametrize("hw", [(42, 56), (70, 98)])
def test_tail_vs_restatement(ops, act, od, embed, hw):
    g = torch.Generator().manual_seed(od)
    H, W = hw
    C, N = 32, 2
    x = torch.randn(N, C, 8 * (H // 14), 8 * (W // 14), generator=g)
    sd = {"scratch.output_conv2.0.weight": torch.randn(32, C, 3, 3, generator=g) / (9 * C) ** 0.5, "scratch.output_conv2.0.bias": torch.randn(32, generator=g),
          "scratch.output_conv2.2.weight": torch.randn(od, 32, 1, 1, generator=g) * 0.4, "scratch.output_conv2.2.bias": torch.randn(od, generator=g)}
    p64, c64 = R.dpt_tail({k: v.double() for k, v in sd.items()}, x.double(), hw, activation=act, pos_embed=embed)
    p32, c32 = R.dpt_tail(sd, x, hw, activation=act, pos_embed=embed)
    with torch.no_grad():
        p, c = ops.dpt_tail_f32(nhwc(x).cuda(), H, W, ops.pack_conv_weight(sd["scratch.output_conv2.0.weight"]).cuda(), sd["scratch.output_conv2.0.bias"].cuda(),
                                sd["scratch.output_conv2.2.weight"].reshape(od, 32).cuda(), sd["scratch.output_conv2.2.bias"].cuda(), activation=act,
                                tabs=ops.uv_embed_tables(W, H, C, W / H, "cuda") if embed else None)
    assert p.shape == p64.shape and c.shape == c64.shape
    check(f"tail {act} embed={embed} {hw} preds", p, p64, p32)
    check(f"tail {act} embed={embed} {hw} conf", c, c64, c32)


def test_attn_small_vs_float64(ops):
    for (B, S, H, D) in ((1, 3, 2, 32), (2, 10, 16, 128), (1, 128, 2, 128), (1, 65, 3, 64)):
        qkv = torch.randn(B, S, 3, H, D, generator=torch.Generator().manual_seed(S))

        def ref(dt):
            q, k, v = qkv.to(dt).permute(2, 0, 3, 1, 4)
            return (torch.softmax(q @ k.transpose(-2, -1) * D ** -0.5, dim=-1) @ v).transpose(1, 2).reshape(B, S, H * D)
        with torch.no_grad():
            got = ops.attn_small_f32(qkv.cuda())
        check(f"attn_small {(B, S, H, D)}", got, ref(torch.float64), ref(torch.float32))


def _dpt(state, od, act):
    from videogpa_amd.vggt import DPTHead
    head = DPTHead(output_dim=od, activation=act, **DPT_CFG)
    head.load_state_dict(state)
    return head.cuda().eval()


@pytest.mark.parametrize("which", ["depth", "point"])
def test_dpt_heads_vs_reference_goldens_and_chunking_is_bit_identical(ops, which):
    g, gp, _, point_state = load_goldens()
    hw, psi = tuple(int(v) for v in g["image_hw"]), int(g["patch_start_idx"])
    gold, head = (g, _dpt(g["state"], 2, "exp")) if which == "depth" else (gp, _dpt(point_state, 4, "inv_log"))
    toks = [t.cuda() for t in g["tokens"]]
    images = torch.zeros(1, 3, 3, *hw, device="cuda")
    with torch.no_grad():
        p, c = head(toks, images, psi)
        p2, c2 = head(toks, images, psi, frames_chunk_size=2)
        p1, c1 = head(toks, images, psi, frames_chunk_size=1)
    assert p.shape == gold["preds64"].shape and c.shape == gold["conf64"].shape
    check(f"{which} head preds", p, gold["preds64"], gold["preds32"])
    check(f"{which} head conf", c, gold["conf64"], gold["conf32"])
    check(f"{which} head preds (chunk 2 golden)", p2, gold["preds64"], gold["chunk2.preds32"])
    assert torch.equal(p, p2) and torch.equal(c, c2) and torch.equal(p, p1) and torch.equal(c, c1)
    with pytest.raises(RuntimeError, match="forward only"):
        head(toks, images, psi)


def test_dpt_head_without_pos_embed_vs_restatement(ops):
    from videogpa_amd.vggt import DPTHead
    g = load_goldens()[0]
    hw, psi = tuple(int(v) for v in g["image_hw"]), int(g["patch_start_idx"])
    head = DPTHead(output_dim=2, activation="exp", pos_embed=False, **DPT_CFG)
    head.load_state_dict(g["state"])
    with torch.no_grad():
        p, c = head.cuda()([t.cuda() for t in g["tokens"]], torch.zeros(1, 3, 3, *hw, device="cuda"), psi)
    p64, c64 = R.dpt_head({k: v.double() for k, v in g["state"].items()}, [t.double() for t in g["tokens"]], hw, psi, pos_embed=False)
    p32, c32 = R.dpt_head(g["state"], g["tokens"], hw, psi, pos_embed=False)
    check("depth head, pos_embed=False, preds", p, p64, p32)
    check("depth head, pos_embed=False, conf", c, c64, c32)


def test_camera_head_vs_reference_golden(ops):
    from videogpa_amd.vggt import CameraHead
    gc = load_goldens()[2]
    cam = CameraHead(dim_in=64, trunk_depth=2, num_heads=2)
    cam.load_state_dict(gc["state"])
    cam = cam.cuda().eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):          # fp32 whatever autocast says
        out = cam([gc["tokens"].cuda()], num_iterations=4)
    assert len(out) == 4 and out[0].shape == (1, 3, 9) and out[0].dtype == torch.float32
    check("camera head", torch.stack(out), gc["pose64"], gc["pose32"])


def _full_width_state(seed):
    from videogpa_amd.vggt import DPTHead
    torch.manual_seed(seed)
    head = DPTHead(dim_in=2048, output_dim=2, activation="exp", intermediate_layer_idx=[0, 1, 2, 3])
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in head.named_parameters():
            if p.ndim >= 2:
                fan_in = p.shape[0] if name.startswith(("resize_layers.0", "resize_layers.1")) else p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * 1.1 / fan_in ** 0.5)
            else:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g) if name == "norm.weight" else 0.1 * torch.randn(p.shape, generator=g))
    return head


def test_full_width_head_vs_float64_restatement(ops):
    """dim_in 2048, features 256, 2 frames of 518 x 518: float64 restatement on the CPU, d32 from the fp32 restatement on the device"""
    head = _full_width_state(3)
    g = torch.Generator().manual_seed(4)
    toks = [torch.randn(1, 2, 5 + 37 * 37, 2048, generator=g) for _ in range(4)]
    sd = {k: v.detach() for k, v in head.state_dict().items()}
    with torch.no_grad():
        p64, c64 = R.dpt_head({k: v.double() for k, v in sd.items()}, [t.double() for t in toks], (518, 518), 5)
        prev = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
        torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
        try:
            p32, c32 = R.dpt_head({k: v.cuda() for k, v in sd.items()}, [t.cuda() for t in toks], (518, 518), 5)
        finally:
            torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = prev
        p, c = head.cuda().eval()([t.cuda() for t in toks], torch.zeros(1, 2, 3, 518, 518, device="cuda"), 5)
    assert p.shape == (1, 2, 518, 518, 1) and c.shape == (1, 2, 518, 518)
    check("full-width depth head preds", p, p64, p32)
    check("full-width depth head conf", c, c64, c32)


def test_tail_never_builds_the_full_resolution_tensor(ops):
    """8 frames, full width: the call's peak allocation stays below 256 MB over its inputs (its outputs are 43 MB; [8,518,518,128] fp32 is 1.1 GB)"""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(8, 296, 296, 128, generator=g).cuda()
    w1, b1 = ops.pack_conv_weight(torch.randn(32, 128, 3, 3, generator=g) / 34).cuda(), torch.randn(32, generator=g).cuda()
    w2, b2 = (torch.randn(2, 32, generator=g) * 0.2).cuda(), torch.randn(2, generator=g).cuda()
    tabs = ops.uv_embed_tables(518, 518, 128, 1.0, "cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    with torch.no_grad():
        p, c = ops.dpt_tail_f32(x, 518, 518, w1, b1, w2, b2, activation="exp", tabs=tabs)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"tail peak allocation over its inputs: {grown / 1e6:.1f} MB")
    assert p.shape == (8, 518, 518, 1) and bool(torch.isfinite(p).all()) and bool(torch.isfinite(c).all())
    assert grown < 256e6, grown


SMALL = dict(img_size=28, patch_size=14, embed_dim=64, patch_embed="conv", aggregator_kwargs=dict(depth=4, num_heads=1),
             camera_kwargs=dict(trunk_depth=2, num_heads=2), dpt_kwargs=dict(features=32, out_channels=[16, 16, 32, 32], intermediate_layer_idx=[0, 1, 2, 3]))


def _small_vggt(seed=0):
    from videogpa_amd.vggt import VGGT
    torch.manual_seed(seed)
    m = VGGT(**SMALL)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "head" in name and p.ndim >= 2:
                p.mul_(1.5)
    return m.cuda().eval()


def test_vggt_forward_equals_aggregator_then_heads(ops):
    m = _small_vggt()
    images = torch.rand(1, 3, 3, 42, 56, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):         # the aggregator's kernels are bf16; the heads stay fp32
        out = m(images)
        toks, psi = m.aggregator(images)
        pose = m.camera_head(toks)
        d, dc = m.depth_head(toks, images=images, patch_start_idx=psi)
        w, wc = m.point_head(toks, images=images, patch_start_idx=psi)
        unbatched = m(images[0])
    assert set(out) == {"pose_enc", "pose_enc_list", "depth", "depth_conf", "world_points", "world_points_conf", "images"}
    assert out["depth"].shape == (1, 3, 42, 56, 1) and out["depth_conf"].shape == (1, 3, 42, 56) and out["world_points"].shape == (1, 3, 42, 56, 3)
    assert out["pose_enc"].shape == (1, 3, 9) and len(out["pose_enc_list"]) == 4
    for a, b in ((out["pose_enc"], pose[-1]), (out["depth"], d), (out["depth_conf"], dc), (out["world_points"], w), (out["world_points_conf"], wc),
                 (unbatched["depth"], d)):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert out["depth"].dtype == torch.float32 and out["pose_enc"].dtype == torch.float32
    with pytest.raises(NotImplementedError):
        m(images, query_points=torch.zeros(1, 2, device="cuda"))


def test_video_processor_runs_on_the_own_vggt(ops):
    from videogpa_amd import scorer as sc
    from videogpa_amd.process_video import VideoProcessor
    m = _small_vggt(2)
    frames = np.random.default_rng(3).integers(0, 256, (3, 72, 128, 3), dtype=np.uint8)
    metrics = {"mse": sc.MSEMetric(), "psnr": sc.PSNRMetric()}
    vp = VideoProcessor(metrics, backbone="vggt", vggt_model=m)
    res = vp.process(frames, thresholds=[0.0, 50.0], num_frames=3)
    preds = vp.backbone_fn(frames)
    assert preds["depth"].shape == (3, 294, 518, 1) and preds["world_points_from_depth"].shape == (3, 294, 518, 3) and preds["pose_enc"].shape == (3, 9)
    same = VideoProcessor(metrics, backbone="vggt", backbone_fn=lambda fr: preds).process(frames, thresholds=[0.0, 50.0], num_frames=3)
    for th in (0.0, 50.0):
        for name in metrics:
            a, b = float(res[th][name]), float(same[th][name])
            print(f"VideoProcessor th {th} {name}: {a:.6f} / {b:.6f}")
            assert np.isfinite(a) and a == b
    assert np.isfinite(np.asarray(res["_extrinsic"])).all()
