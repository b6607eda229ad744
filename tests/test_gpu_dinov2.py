"""The DINOv2 patch embedding on the device: the fused token-embed kernel (csrc/dino_embed.hip) against a float64 torch-op evaluation, its
bit-stability under frame splits, the whole DinoVisionTransformer and the aggregator behind it against goldens made by the reference's own modules
(tests/golden/make_golden_dinov2.py), and a small VGGT with a DINOv2 front through the VideoProcessor.

Bounds.  Kernel, fp32 out: 8 x d32, d32 = the distance of the fp32 torch evaluation (conv2d + cat + add) from the float64 one -- the bound of the
heads' convolutions; bf16 out: that + 2^-8 (one bf16 rounding of the largest element, doubled).  Errors are max-abs over the max-abs of the float64
answer, taken separately for the class row, the register rows and the patch rows.  Whole module: every returned tensor within 2 x d16, d16 = the
distance of a bf16-autocast torch evaluation (tests/dinov2_ref.py, same session) from the float64 golden -- two realisations of the same rounding
noise, the factor of the SSIM tests -- and within the family's cap, 2 % of range and cosine >= 0.999."""
import os

import numpy as np
import pytest
import torch

import dinov2_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("x_norm_patchtokens", "x_norm_clstoken", "x_norm_regtokens", "x_prenorm")
SHAPES = ("70x70", "42x70", "98x56")


def gold(name):
    return torch.load(os.path.join(HERE, "golden", name))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops as o
    return o


def golden_state(tag):
    g = gold(f"vggt_dinov2_{tag}.pt")
    state = R.seeded_state(g["shapes"], g["cfg"]["seed"])
    R.check_state_sums(state, g["sums"])
    if tag == "a":
        stored = gold("vggt_dinov2_a_state.pt")
        assert all(torch.equal(state[k], stored[k]) for k in stored)
    return g, state


def rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


def embed_case(name):
    """-> (images fp32 [N,3,H,W], {proj weight, bias, cls, reg, pos [1+P,C]} fp32), all on the CPU"""
    if name[0] in "ab":
        g, state = golden_state(name[0])
        x = gold("vggt_dinov2_inputs.pt")[name[2:]]
        return x, {"w": state["patch_embed.proj.weight"], "b": state["patch_embed.proj.bias"], "cls": state["cls_token"], "reg": state["register_tokens"],
                   "pos": g["cases"][name[2:]]["pos"][0]}
    N, H, W, C = (int(v) for v in name.split(","))
    gen = torch.Generator().manual_seed(N * 1000003 + H * 1009 + W * 13 + C)
    P = (H // 14) * (W // 14)
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    return (torch.rand(N, 3, H, W, generator=gen) - mean) / std, {
        "w": (2 * torch.rand(C, 3, 14, 14, generator=gen) - 1) / 588 ** 0.5, "b": 0.1 * torch.randn(C, generator=gen),
        "cls": 0.5 * torch.randn(1, 1, C, generator=gen), "reg": 0.5 * torch.randn(1, 4, C, generator=gen), "pos": 0.3 * torch.randn(1 + P, C, generator=gen)}


def torch_embed(x, p, dtype):
    sd = {"patch_embed.proj.weight": p["w"].to(dtype), "patch_embed.proj.bias": p["b"].to(dtype), "cls_token": p["cls"].to(dtype),
          "register_tokens": p["reg"].to(dtype)}
    return R.prepare_tokens(sd, x.to(dtype), 14, p["pos"][None].to(dtype))


EMBED_CASES = [f"{t}:{s}" for t in "ab" for s in SHAPES] + ["2,518,518,1024", "3,294,518,1024", "1,14,14,32", "5,70,42,384"]


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["out32", "out16"])
@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16], ids=["in32", "in16"])
@pytest.mark.parametrize("case", EMBED_CASES)
def test_dino_embed_against_float64(ops, case, in_dtype, out_dtype):
    x, p = embed_case(case)
    x = x.to(in_dtype).cuda()                                  # a bf16 input is the input: both evaluations start from the rounded frames
    p = {k: v.cuda() for k, v in p.items()}
    with torch.no_grad():
        ref64, ref32 = torch_embed(x, p, torch.float64), torch_embed(x, p, torch.float32)
        got = ops.dino_embed(x, ops.pack_patch_weight(p["w"]), p["b"].contiguous(), p["cls"], p["reg"], p["pos"].contiguous(), out_dtype)
    assert got.dtype == out_dtype and got.shape == ref64.shape and bool(torch.isfinite(got).all())
    if case.startswith("a:") and in_dtype == torch.float32:     # the torch-op evaluation is the reference's own prepare_tokens_with_masks
        assert rel(ref64.cpu(), gold("vggt_dinov2_a.pt")["cases"][case[2:]]["prepare64"]) < 1e-9
    R_ = p["reg"].shape[1]
    for what, rows in (("class row", slice(0, 1)), ("register rows", slice(1, 1 + R_)), ("patch rows", slice(1 + R_, None))):
        d32, err = rel(ref32[:, rows], ref64[:, rows]), rel(got[:, rows], ref64[:, rows])
        bound = 8 * d32 + (2.0 ** -8 if out_dtype == torch.bfloat16 else 0.0)
        print(f"dino_embed {case} {str(in_dtype)[6:]}->{str(out_dtype)[6:]} {what}: err {err:.3e} d32 {d32:.3e} bound {bound:.3e}")
        assert err <= bound, (case, what, err, d32, bound)


@pytest.mark.parametrize("case,cut", [("5,70,42,384", 2), ("3,294,518,1024", 1), ("b:98x56", 1)])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["out32", "out16"])
def test_dino_embed_is_bit_identical_under_frame_splits(ops, case, cut, out_dtype):
    x, p = embed_case(case)
    x, p = x.cuda(), {k: v.cuda() for k, v in p.items()}
    args = (ops.pack_patch_weight(p["w"]), p["b"].contiguous(), p["cls"], p["reg"], p["pos"].contiguous(), out_dtype)
    with torch.no_grad():
        whole = ops.dino_embed(x, *args)
        parts = torch.cat([ops.dino_embed(x[:cut].contiguous(), *args), ops.dino_embed(x[cut:].contiguous(), *args)])
        again = ops.dino_embed(x, *args)
    assert torch.equal(whole, parts) and torch.equal(whole, again)


@pytest.mark.parametrize("M,D", [(7, 64), (300, 1024), (33, 1536), (5, 40)])
def test_stream_ln_against_float64(ops, M, D):
    """The fp32 residual-stream kernel: x + gamma * y and the LayerNorm behind it against float64 torch ops.  Bound: 8 x d32 as for the embed kernel (fp32
    in, fp32 arithmetic, another summation order), + 2^-8 where the output is bf16."""
    gen = torch.Generator().manual_seed(M * 131 + D)
    x, y = torch.randn(2, M, D, generator=gen).cuda(), torch.randn(2, M, D, generator=gen).to(torch.bfloat16).cuda()
    gamma, w, b = (0.5 + torch.rand(D, generator=gen)).cuda(), (1 + 0.2 * torch.randn(D, generator=gen)).cuda(), (0.1 * torch.randn(D, generator=gen)).cuda()

    def ref(dt):
        xn = x.to(dt) + gamma.to(dt) * y.to(dt)
        return xn, torch.nn.functional.layer_norm(xn, (D,), w.to(dt), b.to(dt), 1e-6), torch.nn.functional.layer_norm(x.to(dt), (D,), w.to(dt), b.to(dt), 1e-6)
    (x64, n64, p64), (x32, n32, p32) = ref(torch.float64), ref(torch.float32)
    with torch.no_grad():
        xa, na = ops.stream_ln(x, y, gamma, w, b, 1e-6, torch.bfloat16)
        xb, nb = ops.stream_ln(x, y, gamma, w, b, 1e-6, torch.float32)
        xc, nc = ops.stream_ln(x, y, gamma)
        xd, nd = ops.stream_ln(x, None, None, w, b, 1e-6, torch.float32)
    assert nc is None and xd is None and torch.equal(xa, xb) and torch.equal(xa, xc) and na.dtype == torch.bfloat16
    for what, got, r64, r32, extra in (("x_new", xa, x64, x32, 0.0), ("LN fp32", nb, n64, n32, 0.0), ("LN bf16", na, n64, n32, 2.0 ** -8), ("plain LN", nd, p64, p32, 0.0)):
        err, d32 = rel(got, r64), rel(r32, r64)
        print(f"stream_ln [{M} x {D}] {what}: err {err:.3e} d32 {d32:.3e}")
        assert err <= 8 * d32 + extra, (what, err, d32)
    with pytest.raises(RuntimeError, match="forward only"):
        ops.stream_ln(x.clone().requires_grad_(True), y, gamma)
    with torch.no_grad(), pytest.raises(RuntimeError, match="do not fit"):
        ops.stream_ln(x, y[:, :1].contiguous(), gamma)


def test_dino_embed_refuses_what_it_does_not_cover(ops):
    x, p = embed_case("1,14,14,32")
    x, p = x.cuda(), {k: v.cuda() for k, v in p.items()}
    wp = ops.pack_patch_weight(p["w"])
    with pytest.raises(RuntimeError, match="forward only"):
        ops.dino_embed(x.requires_grad_(True), wp, p["b"], p["cls"], p["reg"], p["pos"])
    x = x.detach()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="do not fit"):
            ops.dino_embed(x[:, :, :, :13].contiguous(), wp, p["b"], p["cls"], p["reg"], p["pos"])
        with pytest.raises(RuntimeError, match="do not fit"):
            ops.dino_embed(x, wp[:588].contiguous(), p["b"], p["cls"], p["reg"], p["pos"])
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.dino_embed(x.transpose(2, 3), wp, p["b"], p["cls"], p["reg"], p["pos"])
        none = ops.dino_embed(x, wp, p["b"], p["cls"], None, p["pos"], torch.float32)          # no registers: [N, 1 + P, C]
    assert none.shape == (1, 2, 32) and torch.equal(none[:, 0], (p["cls"].reshape(-1) + p["pos"][0])[None])


def build(cfg, state):
    from videogpa_amd.vggt import DinoVisionTransformer
    m = DinoVisionTransformer(img_size=cfg["img_size"], patch_size=cfg["patch_size"], embed_dim=cfg["embed_dim"], depth=cfg["depth"],
                              num_heads=cfg["num_heads"], mlp_ratio=4, num_register_tokens=cfg["num_register_tokens"], interpolate_antialias=True,
                              interpolate_offset=0.0, block_chunks=0, init_values=1.0)
    m.load_state_dict(state, strict=True)
    return m.cuda().eval()


def cosine(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm()).clamp_min(1e-300))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("tag", ["a", "b"])
def test_whole_module_matches_the_reference_goldens(ops, tag, shape):
    g, state = golden_state(tag)
    cfg, c = g["cfg"], g["cases"][shape]
    x = gold("vggt_dinov2_inputs.pt")[shape].cuda()
    m = build(cfg, state)
    sd = {k: v.cuda() for k, v in state.items()}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        got = m(x)
        noise = R.forward(sd, x, cfg["patch_size"], cfg["num_heads"])
        inter = m.get_intermediate_layers(x, n=1, reshape=True, return_class_token=True, norm=True)
        got_train = m.train()(x)                                                   # train mode under no_grad: the same values
        m.eval()
    assert got["masks"] is None and set(got) == set(KEYS) | {"masks"}
    pos = m.pos_table(x.shape[2], x.shape[3])
    assert (pos is m.pos_embed) == (shape == "70x70") and rel(pos.detach().cpu(), c["pos"]) <= 1e-5
    fails = []
    for k in KEYS:
        ref = c[k + "64"]
        assert got[k].shape == ref.shape and got[k].dtype == torch.float32 and torch.equal(got[k], got_train[k])     # fp32, as autocast returns upstream
        err, d16, cos = rel(got[k].cpu(), ref), rel(noise[k].cpu(), ref), cosine(got[k].cpu(), ref)
        print(f"dinov2 ({tag}) {shape} {k}: err {err:.4e} d16 {d16:.4e} ratio {err / d16:.3f} cosine {cos:.6f} (reference's CPU bf16 distance "
              f"{c['ref_bf16_distance'][k]:.4e})")
        if not (err <= 2 * d16 and err <= 0.02 and cos >= 0.999):
            fails.append((k, err, d16, cos))
    assert not fails, fails
    (patch_map, cls), = inter
    hp, wp = x.shape[2] // 14, x.shape[3] // 14
    assert patch_map.shape == (2, cfg["embed_dim"], hp, wp) and torch.equal(cls, got["x_norm_clstoken"])
    assert torch.equal(patch_map, got["x_norm_patchtokens"].reshape(2, hp, wp, -1).permute(0, 3, 1, 2))
    with torch.no_grad():                                                          # bf16 parameters, no autocast: the other side of the contract
        mb = m.to(torch.bfloat16)
        out16 = mb(x.to(torch.bfloat16))
    assert rel(out16["x_prenorm"].cpu(), c["x_prenorm64"]) <= 0.02 and cosine(out16["x_prenorm"].cpu(), c["x_prenorm64"]) >= 0.999


def _close(got, ref, tol, what):          # the bounds of tests/test_gpu_vggt.py
    got, ref = got.float().cpu(), ref.float()
    err = (got - ref).abs().max().item()
    cos = cosine(got, ref)
    print(f"{what}: err / range {err / ref.abs().max().item():.4e} cosine {cos:.6f}")
    assert err <= tol * ref.abs().max().item() and cos >= 0.999, (what, err, ref.abs().max().item(), cos)


def test_aggregator_with_the_dinov2_front_matches_the_reference(ops):
    from videogpa_amd.vggt import Aggregator, DinoVisionTransformer
    c = gold("vggt_dinov2_agg.pt")
    cfg = c["cfg"]
    front = DinoVisionTransformer(img_size=70, patch_size=14, embed_dim=cfg["embed_dim"], depth=cfg["dino_depth"], num_heads=cfg["num_heads"], mlp_ratio=4,
                                  num_register_tokens=4, interpolate_antialias=True, interpolate_offset=0.0, block_chunks=0, init_values=1.0)
    agg = Aggregator(img_size=70, patch_size=14, embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"], mlp_ratio=cfg["mlp_ratio"],
                     num_register_tokens=4, patch_embed=front, qk_norm=True, rope_freq=100, init_values=0.01)
    state = R.seeded_state({k: v.shape for k, v in agg.state_dict().items()}, cfg["seed"], bf16_representable=True)
    R.check_state_sums(state, c["sums"])
    agg.load_state_dict(state, strict=True)                                         # the reference's names, strictly
    agg = agg.to(device="cuda", dtype=torch.bfloat16).eval()
    with torch.no_grad():
        outs, start = agg(c["images"].cuda().float())
    assert start == c["patch_start_idx"] and len(outs) == len(c["outputs"])
    for i, (o, r) in enumerate(zip(outs, c["outputs"])):
        assert o.shape == r.shape
        _close(o, r, 0.02, f"aggregator behind DINOv2, depth {i}")
    with pytest.raises(RuntimeError, match="forward only"):                         # grad mode: the front has no backward
        agg(c["images"].cuda().float())


def test_video_processor_runs_on_a_vggt_with_the_dinov2_front(ops):
    from videogpa_amd import scorer as sc
    from videogpa_amd.process_video import VideoProcessor
    from videogpa_amd.vggt import VGGT, DinoVisionTransformer
    torch.manual_seed(5)
    m = VGGT(img_size=28, patch_size=14, embed_dim=384, patch_embed="dinov2_vits14_reg", aggregator_kwargs=dict(depth=4, num_heads=6),
             camera_kwargs=dict(trunk_depth=2, num_heads=6), dpt_kwargs=dict(features=32, out_channels=[16, 16, 32, 32], intermediate_layer_idx=[0, 1, 2, 3]))
    assert isinstance(m.aggregator.patch_embed, DinoVisionTransformer) and len(m.aggregator.patch_embed.blocks) == 12
    m = m.cuda().eval()
    frames = np.random.default_rng(3).integers(0, 256, (3, 72, 128, 3), dtype=np.uint8)
    metrics = {"mse": sc.MSEMetric(), "psnr": sc.PSNRMetric()}
    vp = VideoProcessor(metrics, backbone="vggt", vggt_model=m)
    res = vp.process(frames, thresholds=[0.0, 50.0], num_frames=3)
    preds = vp.backbone_fn(frames)
    assert preds["depth"].shape == (3, 294, 518, 1) and preds["world_points_from_depth"].shape == (3, 294, 518, 3) and preds["pose_enc"].shape == (3, 9)
    for k in ("depth", "world_points_from_depth", "pose_enc"):
        assert np.isfinite(np.asarray(preds[k].cpu() if torch.is_tensor(preds[k]) else preds[k], dtype=np.float64)).all(), k
    for th in (0.0, 50.0):
        for name in metrics:
            print(f"VideoProcessor (DINOv2 front) th {th} {name}: {float(res[th][name]):.6f}")
            assert np.isfinite(float(res[th][name]))
    images = torch.rand(1, 2, 3, 28, 42, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(RuntimeError, match="forward only"):
            m(images.clone().requires_grad_(True))
        with torch.no_grad():
            out = m(images)
    assert out["depth"].shape == (1, 2, 28, 42, 1) and bool(torch.isfinite(out["depth"]).all())
