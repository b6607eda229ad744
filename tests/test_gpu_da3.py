"""Depth Anything 3's backbone and camera decoder on the device (videogpa_amd/da3.py, csrc/da3.hip): the kernels one by one against torch in float64, the
whole backbone against goldens made by the reference's own modules (tests/golden/make_golden_da3.py), and the cameras.

Bounds.  Selection metrics and the tap's LayerNorm: 4 x d32, d32 = the distance of torch's own fp32 evaluation of the same formula on the same input from
its float64 one (max-abs over the max-abs of the float64 answer).  Gather, restore, camera-token write, the tap's copied half and its camera row: bit
for bit.  Whole backbone: the rule of tests/test_gpu_dinov2.py -- every returned tensor within 2 x d16 of the float64 golden, d16 = the distance of the
reference's own bf16-autocast evaluation (stored per output tensor), and within the family's cap, 2 % of range and cosine >= 0.999.  Cameras: 8 x the
reference's fp32-vs-float64 distance stored in the fixture."""
import os

import pytest
import torch
import torch.nn.functional as F

import da3_ref as D
import dinov2_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STRATEGIES = ("first", "middle", "saddle_balanced", "saddle_sim_range")
# inputs whose float64 balance scores have a gap >= 0.05 between the best two views (and distinct similarity ranges), found on the CPU
SCORE_SEEDS = {(1, 3, 64): 1, (1, 3, 384): 1, (1, 3, 1024): 1, (1, 4, 64): 2, (1, 4, 384): 2, (1, 4, 1024): 1, (1, 10, 64): 1, (1, 10, 384): 3, (1, 10, 1024): 1,
               (2, 3, 64): 2, (2, 3, 384): 2, (2, 3, 1024): 5, (2, 4, 64): 2, (2, 4, 384): 1, (2, 4, 1024): 1, (2, 10, 64): 1, (2, 10, 384): 1, (2, 10, 1024): 1}


def gold(name):
    return torch.load(os.path.join(HERE, "golden", name))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops as o
    return o


def cosine(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm()).clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------------------ 1. selection
def class_tokens(seed, B, S, C):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, C, generator=g) * (0.5 + torch.rand(B, S, 1, generator=g))


@pytest.mark.parametrize("B,S,C", sorted(SCORE_SEEDS))
def test_ref_view_scores_and_choice_against_float64(ops, B, S, C):
    cls = class_tokens(SCORE_SEEDS[(B, S, C)], B, S, C)
    m64, m32 = D.select_metrics(cls.double()), D.select_metrics(cls)
    top = m64[3].sort(dim=1).values
    assert float((top[:, 1] - top[:, 0]).min()) >= 0.05, "the seed no longer gives a float64 gap of 0.05"
    rng = m64[4].sort(dim=1, descending=True).values
    assert float((rng[:, 0] - rng[:, 1]).min()) >= 1e-4
    x = torch.randn(B, S, 3, C, generator=torch.Generator().manual_seed(5))
    x[:, :, 0] = cls
    x = x.cuda()
    for strategy in STRATEGIES:
        ref_idx, met = ops.da3_ref_view(x, strategy, return_metrics=True)
        assert ref_idx.dtype == torch.int32 and ref_idx.is_cuda and met.shape == (B, S, 4)
        assert ref_idx.cpu().tolist() == D.select(cls.double(), strategy).tolist(), strategy
        for k, what in enumerate(("mean off-diagonal similarity", "norm", "variance of the normalised token")):
            err, d32 = D.rel(met[..., k].cpu(), m64[k]), D.rel(m32[k], m64[k])
            print(f"ref_view [{B},{S},{C}] {strategy} {what}: err {err:.3e} d32 {d32:.3e}")
            assert err <= 4 * d32, (what, err, d32)
        score = m64[4] if strategy == "saddle_sim_range" else m64[3]
        assert D.rel(met[..., 3].cpu(), score) <= 4 * D.rel((m32[4] if strategy == "saddle_sim_range" else m32[3]), score)
        assert torch.equal(ref_idx, ops.da3_ref_view(x, strategy))          # the same answer without the metrics buffer, and run to run


def test_ref_view_edges(ops):
    x = torch.randn(2, 65, 2, 64, device="cuda")
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.da3_ref_view(x)                                                  # more than 64 views
    assert ops.da3_ref_view(x[:, :64].contiguous()).shape == (2,)
    with pytest.raises(ValueError, match="Unknown reference view selection strategy"):
        ops.da3_ref_view(x[:, :4].contiguous(), "last")
    for strategy in STRATEGIES:                                              # one view: always 0
        assert ops.da3_ref_view(x[:, :1].contiguous(), strategy).cpu().tolist() == [0, 0]
    tie = torch.randn(1, 1, 2, 64, device="cuda").expand(1, 5, 2, 64).contiguous()          # identical views: every score ties, the lowest index wins
    assert ops.da3_ref_view(tie, "saddle_balanced").item() == 0 and ops.da3_ref_view(tie, "saddle_sim_range").item() == 0
    assert ops.da3_ref_view(tie, "middle").item() == 2


# ------------------------------------------------------------------------------------------------------------------------ 2. gather / restore
@pytest.mark.parametrize("S", [2, 3, 5])
def test_view_gather_and_restore_are_torch_indexing_bit_for_bit(ops, S):
    B, N, C = 2, 3, 36
    g = torch.Generator().manual_seed(S)
    x, y = torch.randn(B, S, N, C, generator=g).cuda(), torch.randn(B, S, N, C, generator=g).cuda()
    for r in range(S):
        refs = [r, (r + 1) % S]                                              # another reference per batch element
        ref_idx = torch.tensor(refs, dtype=torch.int32, device="cuda")
        want = torch.stack([x[b, D.order(refs[b], S)] for b in range(B)])
        want_y = torch.stack([y[b, D.order(refs[b], S)] for b in range(B)])
        got = ops.da3_view_gather(x, ref_idx)
        got2, got_y = ops.da3_view_gather(x, ref_idx, other=y)
        assert torch.equal(got, want) and torch.equal(got2, want) and torch.equal(got_y, want_y), refs
        back = torch.stack([got[b, D.inverse_order(refs[b], S)] for b in range(B)])
        assert torch.equal(ops.da3_view_gather(got, ref_idx, inverse=True), back) and torch.equal(back, x), refs
        bx, by = ops.da3_view_gather(got, ref_idx, other=got_y, inverse=True)
        assert torch.equal(bx, x) and torch.equal(by, y), refs


def test_view_gather_large_slab_and_refusals(ops):
    from videogpa_amd import _lib
    B, S, N, C = 1, 2, 4100, 1024                                            # a slab of more float4 than one pass of the grid covers
    x = torch.randn(B, S, N, C, device="cuda")
    ref_idx = torch.tensor([1], dtype=torch.int32, device="cuda")
    got = ops.da3_view_gather(x, ref_idx)
    assert torch.equal(got, x[:, [1, 0]]) and torch.equal(ops.da3_view_gather(got, ref_idx, inverse=True), x)
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="invalid argument"):              # never in place
        _lib.call("vgpa_da3_view_gather", x, x, None, None, ref_idx, 0, B, S, N, C, stream)
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.da3_view_gather(x, ref_idx, other=x[:, :, :1].contiguous())
    with pytest.raises(RuntimeError, match="int32"):
        ops.da3_view_gather(x, ref_idx.long())
    with pytest.raises(RuntimeError, match="forward only"):
        ops.da3_view_gather(x.clone().requires_grad_(True), ref_idx)


# ------------------------------------------------------------------------------------------------------------------------ 3. camera token
@pytest.mark.parametrize("B,S,N,C", [(2, 3, 4, 100), (1, 1, 2, 64), (2, 5, 3, 1028)])
def test_cam_token_write_is_exact_and_touches_nothing_else(ops, B, S, N, C):
    g = torch.Generator().manual_seed(B * 100 + S)
    x = torch.randn(B, S, N, C, generator=g).cuda()
    param, own = torch.randn(1, 2, C, generator=g).cuda(), torch.randn(B, S, C, generator=g).cuda()
    for cam, per_view in ((param, False), (own, True)):
        t = x.clone()
        assert ops.da3_cam_token(t, cam, per_view=per_view) is t
        want = x.clone()
        want[:, :, 0] = cam if per_view else torch.cat([param[:, :1].expand(B, 1, C), param[:, 1:].expand(B, S - 1, C)], dim=1)
        assert torch.equal(t, want)
    with pytest.raises(RuntimeError, match="camera_token parameter"):
        ops.da3_cam_token(x, own[:, :, :8].contiguous(), per_view=False)


# ------------------------------------------------------------------------------------------------------------------------ 4. tap
@pytest.mark.parametrize("B,S,N,C", [(2, 3, 14, 384), (1, 4, 6, 100), (2, 2, 3, 2052), (1, 1, 1, 64)])
def test_tap_copies_exactly_and_normalises_within_fp32(ops, B, S, N, C):
    g = torch.Generator().manual_seed(N * 1000 + C)
    local, x = torch.randn(B, S, N, C, generator=g).cuda(), (2.0 * torch.randn(B, S, N, C, generator=g) + 0.3).cuda()
    w, b = (1 + 0.2 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
    for refs in (None, [(S - 1 - i) % S for i in range(B)]):
        ref_idx = None if refs is None else torch.tensor(refs, dtype=torch.int32, device="cuda")
        feats, cam = ops.da3_tap(local, x, w, b, 1e-5, ref_idx)
        assert feats.shape == (B, S, N - 1, 2 * C) and cam.shape == (B, S, 2 * C) and feats.dtype == cam.dtype == torch.float32
        if refs is None:
            ls, xs = local, x
        else:                                                                 # the inputs are in reordered view order: the outputs in the original one
            ls = torch.stack([local[i, D.inverse_order(refs[i], S)] for i in range(B)])
            xs = torch.stack([x[i, D.inverse_order(refs[i], S)] for i in range(B)])
        assert torch.equal(cam, torch.cat([ls[:, :, 0], xs[:, :, 0]], dim=-1))
        assert torch.equal(feats[..., :C], ls[:, :, 1:])
        if N > 1:
            n64 = F.layer_norm(xs[:, :, 1:].double(), (C,), w.double(), b.double(), 1e-5)
            n32 = F.layer_norm(xs[:, :, 1:], (C,), w, b, 1e-5)
            err, d32 = D.rel(feats[..., C:], n64), D.rel(n32, n64)
            print(f"tap [{B},{S},{N},{C}] restore {refs}: err {err:.3e} d32 {d32:.3e}")
            assert err <= 4 * d32, (err, d32)
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.da3_tap(local, x, w[:4].contiguous(), b, 1e-5)


# ------------------------------------------------------------------------------------------------------------------------ 5. the backbone
_MODELS = {}


def model(tag):
    """the configuration's DA3Cameras on the device with the golden's states (regenerated from the seeded recipe and checked against the stored sums)"""
    if tag not in _MODELS:
        from videogpa_amd.da3 import CameraDec, DA3Cameras, DinoV2
        g = gold(f"da3_{tag}.pt")
        cfg = g["cfg"]
        assert {k: v for k, v in cfg.items() if k in D.CONFIGS[tag]} == D.CONFIGS[tag]
        state, dec_state = D.seeded_state(g["shapes"], cfg["seed"]), D.cam_dec_state(g["cam_dec_shapes"], cfg["seed"])
        dinov2_ref.check_state_sums(state, g["sums"])
        dinov2_ref.check_state_sums(dec_state, g["cam_dec_sums"])
        net = DinoV2("vits", cfg["out_layers"], cfg["alt_start"], cfg["qknorm_start"], cfg["rope_start"], True,
                     encoder_kwargs=dict(img_size=cfg["img_size"], patch_size=cfg["patch_size"], embed_dim=cfg["embed_dim"], depth=cfg["depth"],
                                         num_heads=cfg["num_heads"]))
        net.pretrained.load_state_dict(state, strict=True)
        dec = CameraDec(2 * cfg["embed_dim"])
        dec.load_state_dict(dec_state, strict=True)
        _MODELS[tag] = (g, DA3Cameras(net, dec).cuda().eval())
    return _MODELS[tag]


def case_inputs(g, name):
    B, S, hw, strategy, own_cam = D.CASES[name]
    seed = g["input_seed"][name]
    x = torch.cat([D.images(s, 1, S, hw) for s in seed]) if isinstance(seed, list) else D.images(seed, B, S, hw)
    cam = D.cam_tokens(seed, B, S, g["cfg"]["embed_dim"]).cuda() if own_cam else None
    return x.cuda(), cam, strategy


def run(m, x, cam, strategy):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        feats, aux = m.backbone(x, cam_token=cam, ref_view_strategy=strategy)
    assert aux == []
    return feats


ALL_CASES = [(tag, name) for tag in D.CONFIGS for name in D.CASES_OF[tag]]


@pytest.mark.parametrize("tag,name", ALL_CASES, ids=[f"{t}-{n}" for t, n in ALL_CASES])
def test_backbone_matches_the_reference_goldens(ops, tag, name):
    g, m = model(tag)
    c = D.load_case(os.path.join(HERE, "golden"), tag, name)
    B, S, (H, W), strategy, own_cam = D.CASES[name]
    x, cam, strategy = case_inputs(g, name)
    feats = run(m, x, cam, strategy)
    C, P = g["cfg"]["embed_dim"], (H // 14) * (W // 14)
    assert len(feats) == len(g["cfg"]["out_layers"]) == len(c["out64"])
    pos = m.backbone.pretrained.pos_table(H, W)
    assert (pos is m.backbone.pretrained.pos_embed) == ((H, W) == (70, 70))
    selects = S >= 3 and not own_cam
    chosen = m.backbone.pretrained.ref_idx
    assert (chosen is not None) == selects and ("ref64" in c) == selects
    if selects:
        if strategy == "saddle_balanced":                      # a kept case: float64, fp32 and bf16 autocast agree upstream, with a float64 gap >= 0.15
            assert torch.equal(c["ref64"], c["ref32"]) and torch.equal(c["ref64"], c["ref16"]) and c["gap64"] >= 0.15
        print(f"da3 ({tag}) {name}: reference view {chosen.cpu().tolist()} (golden {c['ref64'].tolist()}, float64 gap {c['gap64']:.3f})")
        assert chosen.cpu().tolist() == c["ref64"].tolist()
    fails = []
    for layer, ((f, t), (f64, t64), (df, dt)) in enumerate(zip(feats, c["out64"], c["d16"])):
        assert f.shape == f64.shape == (B, S, P, 2 * C) and t.shape == t64.shape == (B, S, 2 * C) and f.dtype == t.dtype == torch.float32
        for what, got, ref, d16 in (("features", f, f64, df), ("camera token", t, t64, dt)):
            err, cos = D.rel(got.cpu(), ref), cosine(got.cpu(), ref)
            print(f"da3 ({tag}) {name} out layer {g['cfg']['out_layers'][layer]} {what}: err {err:.4e} d16 {d16:.4e} ratio {err / d16:.3f} cosine {cos:.6f}")
            if not (err <= 2 * d16 and err <= 0.02 and cos >= 0.999):
                fails.append((layer, what, err, d16, cos))
    assert not fails, fails


@pytest.mark.parametrize("tag,name", [("a", "s2"), ("b", "saddle_b2"), ("c", "saddle_b2")])
def test_backbone_is_bit_identical_when_the_batch_is_split(ops, tag, name):
    g, m = model(tag)
    x, cam, strategy = case_inputs(g, name)
    whole = run(m, x, cam, strategy)
    parts = [run(m, x[b:b + 1].contiguous(), cam, strategy) for b in range(x.shape[0])]
    for layer, (f, t) in enumerate(whole):
        assert torch.equal(f, torch.cat([p[layer][0] for p in parts])) and torch.equal(t, torch.cat([p[layer][1] for p in parts])), layer


@pytest.mark.parametrize("tag,name", [("a", "s1"), ("a", "s2"), ("b", "s1"), ("b", "s2"), ("c", "s1"), ("c", "s2")])
def test_fewer_than_three_views_never_select(ops, tag, name):
    g, m = model(tag)
    x, cam, _ = case_inputs(g, name)
    ops.TIMER = timer = ops.KernelTimer()                                    # records every launch by name
    try:
        balanced = run(m, x, cam, "saddle_balanced")
    finally:
        ops.TIMER = None
    assert "da3_tap" in timer.records and "da3_cam_token" in timer.records
    assert m.backbone.pretrained.ref_idx is None and "da3_ref_view" not in timer.records and "da3_view_gather" not in timer.records
    first = run(m, x, cam, "first")
    for (f, t), (f2, t2) in zip(balanced, first):
        assert torch.equal(f, f2) and torch.equal(t, t2)


# ------------------------------------------------------------------------------------------------------------------------ 6. cameras
@pytest.mark.parametrize("tag", list(D.CONFIGS))
def test_camera_decoder_and_pose_decoding_against_the_reference(ops, tag):
    from videogpa_amd.da3 import decode_cameras
    g, m = model(tag)
    cams = g["cameras"]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):     # the decoder computes in fp32 whatever autocast says
        pose = m.cam_dec(cams["cam_in"].cuda())
        ext, intr = decode_cameras(pose, cams["hw"])
    assert pose.dtype == ext.dtype == intr.dtype == torch.float32 and ext.shape == (*pose.shape[:2], 3, 4) and intr.shape == (*pose.shape[:2], 3, 3)
    for what, got in (("pose_enc", pose), ("extrinsics", ext), ("intrinsics", intr)):
        err, d32 = D.rel(got.cpu(), cams[what + "64"]), cams["d32"][what]
        print(f"da3 cameras ({tag}) {what}: err {err:.3e} reference fp32 distance {d32:.3e}")
        assert err <= 8 * d32, (what, err, d32)
    R = ext[..., :3].double().cpu()
    eye = torch.eye(3, dtype=torch.float64).expand_as(R)
    assert float((R @ R.mT - eye).abs().max()) <= 1e-5 and float((torch.linalg.det(R) - 1).abs().max()) <= 1e-5
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(*ext.shape[:2], 1, 4)
    w2c, c2w = torch.cat([ext.double().cpu(), bottom], dim=-2), torch.cat([cams["c2w64"], bottom], dim=-2)
    assert float((w2c @ c2w - torch.eye(4, dtype=torch.float64)).abs().max()) <= 1e-5


def test_pose_decode_against_float64_with_a_closed_field_of_view(ops):
    """the decoding itself restated with torch (tests/da3_ref.py: rotation, invert_rigid, pinhole), float64 against fp32, on random encodings; a field of view of 0
    (what CameraDec's ReLU returns for a negative pre-activation) takes the 1e-6 clamp"""
    from videogpa_amd.da3 import decode_cameras
    g = torch.Generator().manual_seed(77)
    pose = torch.cat([torch.randn(3, 7, 3, generator=g), torch.randn(3, 7, 4, generator=g), 0.3 + torch.rand(3, 7, 2, generator=g)], dim=-1)
    H, W = 294, 518

    def formula(p):          # camera-to-world [R(q) | t] inverted, and the pinhole intrinsics: tests/da3_ref.py
        return D.invert_rigid(torch.cat([D.rotation(p[..., 3:7]), p[..., :3, None]], dim=-1)), D.pinhole(p[..., 7:], (H, W))
    (e64, k64), (e32, k32) = formula(pose.double()), formula(pose)
    ext, intr = decode_cameras(pose.cuda(), (H, W))
    for what, got, r64, r32 in (("extrinsics", ext, e64, e32), ("intrinsics", intr, k64, k32)):
        err, d32 = D.rel(got.cpu(), r64), D.rel(r32, r64)
        print(f"pose decode {what}: err {err:.3e} d32 {d32:.3e}")
        assert err <= 8 * d32, (what, err, d32)
    closed = pose[:1, :2].clone()
    closed[..., 7:] = 0.0
    _, k0 = decode_cameras(closed.cuda(), (H, W))
    assert torch.equal(k0[..., 1, 1].cpu(), torch.full((1, 2), H / 2.0 / 1e-6).float()) and torch.equal(k0[..., 0, 0].cpu(), torch.full((1, 2), W / 2.0 / 1e-6).float())


def test_da3cameras_forward_returns_cameras_for_a_golden_case(ops):
    g, m = model("b")
    x, _, _ = case_inputs(g, "saddle0")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(x)
    B, S = x.shape[:2]
    assert set(out) == {"feats", "pose_enc", "extrinsics", "intrinsics"} and len(out["feats"]) == len(g["cfg"]["out_layers"])
    assert out["pose_enc"].shape == (B, S, 9) and out["extrinsics"].shape == (B, S, 3, 4) and out["intrinsics"].shape == (B, S, 3, 3)
    for k in ("pose_enc", "extrinsics", "intrinsics"):
        assert out[k].dtype == torch.float32 and bool(torch.isfinite(out[k]).all()), k
    assert all(bool(torch.isfinite(f).all()) and bool(torch.isfinite(t).all()) for f, t in out["feats"])
    with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(RuntimeError, match="forward only"):
        m(x)                                                                  # grad mode with trainable parameters


def test_da3cameras_with_bf16_parameters(ops):
    """the other side of the precision contract: bf16 parameters without autocast; the camera decoder still computes in fp32"""
    import copy
    g, m = model("a")
    c = D.load_case(os.path.join(HERE, "golden"), "a", "saddle0")
    x, _, _ = case_inputs(g, "saddle0")
    mb = copy.deepcopy(m).to(torch.bfloat16)
    with torch.no_grad():
        out = mb(x.to(torch.bfloat16))
    assert mb.backbone.pretrained.ref_idx.cpu().tolist() == c["ref64"].tolist()
    f, t = out["feats"][-1]
    f64, t64 = c["out64"][-1]
    assert f.dtype == out["extrinsics"].dtype == out["pose_enc"].dtype == torch.float32
    for what, got, ref in (("features", f, f64), ("camera token", t, t64)):           # the family's cap: bf16 parameters and frames are not the golden's
        err, cos = D.rel(got.cpu(), ref), cosine(got.cpu(), ref)
        print(f"da3 (a) saddle0 with bf16 parameters, last out layer {what}: err {err:.4e} cosine {cos:.6f}")
        assert err <= 0.02 and cos >= 0.999, (what, err, cos)
    assert all(bool(torch.isfinite(out[k]).all()) for k in ("pose_enc", "extrinsics", "intrinsics"))
