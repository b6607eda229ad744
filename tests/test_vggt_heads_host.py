"""The VGGT heads without a GPU: the restatement the GPU tests compare against (tests/vggt_heads_ref.py) is pinned on the float64 goldens of
the reference modules (tests/golden/make_golden_vggt_heads.py), the modules' state-dict names equal the reference's, the C ABI declares the
new entry points in all three places, and everything fails loudly where there is no device."""
import os
import re

import pytest
import torch

import vggt_heads_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DPT_CFG = dict(dim_in=32, features=32, out_channels=[16, 16, 32, 32], intermediate_layer_idx=[0, 1, 2, 3])
ENTRIES = {"vgpa_conv3x3_f32": 14, "vgpa_conv1x1_f32": 8, "vgpa_dpt_tail_f32": 18, "vgpa_upsample_bilinear_ac_f32": 11, "vgpa_attn_small_f32": 13}


def load_goldens():
    g = torch.load(os.path.join(GOLDEN, "vggt_heads.pt"))
    gp = torch.load(os.path.join(GOLDEN, "vggt_heads_point.pt"))
    gc = torch.load(os.path.join(GOLDEN, "vggt_heads_camera.pt"))
    point_state = dict(g["state"])
    point_state.update(gp["state_delta"])
    return g, gp, gc, point_state


def test_restatement_matches_the_float64_goldens():
    g, gp, gc, point_state = load_goldens()
    hw, psi = tuple(int(v) for v in g["image_hw"]), int(g["patch_start_idx"])
    toks = [t.double() for t in g["tokens"]]
    for state, gold, act in ((g["state"], g, "exp"), (point_state, gp, "inv_log")):
        p, c = R.dpt_head({k: v.double() for k, v in state.items()}, toks, hw, psi, activation=act)
        assert p.shape == gold["preds64"].shape and c.shape == gold["conf64"].shape
        assert R.rel_err(p, gold["preds64"]) < 1e-9 and R.rel_err(c, gold["conf64"]) < 1e-9
    pose = torch.stack(R.camera_head({k: v.double() for k, v in gc["state"].items()}, [gc["tokens"].double()], num_heads=2, trunk_depth=2))
    assert R.rel_err(pose, gc["pose64"]) < 1e-9


def test_goldens_exercise_both_activation_branches_and_chunking():
    g, gp, gc, _ = load_goldens()
    pre = torch.log(g["preds64"])
    assert float(pre.min()) < -2 and float(pre.max()) > 2                      # exp on both sides of 1, several units wide
    assert float(gp["preds64"].min()) < -5 and float(gp["preds64"].max()) > 5  # inv_log on both signs
    for gold in (g, gp):                                                        # the reference's own chunking changes nothing beyond fp32 noise
        assert R.rel_err(gold["chunk2.preds32"], gold["preds64"]) < 1e-4
        assert 1e-9 < R.rel_err(gold["preds32"], gold["preds64"]) < 1e-4        # fp32 and float64 evaluations both present and distinct
    assert gc["pose64"].shape == (4, 1, 3, 9) and bool((gc["pose64"][..., 7:] >= 0).all())


def test_state_dict_names_equal_the_reference():
    from videogpa_amd.vggt import CameraHead, DPTHead
    g, gp, gc, point_state = load_goldens()
    depth = DPTHead(output_dim=2, activation="exp", **DPT_CFG)
    point = DPTHead(output_dim=4, activation="inv_log", **DPT_CFG)
    cam = CameraHead(dim_in=64, trunk_depth=2, num_heads=2)
    for mod, state in ((depth, g["state"]), (point, point_state), (cam, gc["state"])):
        own = mod.state_dict()
        assert set(own) == set(state)
        assert all(own[k].shape == state[k].shape for k in state)
        mod.load_state_dict(state, strict=True)
    names = set(depth.state_dict())
    for k in ("scratch.refinenet1.resConfUnit1.conv1.weight", "projects.3.bias", "resize_layers.0.weight", "resize_layers.3.bias",
              "scratch.output_conv2.0.weight", "scratch.output_conv2.2.bias", "scratch.layer4_rn.weight", "norm.weight"):
        assert k in names, k
    assert not any(k.startswith("scratch.refinenet4.resConfUnit1") for k in names)


def test_vggt_surface_and_unsupported_arguments():
    from videogpa_amd.vggt import DPTHead, VGGT
    small = dict(aggregator_kwargs=dict(depth=4, num_heads=1), camera_kwargs=dict(trunk_depth=1, num_heads=2), dpt_kwargs=DPT_CFG_64)
    m = VGGT(img_size=28, patch_size=14, embed_dim=64, patch_embed="conv", **small)
    keys = set(m.state_dict())
    assert any(k.startswith("aggregator.frame_blocks.0.") for k in keys) and any(k.startswith("camera_head.trunk.0.attn.qkv") for k in keys)
    assert any(k.startswith("depth_head.scratch.") for k in keys) and any(k.startswith("point_head.projects.") for k in keys)
    sd = dict(m.state_dict())
    sd["track_head.tracker.something"] = torch.zeros(3)
    m.load_state_dict(sd, strict=True)                                          # track head keys are dropped
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 2, 3, 28, 28), query_points=torch.zeros(1, 2))
    with pytest.raises(NotImplementedError):
        VGGT(img_size=28, embed_dim=64, patch_embed="conv", enable_track=True, **small)
    for bad in (dict(feature_only=True), dict(down_ratio=2), dict(activation="norm_exp")):
        with pytest.raises(NotImplementedError):
            DPTHead(**{**DPT_CFG, **bad})
    assert VGGT(img_size=28, embed_dim=64, patch_embed="conv", enable_camera=False, enable_point=False, **small).point_head is None


DPT_CFG_64 = dict(features=32, out_channels=[16, 16, 32, 32], intermediate_layer_idx=[0, 1, 2, 3])


def test_cabi_declares_the_head_entries():
    from videogpa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "videogpa_hip.h")).read()
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name), name
    # argument checks are host code: they answer without a device
    assert lib.vgpa_conv3x3_f32(None, None, None, None, None, None, 1, 5, 7, 16, 16, 1, 0, None) == -1
    assert lib.vgpa_attn_small_f32(None, None, None, 0, 0, 0, None, 1, 1, 129, 128, 1.0, None) == -1


def test_uv_embed_tables_are_the_separable_halves_of_the_embedding():
    from videogpa_amd import ops
    for (w, h, c, aspect) in ((4, 3, 16, 56 / 42), (56, 42, 16, 56 / 42), (7, 7, 32, 1.0)):
        xt, yt = ops.uv_embed_tables(w, h, c, aspect, "cpu")
        full = R.uv_embed(w, h, c, aspect, torch.float32)                       # [c, h, w]
        assert torch.equal(full[: c // 2], xt.t()[:, None, :].expand(c // 2, h, w))
        assert torch.equal(full[c // 2:], yt.t()[:, :, None].expand(c // 2, h, w))


def test_heads_fail_loudly_without_gpu_and_with_gradients():
    from videogpa_amd import ops
    from videogpa_amd.vggt import CameraHead, DPTHead
    g, _, gc, _ = load_goldens()
    hw, psi = tuple(int(v) for v in g["image_hw"]), int(g["patch_start_idx"])
    head = DPTHead(output_dim=2, activation="exp", **DPT_CFG)
    images = torch.zeros(1, 3, 3, *hw)
    with pytest.raises(RuntimeError, match="forward only"):
        head(g["tokens"], images, psi)
    with pytest.raises(RuntimeError, match="forward only"):
        CameraHead(dim_in=64, trunk_depth=2, num_heads=2)([gc["tokens"]])
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            head(g["tokens"], images, psi)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            CameraHead(dim_in=64, trunk_depth=2, num_heads=2)([gc["tokens"]])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.conv3x3_f32(torch.zeros(1, 5, 7, 16), torch.zeros(3, 3, 16, 16))
