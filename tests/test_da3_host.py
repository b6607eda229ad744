"""videogpa_amd.da3 without a GPU: parameter names and shapes against the reference's (tests/golden/da3_names.json, written by make_golden_da3.py from
DinoV2("vitl", [11, 15, 19, 23], 8, 8, 8, True) and CameraDec(2048)), state-dict loading, what is refused, and the ops' failure without a device."""
import json
import os

import pytest
import torch

import da3_ref as D

HERE = os.path.dirname(os.path.abspath(__file__))


def small(tag="a"):
    from videogpa_amd.da3 import CameraDec, DA3Cameras, DinoV2
    cfg = D.CONFIGS[tag]
    net = DinoV2("vits", cfg["out_layers"], cfg["alt_start"], cfg["qknorm_start"], cfg["rope_start"], True,
                 encoder_kwargs=dict(img_size=D.IMG_SIZE, embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"]))
    return DA3Cameras(net, CameraDec(2 * cfg["embed_dim"]))


def test_state_dict_names_and_shapes_are_the_reference_s():
    from videogpa_amd.da3 import CameraDec, DinoV2
    names = json.load(open(os.path.join(HERE, "golden", "da3_names.json")))
    with torch.device("meta"):
        net, dec = DinoV2("vitl", [11, 15, 19, 23], 8, 8, 8, True), CameraDec(2048)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == names["backbone"]
    assert {k: list(v.shape) for k, v in dec.state_dict().items()} == names["cam_dec"]
    assert net.pretrained.patch_start_idx == 1 and net.pretrained.norm.eps == 1e-5 and net.pretrained.blocks[0].norm1.eps == 1e-6
    assert "pretrained.blocks.7.attn.q_norm.weight" not in names["backbone"] and "pretrained.blocks.8.attn.q_norm.weight" in names["backbone"]


def test_strict_round_trip_and_the_stored_state():
    from videogpa_amd.da3 import CameraDec
    m = small("a")
    state = torch.load(os.path.join(HERE, "golden", "da3_a_state.pt"))
    dec_state = torch.load(os.path.join(HERE, "golden", "da3_a_cam_dec_state.pt"))
    g = torch.load(os.path.join(HERE, "golden", "da3_a.pt"))
    regenerated = D.seeded_state(g["shapes"], g["cfg"]["seed"])
    assert set(regenerated) == set(state) and all(torch.equal(regenerated[k], state[k]) for k in state)
    assert all(torch.equal(v, dec_state[k]) for k, v in D.cam_dec_state(g["cam_dec_shapes"], g["cfg"]["seed"]).items())
    m.backbone.pretrained.load_state_dict(state, strict=True)                       # the reference's names, strictly
    m.cam_dec.load_state_dict(dec_state, strict=True)
    saved = m.state_dict()
    again = small("a")
    assert again.load_state_dict(saved) == []
    assert all(torch.equal(v, saved[k]) for k, v in again.state_dict().items()) and set(saved) == set(again.state_dict())
    assert set(CameraDec(8).state_dict()) == set(dec_state)


def test_da3cameras_loads_a_depthanything3net_state_dict():
    m = small("a")
    own = {k: torch.randn_like(v) for k, v in m.state_dict().items()}
    assert all(k.startswith(("backbone.pretrained.", "cam_dec.")) for k in own)
    foreign = {"head.scratch.x.weight": torch.zeros(2), "cam_enc.token_norm.bias": torch.zeros(2), "gs_head.a": torch.zeros(1)}
    assert m.load_state_dict({**own, **foreign}) == ["cam_enc.", "gs_head.", "head."]
    assert all(torch.equal(v, own[k]) for k, v in m.state_dict().items())
    m2 = small("a")
    assert m2.load_state_dict({"model." + k: v for k, v in {**own, "gs_adapter.q": torch.zeros(1)}.items()}) == ["gs_adapter."]
    assert all(torch.equal(v, own[k]) for k, v in m2.state_dict().items())
    with pytest.raises(RuntimeError, match="Unexpected key"):
        m.load_state_dict({**own, "heads.stray": torch.zeros(1)})                   # not one of the four prefixes
    with pytest.raises(RuntimeError, match="Unexpected key"):
        m.load_state_dict({**own, "track_head.w": torch.zeros(1)})
    missing = dict(own)
    del missing["cam_dec.fc_t.weight"]
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict(missing)
    with pytest.raises(ValueError, match="strictly"):
        m.load_state_dict(own, strict=False)


def test_what_is_not_built_raises():
    from videogpa_amd.da3 import DinoV2
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        DinoV2("vitg", [19, 27, 33, 39], 13, 13, 13, True)
    with pytest.raises(AssertionError):
        DinoV2("vitx", [1])
    with pytest.raises(TypeError):
        DinoV2("vits", [11], 4, 4, 4, True, alt_strat=4)                            # a misspelt option is refused, not ignored
    m = small("a")
    x = torch.zeros(1, 1, 3, 14, 14)
    with pytest.raises(NotImplementedError, match="export_feat_layers"):
        m.backbone(x, export_feat_layers=[3])
    with pytest.raises(ValueError, match="Unknown reference view selection strategy"):
        m.backbone(x, ref_view_strategy="last")
    with pytest.raises(NotImplementedError, match="cat_token"):
        DinoV2("vits", [11], 4, 4, 4, False)
    with pytest.raises(NotImplementedError, match="RoPE without QK-norm"):
        DinoV2("vits", [11], 4, 6, 4, True, encoder_kwargs=dict(embed_dim=64, depth=8, num_heads=1, img_size=70))


def test_ops_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from videogpa_amd import ops
    from videogpa_amd.da3 import decode_cameras
    x = torch.zeros(1, 3, 2, 64)
    ref = torch.zeros(1, dtype=torch.int32)
    for call in (lambda: ops.da3_ref_view(x), lambda: ops.da3_view_gather(x, ref), lambda: ops.da3_cam_token(x, torch.zeros(1, 2, 64), per_view=False),
                 lambda: ops.da3_tap(x, x, torch.ones(64), torch.zeros(64)), lambda: ops.da3_pose_decode(torch.zeros(2, 9), (14, 14)),
                 lambda: decode_cameras(torch.zeros(1, 2, 9), (14, 14))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    m = small("a").to(torch.bfloat16)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 2, 3, 42, 56, dtype=torch.bfloat16))
