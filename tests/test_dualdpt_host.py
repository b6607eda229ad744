"""videogpa_amd.da3.DualDPT / DepthAnything3Net and VideoProcessor(da3_model=...) without a GPU: parameter names and shapes against the reference's
(tests/golden/dualdpt_names.json, written by make_golden_dualdpt.py from DualDPT(2048) on the meta device), the restatement of tests/dualdpt_ref.py
against the reference's goldens, state-dict loading, what is refused, and the new op's failure without a device."""
import json
import os

import pytest
import torch

import da3_ref as D
import dualdpt_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def load_golden():
    """-> (meta, the regenerated state checked against the stored sums)"""
    meta = torch.load(os.path.join(GOLDEN, "dualdpt.pt"))
    assert meta["cfg"] == R.CFG and meta["seed"] == R.SEED
    state = R.seeded_state(meta["shapes"], meta["seed"])
    R.check_state_sums(state, meta["sums"])
    return meta, state


def load_case(name):
    return torch.load(os.path.join(GOLDEN, f"dualdpt_{name}.pt"))


def small_net(head_kwargs=None):
    """da3_ref's configuration (a), all four of its blocks tapped, with a head of dim_in = 128, features = 32"""
    from videogpa_amd.da3 import CameraDec, DepthAnything3Net, DinoV2, DualDPT
    cfg = D.CONFIGS["a"]
    net = DinoV2("vits", [0, 1, 2, 3], cfg["alt_start"], cfg["qknorm_start"], cfg["rope_start"], True,
                 encoder_kwargs=dict(img_size=D.IMG_SIZE, embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"]))
    head = DualDPT(2 * cfg["embed_dim"], **(head_kwargs or dict(features=32, out_channels=[16, 16, 32, 32])))
    return DepthAnything3Net(net, head, CameraDec(2 * cfg["embed_dim"]))


def test_state_dict_names_and_shapes_are_the_reference_s():
    from videogpa_amd.da3 import DualDPT
    names = json.load(open(os.path.join(GOLDEN, "dualdpt_names.json")))
    with torch.device("meta"):
        head = DualDPT(2048)
    own = {k: list(v.shape) for k, v in head.state_dict().items()}
    assert own == names and len(own) == 162
    for level in (0, 1, 2, 3):
        assert own[f"scratch.output_conv2_aux.{level}.2.weight"] == [32] and own[f"scratch.output_conv2_aux.{level}.5.weight"] == [7, 32, 1, 1]
        assert len([k for k in own if k.startswith(f"scratch.output_conv1_aux.{level}.")]) == 10
    meta, state = load_golden()
    small = DualDPT(**R.CFG)
    small.load_state_dict(state, strict=True)
    assert {k: list(v.shape) for k, v in small.state_dict().items()} == meta["shapes"]
    named = DualDPT(32, features=32, out_channels=[16, 16, 32, 32], head_names=("dist", "beam"))
    assert (named.head_main, named.head_aux) == ("dist", "beam")


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_reproduces_the_reference_goldens(name):
    """float64 against out64 to rounding; fp32 within the class of the stored d32, by the project's measure of a class (8 x d32,
    tests/test_gpu_vggt_heads.py): the same operations in the same dtype, only library code paths and summation orders differ"""
    _, state = load_golden()
    c = load_case(name)
    H, W = c["hw"]
    assert all(torch.equal(a, b) for a, b in zip(R.features(name), c["feats"]))
    with torch.no_grad():
        o64 = R.head({k: v.double() for k, v in state.items()}, [f.double() for f in c["feats"]], H, W)
        o32 = R.head(state, c["feats"], H, W)
        main_only = R.head(state, c["feats"], H, W, aux=False)
    assert tuple(main_only) == ("depth", "depth_conf") and torch.equal(main_only["depth"], o32["depth"])
    for k in R.OUTPUTS:
        assert o64[k].shape == c["out64"][k].shape and o64[k].dtype == torch.float64
        e64, e32, d32 = R.rel(o64[k], c["out64"][k]), R.rel(o32[k], c["out64"][k]), c["d32"][k]
        print(f"{name} {k}: float64 {e64:.2e} fp32 {e32:.2e} d32 {d32:.2e}")
        assert e64 <= 1e-12, (k, e64)
        assert e32 <= 8 * d32, (k, e32, d32)
        lo, hi = c["logit_range"][k]
        assert lo < -1.0 and hi > 1.0, (k, lo, hi)                       # the goldens pin something: several units, both signs


def test_depthanything3net_loads_a_full_state_dict():
    m = small_net()
    own = {k: torch.randn_like(v) for k, v in m.state_dict().items()}
    assert all(k.startswith(("backbone.pretrained.", "head.", "cam_dec.")) for k in own) and sum(k.startswith("head.") for k in own) == 162
    foreign = {"cam_enc.token_norm.bias": torch.zeros(2), "gs_head.a": torch.zeros(1), "gs_adapter.q": torch.zeros(1)}
    assert m.load_state_dict({**own, **foreign}) == ["cam_enc.", "gs_adapter.", "gs_head."]
    assert all(torch.equal(v, own[k]) for k, v in m.state_dict().items())
    m2 = small_net()
    assert m2.load_state_dict({"model." + k: v for k, v in {**own, "cam_enc.x": torch.zeros(1)}.items()}) == ["cam_enc."]
    assert all(torch.equal(v, own[k]) for k, v in m2.state_dict().items())
    assert m2.load_state_dict(own) == []
    missing = dict(own)
    del missing["head.scratch.output_conv2_aux.3.2.weight"]
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict(missing)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        m.load_state_dict({**own, "heads.stray": torch.zeros(1)})
    with pytest.raises(ValueError, match="strictly"):
        m.load_state_dict(own, strict=False)


def test_presets_and_local_checkpoints(tmp_path):
    from videogpa_amd.da3 import DepthAnything3Net, DualDPT
    assert DepthAnything3Net.presets() == ["da3-base", "da3-large", "da3-small"]
    with pytest.raises(ValueError, match="unknown preset"):
        DepthAnything3Net.from_preset("da3-giant")                       # vitg: not offered
    names = json.load(open(os.path.join(GOLDEN, "da3_names.json")))
    head_names = json.load(open(os.path.join(GOLDEN, "dualdpt_names.json")))
    with torch.device("meta"):
        large = DepthAnything3Net.from_preset("da3-large")
        small = DepthAnything3Net.from_preset("da3-small")
    want = {**{"backbone." + k: v for k, v in names["backbone"].items()}, **{"head." + k: v for k, v in head_names.items()},
            **{"cam_dec." + k: v for k, v in names["cam_dec"].items()}}
    assert {k: list(v.shape) for k, v in large.state_dict().items()} == want           # a DA3-Large checkpoint's key set loads by name
    assert isinstance(small.head, DualDPT) and small.head.norm.normalized_shape == (768,) and small.cam_dec.fc_t.in_features == 768
    with pytest.raises(FileNotFoundError, match="local checkpoints only"):
        DepthAnything3Net.from_pretrained(tmp_path / "nowhere")
    with pytest.raises(FileNotFoundError, match="neither model.safetensors nor model.pt"):
        DepthAnything3Net.from_pretrained(tmp_path)


def test_what_is_not_built_raises():
    from videogpa_amd.da3 import DualDPT
    kw = dict(features=32, out_channels=[16, 16, 32, 32])
    for bad in (dict(down_ratio=2), dict(activation="linear"), dict(conf_activation="sigmoid"), dict(aux_pyramid_levels=3), dict(aux_out1_conv_num=3)):
        with pytest.raises(NotImplementedError, match="DualDPT on the HIP path"):
            DualDPT(32, **kw, **bad)
    for bad in (dict(dim_in=40, **kw), dict(dim_in=32, features=48, out_channels=[16, 16, 32, 32]), dict(dim_in=32, features=32, out_channels=[16, 16, 32, 24])):
        with pytest.raises(NotImplementedError, match="multiples of"):
            DualDPT(**bad)
    with pytest.raises(TypeError):
        DualDPT(32, 14)                                                   # everything but dim_in is keyword-only, as upstream
    m = small_net()
    x = torch.zeros(1, 2, 3, 42, 56)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="cam_enc"):
            m(x, extrinsics=torch.zeros(1, 2, 4, 4), intrinsics=torch.zeros(1, 2, 3, 3))
        with pytest.raises(NotImplementedError, match="cam_enc"):
            m(x, intrinsics=torch.zeros(1, 2, 3, 3))
        with pytest.raises(NotImplementedError, match="infer_gs"):
            m(x, infer_gs=True)
        with pytest.raises(NotImplementedError, match="use_ray_pose"):
            m(x, use_ray_pose=True)
        with pytest.raises(NotImplementedError, match="export_feat_layers"):
            m(x, export_feat_layers=[1])
        feats = [(torch.zeros(1, 2, 12, 128), None)] * 4
        with pytest.raises(ValueError, match="patch tokens do not make"):
            m.head(feats, 42, 70, patch_start_idx=0)
        with pytest.raises(ValueError, match="multiples of 14"):
            m.head(feats, 43, 56, patch_start_idx=0)
    with pytest.raises(RuntimeError, match="forward only"):
        m.head([(torch.zeros(1, 2, 12, 128), None)] * 4, 42, 56, patch_start_idx=0)


def test_video_processor_refuses_frames_it_would_have_to_resize():
    from videogpa_amd.process_video import VideoProcessor
    vp = VideoProcessor({}, backbone="da3", da3_model=lambda x, aux: None, device="cpu")
    assert vp.backbone_fn is not None
    with pytest.raises(ValueError, match="multiples of 14.*input resizing"):
        vp._run_da3(None, torch.zeros(3, 43, 56, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8 frames"):
        vp._run_da3(None, torch.zeros(3, 42, 56, 3))
    own = lambda frames: None
    assert VideoProcessor({}, backbone="da3", da3_model=object(), backbone_fn=own).backbone_fn is own


def test_ops_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from videogpa_amd import ops
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dualdpt_aux_tail_f32(z(1, 5, 7, 16), z(3, 3, 16, 32), z(32), torch.ones(32), z(32), 1e-5, z(7, 32), z(7))
    _, state = load_golden()
    from videogpa_amd.da3 import DualDPT
    head = DualDPT(**R.CFG)
    head.load_state_dict(state)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        head([(f, None) for f in R.features("B")], 28, 42, patch_start_idx=0)
    m = small_net().to(torch.bfloat16)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 2, 3, 42, 56, dtype=torch.bfloat16))


def test_state_dict_order_is_the_one_before_the_shared_head():
    """`state_dict()` key ORDER (the tests seed states from it) and shapes of both DPT heads and of VGGT at the reduced sizes against
    tests/golden/state_dict_order.json: the `[[key, shape], ...]` lists of `state_dict().items()` as the commit before videogpa_amd/dpt.py gave them
    (written from an export of that commit with the constructor arguments used below; 585 entries, hence a fixture and not a literal).  The three
    presets on the meta device: backbone, head, camera decoder in that order, the head's names in the fixture's order, and for DA3-Large names and
    shapes equal to the reference's lists (tests/golden/da3_names.json, dualdpt_names.json; those files are sorted, so they bound the set only)."""
    import test_vggt_heads_host as V
    from videogpa_amd.da3 import DepthAnything3Net, DualDPT
    from videogpa_amd.vggt import DPTHead, VGGT
    want = json.load(open(os.path.join(GOLDEN, "state_dict_order.json")))
    ordered = lambda m: [[k, list(v.shape)] for k, v in m.state_dict().items()]
    small = dict(aggregator_kwargs=dict(depth=4, num_heads=1), camera_kwargs=dict(trunk_depth=1, num_heads=2), dpt_kwargs=V.DPT_CFG_64)
    got = {"DPTHead.depth": DPTHead(output_dim=2, activation="exp", **V.DPT_CFG), "DPTHead.point": DPTHead(output_dim=4, activation="inv_log", **V.DPT_CFG),
           "DualDPT": DualDPT(**R.CFG), "VGGT": VGGT(img_size=28, patch_size=14, embed_dim=64, patch_embed="conv", **small)}
    assert sorted(got) == sorted(want)
    for name, module in got.items():
        assert ordered(module) == want[name], name
    meta, _ = load_golden()
    assert dict(want["DualDPT"]) == meta["shapes"]
    heads = torch.load(os.path.join(GOLDEN, "vggt_heads.pt"))["state"]
    assert dict(want["DPTHead.depth"]) == {k: list(v.shape) for k, v in heads.items()}
    names, head_names = json.load(open(os.path.join(GOLDEN, "da3_names.json"))), json.load(open(os.path.join(GOLDEN, "dualdpt_names.json")))
    for preset in DepthAnything3Net.presets():
        with torch.device("meta"):
            keys = ordered(DepthAnything3Net.from_preset(preset))
        groups = [k.split(".")[0] for k, _ in keys]
        assert [g for i, g in enumerate(groups) if i == 0 or g != groups[i - 1]] == ["backbone", "head", "cam_dec"], preset
        assert [k[len("head."):] for k, _ in keys if k.startswith("head.")] == [k for k, _ in want["DualDPT"]], preset
        if preset == "da3-large":
            assert dict(keys) == {**{"backbone." + k: v for k, v in names["backbone"].items()}, **{"head." + k: v for k, v in head_names.items()},
                                  **{"cam_dec." + k: v for k, v in names["cam_dec"].items()}}
