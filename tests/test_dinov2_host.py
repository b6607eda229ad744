"""The DINOv2 patch embedding without a GPU: Aggregator / VGGT construct with their default patch_embed and carry the reference's names and shapes
(tests/golden/vggt_dinov2_vitl14_reg_names.json, made by tests/golden/make_golden_dinov2.py from the reference), the position table equals the
reference's on the CPU, VGGT.from_pretrained reads a local checkpoint, the C ABI declares vgpa_dino_embed in all three places and its argument checks
answer without a device, and the goldens are what the GPU tests need them to be."""
import json
import os
import re

import pytest
import torch

import dinov2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KEYS = ("x_norm_patchtokens", "x_norm_clstoken", "x_norm_regtokens", "x_prenorm")


def gold(name):
    return torch.load(os.path.join(GOLDEN, name))


def reduced(cfg, **kw):
    from videogpa_amd.vggt import DinoVisionTransformer
    return DinoVisionTransformer(img_size=cfg["img_size"], patch_size=cfg["patch_size"], embed_dim=cfg["embed_dim"], depth=cfg["depth"],
                                 num_heads=cfg["num_heads"], mlp_ratio=4, num_register_tokens=cfg["num_register_tokens"],
                                 **{**dict(interpolate_antialias=True, interpolate_offset=0.0, block_chunks=0, init_values=1.0), **kw})


def test_default_aggregator_and_vggt_construct_with_the_reference_names():
    from videogpa_amd.vggt import VGGT, Aggregator, DinoVisionTransformer
    want = json.load(open(os.path.join(GOLDEN, "vggt_dinov2_vitl14_reg_names.json")))
    assert len(want) == 344 and want["aggregator.patch_embed.pos_embed"] == [1, 1370, 1024]
    with torch.device("meta"):
        agg, model = Aggregator(patch_embed="dinov2_vitl14_reg"), VGGT()
    assert isinstance(agg.patch_embed, DinoVisionTransformer) and isinstance(model.aggregator.patch_embed, DinoVisionTransformer)
    for sd, prefix in ((agg.state_dict(), "aggregator."), (model.state_dict(), "")):
        got = {prefix + k: list(v.shape) for k, v in sd.items() if (prefix + k).startswith("aggregator.patch_embed.")}
        assert got == want, (sorted(set(got) ^ set(want))[:5], [k for k in got if k in want and got[k] != want[k]][:5])
    pe = model.aggregator.patch_embed
    assert not pe.mask_token.requires_grad and pe.norm.eps == 1e-6 and pe.blocks[0].norm1.eps == 1e-6
    assert pe.interpolate_antialias is True and pe.interpolate_offset == 0.0 and float(pe.blocks[0].ls1.gamma.shape[0]) == 1024
    assert "aggregator.camera_token" in model.state_dict() and not any(k.startswith("track_head") for k in model.state_dict())


@pytest.mark.parametrize("name,dim,depth,heads", [("dinov2_vits14_reg", 384, 12, 6), ("dinov2_vitb14_reg", 768, 12, 12), ("dinov2_vitg2_reg", 1536, 40, 24)])
def test_the_other_named_backbones(name, dim, depth, heads):
    from videogpa_amd.vggt import Aggregator
    with torch.device("meta"):
        agg = Aggregator(embed_dim=dim, depth=1, num_heads=heads, patch_embed=name)
    pe = agg.patch_embed
    assert (pe.embed_dim, len(pe.blocks), pe.num_heads, pe.num_register_tokens, pe.patch_size) == (dim, depth, heads, 4, 14)
    assert tuple(pe.pos_embed.shape) == (1, 1 + 37 * 37, dim)


def test_conv_and_module_patch_embed_keep_working_and_unknown_names_raise():
    from videogpa_amd.vggt import Aggregator, PatchEmbed
    a = Aggregator(img_size=28, embed_dim=64, depth=1, num_heads=1, patch_embed="conv")
    assert isinstance(a.patch_embed, PatchEmbed)
    mod = torch.nn.Identity()
    assert Aggregator(img_size=28, embed_dim=64, depth=1, num_heads=1, patch_embed=mod).patch_embed is mod
    with pytest.raises(KeyError):
        Aggregator(img_size=28, embed_dim=64, depth=1, num_heads=1, patch_embed="dinov2_vitx14")
    with pytest.raises(ValueError):
        with torch.device("meta"):
            Aggregator(embed_dim=64, depth=1, num_heads=1, patch_embed="dinov2_vits14_reg")       # 384 wide


def test_reduced_state_dict_equals_the_golden_and_loads_strictly():
    g, state = gold("vggt_dinov2_a.pt"), gold("vggt_dinov2_a_state.pt")
    m = reduced(g["cfg"])
    own = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert own == {k: list(v.shape) for k, v in state.items()} == g["shapes"]
    m.load_state_dict(state, strict=True)
    R.check_state_sums(R.seeded_state({k: v.shape for k, v in m.state_dict().items()}, g["cfg"]["seed"]), g["sums"])     # (a) is the recipe too
    gb = gold("vggt_dinov2_b.pt")
    mb = reduced(gb["cfg"])
    assert {k: list(v.shape) for k, v in mb.state_dict().items()} == gb["shapes"]
    sb = R.seeded_state({k: v.shape for k, v in mb.state_dict().items()}, gb["cfg"]["seed"])
    R.check_state_sums(sb, gb["sums"])
    mb.load_state_dict(sb, strict=True)
    bad = dict(sb)
    bad["cls_token"] = bad["cls_token"] + 1e-3
    with pytest.raises(AssertionError, match="drifted"):
        R.check_state_sums(bad, gb["sums"])


def test_unsupported_arguments_raise():
    from videogpa_amd.vggt import DinoVisionTransformer
    cfg = gold("vggt_dinov2_a.pt")["cfg"]
    for kw in (dict(block_chunks=1), dict(ffn_layer="swiglufused"), dict(ffn_layer="identity"), dict(qk_norm=True), dict(init_values=None)):
        with pytest.raises(NotImplementedError):
            reduced(cfg, **kw)
    with pytest.raises(NotImplementedError):
        DinoVisionTransformer()                                   # the reference's own default is block_chunks=1
    with pytest.raises(NotImplementedError):
        reduced(dict(cfg, embed_dim=96))                          # head_dim 96
    m = reduced(cfg).to(torch.bfloat16)
    x = torch.zeros(1, 3, 70, 70, dtype=torch.bfloat16)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="masks"):
            m(x, masks=torch.zeros(1, 25, dtype=torch.bool))
        with pytest.raises(NotImplementedError, match="list"):
            m([x, x])
        with pytest.raises(AssertionError, match="multiple of the patch size"):
            m(torch.zeros(1, 3, 70, 72, dtype=torch.bfloat16))
        with pytest.raises(RuntimeError, match="bf16"):
            reduced(cfg)(x.float())                               # fp32 parameters outside autocast
        md = reduced(cfg, drop_path_rate=0.1).to(torch.bfloat16).train()
        with pytest.raises(NotImplementedError, match="stochastic depth"):
            md(x)
    with pytest.raises(RuntimeError, match="forward only"):       # parameters require grad and grad mode is on
        m(x)
    if not torch.cuda.is_available():
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x)


def test_position_table_equals_the_reference_on_the_cpu():
    g, state = gold("vggt_dinov2_a.pt"), gold("vggt_dinov2_a_state.pt")
    m = reduced(g["cfg"])
    m.load_state_dict(state, strict=True)
    for name, c in g["cases"].items():
        h, w = (int(v) for v in name.split("x"))
        t = m.pos_table(h, w)
        assert t.shape == c["pos"].shape == (1, 1 + (h // 14) * (w // 14), 64)
        assert float((t.detach() - c["pos"]).abs().max()) <= 1e-6 * float(c["pos"].abs().max()), name
        assert (t is m.pos_embed) == (name == "70x70")
        x = torch.empty(1, t.shape[1], 64, dtype=torch.bfloat16)
        assert m.interpolate_pos_encoding(x, h, w).dtype == (torch.float32 if name == "70x70" else torch.bfloat16)
        assert torch.equal(R.pos_table(state["pos_embed"], h // 14, w // 14), c["pos"])
    assert not torch.equal(g["cases"]["42x70"]["pos"][0, 1:6], g["cases"]["98x56"]["pos"][0, 1:6])
    first = m.pos_table(42, 70)
    assert m.pos_table(42, 70) is first                                               # cached ...
    with torch.no_grad():
        m.pos_embed.mul_(2.0)
    again = m.pos_table(42, 70)
    assert again is not first and torch.allclose(again, 2.0 * first, rtol=1e-6, atol=0)       # ... per pos_embed._version
    mo = reduced(g["cfg"], interpolate_offset=0.1, interpolate_antialias=False)              # the scale_factor form survives
    mo.load_state_dict(state, strict=True)
    assert torch.equal(mo.pos_table(42, 70).detach(), R.pos_table(state["pos_embed"], 3, 5, antialias=False, offset=0.1))


def test_pack_patch_weight_layout():
    from videogpa_amd import ops
    w = torch.randn(32, 3, 14, 14)
    p = ops.pack_patch_weight(w)
    assert p.shape == (592, 32) and p.dtype == torch.float32 and p.is_contiguous()
    assert torch.equal(p[:588], w.reshape(32, 588).t()) and not p[588:].any()
    assert ops.pack_patch_weight(torch.randn(64, 3, 16, 16)).shape == (768, 64)


def test_from_pretrained_round_trip(tmp_path):
    from safetensors.torch import save_file
    from videogpa_amd.vggt import VGGT
    kw = dict(img_size=28, patch_size=14, embed_dim=384, patch_embed="dinov2_vits14_reg", aggregator_kwargs=dict(depth=1, num_heads=6),
              camera_kwargs=dict(trunk_depth=1, num_heads=6), dpt_kwargs=dict(features=32, out_channels=[16, 16, 32, 32], intermediate_layer_idx=[0, 0, 0, 0]))
    torch.manual_seed(0)
    src = VGGT(**kw)
    state = {k: v.detach().clone() for k, v in src.state_dict().items()}
    state["track_head.tracker.weight"] = torch.zeros(3)                                 # a released checkpoint carries the track head: dropped
    d1, d2 = tmp_path / "st", tmp_path / "pt"
    d1.mkdir(), d2.mkdir()
    save_file(state, str(d1 / "model.safetensors"))
    torch.save(state, str(d2 / "model.pt"))
    for path in (d1, d2, d2 / "model.pt", str(d1 / "model.safetensors")):
        m = VGGT.from_pretrained(path, **kw)
        assert not m.training and all(torch.equal(v, state[k]) for k, v in m.state_dict().items())
    with pytest.raises(FileNotFoundError, match="local"):
        VGGT.from_pretrained("facebook/VGGT-1B", **kw)                                   # a hub name is not looked up anywhere
    with pytest.raises(FileNotFoundError):
        VGGT.from_pretrained(tmp_path, **kw)
    bad = dict(state)
    bad.pop("aggregator.patch_embed.cls_token")
    torch.save(bad, str(d2 / "model.pt"))
    with pytest.raises(RuntimeError, match="cls_token"):
        VGGT.from_pretrained(d2, **kw)


def test_c_abi_declares_dino_embed_and_its_argument_checks_need_no_device():
    from videogpa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "videogpa_hip.h")).read()
    lib = _lib.load()
    assert re.search(r"\bvgpa_dino_embed\s*\(", hdr)
    assert "vgpa_dino_embed" in _lib.SIGNATURES and len(_lib.SIGNATURES["vgpa_dino_embed"][1]) == 17 and hasattr(lib, "vgpa_dino_embed")
    A = 0x10000                                                    # never dereferenced: every call below is refused by the host checks

    def call(img=A, in_dt=0, w=A, k=592, bias=A, cls=A, reg=A, pos=A, out=A, out_dt=1, N=2, H=70, W=42, p=14, C=64, R=4):
        return lib.vgpa_dino_embed(img, in_dt, w, k, bias, cls, reg, pos, out, out_dt, N, H, W, p, C, R, None)
    for null in ("img", "w", "bias", "cls", "reg", "pos", "out"):
        assert call(**{null: None}) == -1, null
    assert call(H=71) == -1 and call(W=43) == -1                   # not multiples of the patch
    assert call(C=48) == -1 and call(C=0) == -1                    # channels in multiples of 32
    assert call(k=588) == -1 and call(k=608) == -1 and call(p=16) == -1      # packed K is 3 p^2 rounded up to 16
    for mis in ("img", "w", "pos", "out"):
        assert call(**{mis: A + 4}) == -1, mis
    assert call(in_dt=2) == -1 and call(out_dt=-1) == -1 and call(N=0) == -1 and call(R=-1) == -1


def test_c_abi_declares_stream_ln_and_its_argument_checks_need_no_device():
    from videogpa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "videogpa_hip.h")).read()
    lib = _lib.load()
    assert re.search(r"\bvgpa_stream_ln_f32\s*\(", hdr) and len(_lib.SIGNATURES["vgpa_stream_ln_f32"][1]) == 12 and hasattr(lib, "vgpa_stream_ln_f32")
    A, B = 0x10000, 0x20000

    def call(x=A, y=A, gamma=A, w=A, b=A, x_new=B, n=B, dt=1, M=4, D=64):
        return lib.vgpa_stream_ln_f32(x, y, gamma, w, b, x_new, n, dt, M, D, 1e-6, None)
    assert call(x=None) == -1 and call(y=None) == -1 and call(gamma=None) == -1 and call(x_new=None) == -1      # the add needs y, gamma and x_new together
    assert call(w=None) == -1 and call(b=None) == -1 and call(n=None) == -1                                      # the norm needs ln_w, ln_b and n together
    assert call(y=None, gamma=None, x_new=None, w=None, b=None, n=None) == -1                                    # nothing to do
    assert call(x_new=A) == -1 and call(dt=2) == -1 and call(M=0) == -1 and call(D=0) == -1


def test_goldens_hold_what_the_gpu_tests_need():
    inputs = gold("vggt_dinov2_inputs.pt")
    assert {k: tuple(v.shape) for k, v in inputs.items()} == {"70x70": (2, 3, 70, 70), "42x70": (2, 3, 42, 70), "98x56": (2, 3, 98, 56)}
    for tag, dim in (("a", 64), ("b", 128)):
        g = gold(f"vggt_dinov2_{tag}.pt")
        assert g["cfg"]["embed_dim"] == dim and set(g["cases"]) == set(inputs)
        for name, c in g["cases"].items():
            P = (inputs[name].shape[2] // 14) * (inputs[name].shape[3] // 14)
            assert c["prepare64"].shape == (2, 5 + P, dim) and c["prepare64"].dtype == torch.float64
            for k in KEYS:
                a64, a32 = c[k + "64"], c[k + "32"]
                assert a64.dtype == torch.float64 and a32.dtype == torch.float32 and a64.shape == a32.shape
                d32 = float((a32.double() - a64).abs().max() / a64.abs().max())
                assert 1e-9 < d32 < 1e-4, (tag, name, k, d32)                        # both evaluations present and distinct
                assert 0 < c["ref_bf16_distance"][k] <= 0.01, (tag, name, k, c["ref_bf16_distance"][k])
            assert c["x_norm_patchtokens64"].shape == (2, P, dim) and c["x_norm_regtokens64"].shape == (2, 4, dim) and c["x_prenorm64"].shape == (2, 5 + P, dim)
            # what the recipe randomises is visible: the register rows differ from each other and from the class row
            assert float((c["prepare64"][:, 1] - c["prepare64"][:, 2]).abs().max()) > 0.1
    # the restatement the GPU tests take d16 from IS the golden's function (float64, case a with its stored state)
    g, state = gold("vggt_dinov2_a.pt"), gold("vggt_dinov2_a_state.pt")
    for name, c in g["cases"].items():
        out = R.forward({k: v.double() for k, v in state.items()}, inputs[name].double(), 14, 1)
        for k in KEYS:
            assert float((out[k] - c[k + "64"]).abs().max() / c[k + "64"].abs().max()) < 1e-6, (name, k)
        pos = R.pos_table(state["pos_embed"], inputs[name].shape[2] // 14, inputs[name].shape[3] // 14)
        prep = R.prepare_tokens({k: v.double() for k, v in state.items()}, inputs[name].double(), 14, pos)
        assert float((prep - c["prepare64"]).abs().max()) < 1e-9
    agg = gold("vggt_dinov2_agg.pt")
    assert len(agg["outputs"]) == 2 and agg["outputs"][0].shape == (1, 2, 5 + 15, 128) and agg["patch_start_idx"] == 5
