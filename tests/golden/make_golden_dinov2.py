"""Writes tests/golden/vggt_dinov2*.pt and vggt_dinov2_vitl14_reg_names.json: the reference's DinoVisionTransformer (vggt/layers/vision_transformer.py)
and its Aggregator with a DINOv2 front, imported from the reference and evaluated on the CPU.

    python tests/golden/make_golden_dinov2.py /path/to/reference

Tensors, numbers and names only, every file below 1 MiB:
  vggt_dinov2_inputs.pt   2 normalised frames at 70 x 70 (the position table's own grid: the shortcut), 42 x 70 and 98 x 56 (interpolated, both orientations)
  vggt_dinov2_a_state.pt  case (a): dim 64, 1 head, depth 2, img_size 70 (5 x 5 table), 4 registers -- the state dict itself
  vggt_dinov2_a.pt        case (a) per input: x_norm_patchtokens / clstoken / regtokens and x_prenorm in float64 and fp32, the fp32 position table, the
                          float64 output of prepare_tokens_with_masks, the reference's own CPU bf16-autocast distance from float64
  vggt_dinov2_b.pt        case (b): dim 128, 2 heads, depth 4 -- the same, with per-tensor float64 sums of the state instead of the state (3.3 MiB): the
                          tests regenerate it from tests/dinov2_ref.py::seeded_state and check the sums
  vggt_dinov2_agg.pt      the reference Aggregator (depth 2, dim 64) whose patch_embed is a reduced DinoVisionTransformer: per-depth outputs, state sums
The parameters come from dinov2_ref.seeded_state (what timm's initialisation leaves trivial is randomised there)."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dinov2_ref  # noqa: E402

PATCH, REG = 14, 4
SHAPES = ((70, 70), (42, 70), (98, 56))
CASES = {"a": dict(embed_dim=64, num_heads=1, depth=2, seed=1), "b": dict(embed_dim=128, num_heads=2, depth=4, seed=2)}
KEYS = ("x_norm_patchtokens", "x_norm_clstoken", "x_norm_regtokens", "x_prenorm")


def save(name, obj):
    path = os.path.join(HERE, name)
    torch.save(obj, path)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20), "fixtures stay below 1 MiB each"


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def main(ref_root):
    sys.path.insert(0, ref_root)
    from vggt.layers.vision_transformer import DinoVisionTransformer
    from vggt.models.aggregator import Aggregator
    g = torch.Generator().manual_seed(2024)
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    inputs = {f"{h}x{w}": ((torch.rand(2, 3, h, w, generator=g) - mean) / std) for h, w in SHAPES}
    save("vggt_dinov2_inputs.pt", inputs)

    def build(cfg):
        return DinoVisionTransformer(img_size=70, patch_size=PATCH, embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"], mlp_ratio=4,
                                     num_register_tokens=REG, interpolate_antialias=True, interpolate_offset=0.0, block_chunks=0, init_values=1.0).eval()

    for tag, cfg in CASES.items():
        m = build(cfg)
        state = dinov2_ref.seeded_state({k: v.shape for k, v in m.state_dict().items()}, cfg["seed"])
        m.load_state_dict(state, strict=True)
        m64 = build(cfg).double()
        m64.load_state_dict({k: v.double() for k, v in state.items()}, strict=True)
        out = {"cfg": dict(cfg, img_size=70, patch_size=PATCH, num_register_tokens=REG), "sums": dinov2_ref.state_sums(state),
               "shapes": {k: list(v.shape) for k, v in state.items()}, "cases": {}}
        for name, x in inputs.items():
            with torch.no_grad():
                o32, o64 = m(x), m64(x.double())
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    o16 = m(x)
                c = {"pos": m.interpolate_pos_encoding(torch.empty(1, 1 + (x.shape[2] // PATCH) * (x.shape[3] // PATCH), cfg["embed_dim"]), x.shape[2], x.shape[3]).clone(),
                     "prepare64": m64.prepare_tokens_with_masks(x.double()).clone(),
                     "ref_bf16_distance": {k: rel(o16[k], o64[k]) for k in KEYS}}
                # the restatement the tests use for d16 is the same function: fp32 against the reference's fp32, float64 against its float64
                r32 = dinov2_ref.forward(state, x, PATCH, cfg["num_heads"])
                r64 = dinov2_ref.forward({k: v.double() for k, v in state.items()}, x.double(), PATCH, cfg["num_heads"])
            for k in KEYS:
                c[k + "64"], c[k + "32"] = o64[k].clone(), o32[k].clone()
                assert rel(r32[k], o32[k]) < 1e-5 and rel(r64[k], o64[k]) < 1e-6, (k, rel(r32[k], o32[k]), rel(r64[k], o64[k]))
            print(tag, name, "reference bf16 distance", {k: round(v, 5) for k, v in c["ref_bf16_distance"].items()}, "fp32 distance",
                  rel(o32["x_prenorm"], o64["x_prenorm"]), "range", float(o64["x_prenorm"].abs().max()))
            out["cases"][name] = c
        if tag == "a":
            save("vggt_dinov2_a_state.pt", state)
        save(f"vggt_dinov2_{tag}.pt", out)

    # the aggregator with a reduced DINOv2 in front (the reference builds only the four full-size ones by name: the module is swapped in)
    cfg = dict(embed_dim=64, num_heads=1, depth=2, mlp_ratio=2.0, dino_depth=2, seed=3, B=1, S=2, H=42, W=70)
    agg = Aggregator(img_size=70, patch_size=PATCH, embed_dim=64, depth=2, num_heads=1, mlp_ratio=2.0, num_register_tokens=REG, patch_embed="conv",
                     qk_norm=True, rope_freq=100, init_values=0.01).eval()
    agg.patch_embed = build(dict(embed_dim=64, num_heads=1, depth=cfg["dino_depth"])).eval()
    state = dinov2_ref.seeded_state({k: v.shape for k, v in agg.state_dict().items()}, cfg["seed"], bf16_representable=True)
    agg.load_state_dict(state, strict=True)
    images = torch.rand(cfg["B"], cfg["S"], 3, cfg["H"], cfg["W"], generator=g).to(torch.bfloat16).float()
    with torch.no_grad():
        outs, start = agg(images)
    save("vggt_dinov2_agg.pt", {"cfg": cfg, "images": images.to(torch.bfloat16), "sums": dinov2_ref.state_sums(state), "outputs": [o.clone() for o in outs],
                                "patch_start_idx": start})

    # names and shapes of the full-size front, as a VGGT checkpoint carries them
    from vggt.layers.vision_transformer import vit_large      # with the arguments of Aggregator.__build_patch_embed__ (aggregator.py:147-178)
    full = vit_large(img_size=518, patch_size=14, num_register_tokens=4, interpolate_antialias=True, interpolate_offset=0.0, block_chunks=0, init_values=1.0)
    names = {"patch_embed." + k: list(v.shape) for k, v in full.state_dict().items()}
    path = os.path.join(HERE, "vggt_dinov2_vitl14_reg_names.json")
    with open(path, "w") as f:
        json.dump({"aggregator." + k: s for k, s in names.items()}, f, indent=0, sort_keys=True)
    print(path, len(names), os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
