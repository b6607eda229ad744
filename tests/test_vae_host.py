"""videogpa_amd.vae without a GPU: the tile arithmetic of tiled_encode, the strict loader over a diffusers-layout directory, the C-ABI exports of the
new entry points, and the refusals (more than one frame, the decoder, unsupported configs)."""
import json
import os
import re

import pytest
import torch

import vae_oracle as vo
from videogpa_amd.vae import AutoencoderKLCogVideoX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARROW = dict(block_out_channels=(32, 64, 64, 64), layers_per_block=2)
NEW_ENTRY_POINTS = ("vgpa_conv3x3_pad_f32", "vgpa_vae_input_f32", "vgpa_groupnorm_stats_workspace_bytes", "vgpa_groupnorm_stats_f32",
                    "vgpa_groupnorm_silu_f32", "vgpa_vae_sample")


def test_tile_arithmetic_at_480x720():
    vae = AutoencoderKLCogVideoX()
    assert (vae.tile_sample_min_height, vae.tile_sample_min_width) == (240, 360)
    assert (vae.tile_latent_min_height, vae.tile_latent_min_width) == (30, 45)
    plan = vae.tile_plan(480, 720)
    assert plan["rows"] == [(0, 240), (200, 240), (400, 80)]
    assert plan["cols"] == [(0, 360), (288, 360), (576, 144)]
    assert plan["blend"] == (5, 9) and plan["keep"] == (25, 36)
    # latent sizes of the tiles (three one-sided stride-2 convolutions), cropped to `keep`, concatenated: the 60 x 90 latent
    lat = lambda n: ((((n - 2) // 2 + 1) - 2) // 2 + 1 - 2) // 2 + 1
    assert [lat(h) for _, h in plan["rows"]] == [30, 30, 10] and [lat(w) for _, w in plan["cols"]] == [45, 45, 18]
    assert sum(min(lat(h), 25) for _, h in plan["rows"]) == 60 and sum(min(lat(w), 36) for _, w in plan["cols"]) == 90


def test_tile_arithmetic_at_the_small_test_size():
    """sample 64 x 96 (tests/test_gpu_vae.py): the same 3 x 3 grid with short last tiles"""
    vae = AutoencoderKLCogVideoX(sample_height=64, sample_width=96, **NARROW)
    plan = vae.tile_plan(64, 96)
    assert plan["rows"] == [(0, 32), (26, 32), (52, 12)]
    assert plan["cols"] == [(0, 48), (38, 48), (76, 20)]
    assert (vae.tile_latent_min_height, vae.tile_latent_min_width) == (4, 6)
    assert plan["blend"] == (0, 1) and plan["keep"] == (4, 5)
    # enable_tiling's overrides (the second tiling case of the GPU test: real ramps in both directions)
    vae.enable_tiling(tile_sample_min_height=48, tile_sample_min_width=48, tile_overlap_factor_height=0.5, tile_overlap_factor_width=0.5)
    plan = vae.tile_plan(64, 96)
    assert plan["rows"] == [(0, 48), (24, 40), (48, 16)] and plan["cols"] == [(0, 48), (24, 48), (48, 48), (72, 24)]
    assert plan["blend"] == (3, 3) and plan["keep"] == (3, 3)


def _write_checkpoint(root, sd, config, shards=1):
    from safetensors.torch import save_file
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "config.json"), "w") as f:
        json.dump(config, f)
    sd = {k: v.to(torch.bfloat16).contiguous() for k, v in sd.items()}
    if shards == 1:
        save_file(sd, os.path.join(root, "diffusion_pytorch_model.safetensors"))
        return
    keys = sorted(sd)
    cut = len(keys) // 2
    weight_map = {}
    for n, part in enumerate((keys[:cut], keys[cut:])):
        fn = f"diffusion_pytorch_model-{n + 1:05d}-of-00002.safetensors"
        save_file({k: sd[k] for k in part}, os.path.join(root, fn))
        weight_map.update({k: fn for k in part})
    with open(os.path.join(root, "diffusion_pytorch_model.safetensors.index.json"), "w") as f:
        json.dump({"metadata": {}, "weight_map": weight_map}, f)


CONFIG = dict(_class_name="AutoencoderKLCogVideoX", _diffusers_version="0.31.0", block_out_channels=[32, 64, 64, 64], layers_per_block=2,
              latent_channels=16, scaling_factor=0.7, sample_height=64, sample_width=96, some_future_key=[1, 2])


@pytest.mark.parametrize("shards", [1, 2])
def test_loader_round_trip(tmp_path, shards):
    sd = vo.seeded_state_dict(**NARROW, with_decoder_keys=True)
    _write_checkpoint(str(tmp_path / "vae"), sd, CONFIG, shards)
    vae = AutoencoderKLCogVideoX.from_pretrained(str(tmp_path), subfolder="vae", torch_dtype=torch.bfloat16)
    assert vae.dtype == torch.bfloat16 and not vae.training
    assert vae.config.some_future_key == [1, 2] and vae.config._class_name == "AutoencoderKLCogVideoX"       # unknown keys are kept
    assert vae.config.block_out_channels == (32, 64, 64, 64) and vae.config.scaling_factor == 0.7 and vae.config.norm_eps == 1e-6
    own = vae.state_dict()
    enc = {k: v for k, v in sd.items() if k.startswith("encoder.")}
    assert set(own) == set(enc)                                                                               # decoder.* skipped, nothing else
    for k, v in enc.items():
        assert torch.equal(own[k].float(), v), k
    assert AutoencoderKLCogVideoX.from_pretrained(str(tmp_path / "vae")).dtype == torch.float32
    assert vae.requires_grad_(False) is vae and not any(p.requires_grad for p in vae.parameters())


def test_loader_names_a_missing_key_and_a_wrong_shape(tmp_path):
    sd = vo.seeded_state_dict(**NARROW)
    missing = dict(sd)
    del missing["encoder.mid_block.resnets.1.norm2.bias"]
    _write_checkpoint(str(tmp_path / "a"), missing, CONFIG)
    with pytest.raises(RuntimeError, match=r"missing: encoder\.mid_block\.resnets\.1\.norm2\.bias"):
        AutoencoderKLCogVideoX.from_pretrained(str(tmp_path / "a"))
    wrong = dict(sd)
    wrong["encoder.down_blocks.1.resnets.0.conv_shortcut.weight"] = torch.zeros(64, 32, 1, 1)              # 4-D where upstream stores 1x1x1
    _write_checkpoint(str(tmp_path / "b"), wrong, CONFIG)
    with pytest.raises(RuntimeError, match=r"shape mismatch: encoder\.down_blocks\.1\.resnets\.0\.conv_shortcut\.weight"):
        AutoencoderKLCogVideoX.from_pretrained(str(tmp_path / "b"))
    extra = dict(sd)
    extra["encoder.down_blocks.0.attentions.0.weight"] = torch.zeros(4)
    _write_checkpoint(str(tmp_path / "c"), extra, CONFIG)
    with pytest.raises(RuntimeError, match=r"unexpected: encoder\.down_blocks\.0\.attentions\.0\.weight"):
        AutoencoderKLCogVideoX.from_pretrained(str(tmp_path / "c"))
    with pytest.raises(FileNotFoundError):
        AutoencoderKLCogVideoX.from_pretrained(str(tmp_path / "nowhere"))


def test_state_dict_names_and_shapes_of_the_5b_config():
    with torch.device("meta"):
        vae = AutoencoderKLCogVideoX()
    sd = vae.state_dict()
    assert tuple(sd["encoder.conv_in.conv.weight"].shape) == (128, 3, 3, 3, 3)
    assert tuple(sd["encoder.down_blocks.1.resnets.0.conv_shortcut.weight"].shape) == (256, 128, 1, 1, 1)
    assert "encoder.down_blocks.2.resnets.0.conv_shortcut.weight" not in sd                                  # 256 -> 256
    assert tuple(sd["encoder.down_blocks.2.downsamplers.0.conv.weight"].shape) == (256, 256, 3, 3)
    assert "encoder.down_blocks.3.downsamplers.0.conv.weight" not in sd
    assert tuple(sd["encoder.mid_block.resnets.1.conv2.conv.weight"].shape) == (512, 512, 3, 3, 3)
    assert tuple(sd["encoder.conv_out.conv.weight"].shape) == (32, 512, 3, 3, 3) and tuple(sd["encoder.norm_out.weight"].shape) == (512,)
    assert sorted(sd) == sorted(vo.seeded_state_dict().keys())                                                # the oracle reads the same names


def test_new_entry_points_are_declared_and_bound():
    from videogpa_amd import _lib
    header = open(os.path.join(ROOT, "include", "videogpa_hip.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
    assert _lib.query("vgpa_groupnorm_stats_workspace_bytes", 0, 10, 32, 32) == 0
    # 120 x 181 pixels of 128 channels: 32 float4 columns -> 8 pixel rows x 64 pixels per workgroup = 512 pixels, 43 chunks of (mean, M2) fp64 per channel
    assert _lib.query("vgpa_groupnorm_stats_workspace_bytes", 2, 120 * 181, 128, 32) == 2 * 43 * 128 * 2 * 8


def test_refusals():
    vae = AutoencoderKLCogVideoX(**NARROW)
    with pytest.raises(NotImplementedError, match="2 frames"):
        vae.encode(torch.zeros(1, 3, 2, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vae.requires_grad_(False).encode(torch.zeros(1, 3, 1, 16, 16))
    with pytest.raises(NotImplementedError):
        vae.decode(torch.zeros(1, 16, 1, 2, 2))
    for bad in (dict(use_quant_conv=True), dict(act_fn="relu"), dict(block_out_channels=(48, 64, 64, 64))):
        with pytest.raises(NotImplementedError):
            AutoencoderKLCogVideoX(**bad)
    # the switches are plain flags
    vae.enable_slicing(); vae.enable_tiling()
    assert vae.use_slicing and vae.use_tiling
    vae.disable_slicing(); vae.disable_tiling()
    assert not vae.use_slicing and not vae.use_tiling


def test_trainer_takes_a_vae_and_honours_its_switches():
    import inspect
    from videogpa_amd.trainer import DEFAULT_CONFIG, CogVideoXDPOTrainer
    assert "vae" in inspect.signature(CogVideoXDPOTrainer.__init__).parameters
    assert DEFAULT_CONFIG["enable_slicing"] is True and DEFAULT_CONFIG["enable_tiling"] is True
