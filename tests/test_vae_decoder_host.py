"""videogpa_amd.vae's decoder without a GPU: the opt-in (`with_decoder=True`) and what stays as it was without it, names and shapes against
tests/vae_decoder_oracle.py, the strict loader on `decoder.*`, the latent frame batches and the tile arithmetic of tiled_decode, the C-ABI exports of
the new entry points, and self-checks of the oracle's own pieces."""
import os
import re

import pytest
import torch

import vae_decoder_oracle as vd
import vae_oracle as vo
from test_vae_host import CONFIG, NARROW, _write_checkpoint
from videogpa_amd.vae import AutoencoderKLCogVideoX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("vgpa_vae_upsample_f32", "vgpa_spatial_norm_silu_f32", "vgpa_vae_output")


def _full_state_dict(**arch):
    return {**vo.seeded_state_dict(**arch), **vd.seeded_decoder_state_dict(**arch)}


def test_decoder_names_and_shapes_of_the_5b_config():
    with torch.device("meta"):
        vae = AutoencoderKLCogVideoX(with_decoder=True)
    sd = vae.state_dict()
    shape = lambda k: tuple(sd[k].shape)
    assert shape("decoder.conv_in.conv.weight") == (512, 16, 3, 3, 3)
    assert shape("decoder.mid_block.resnets.1.conv2.conv.weight") == (512, 512, 3, 3, 3)
    assert shape("decoder.up_blocks.1.resnets.0.conv_shortcut.weight") == (256, 512, 1, 1, 1)
    assert shape("decoder.up_blocks.1.resnets.0.norm1.norm_layer.weight") == (512,)
    assert "decoder.up_blocks.0.resnets.0.conv_shortcut.weight" not in sd and "decoder.up_blocks.2.resnets.0.conv_shortcut.weight" not in sd
    assert shape("decoder.up_blocks.3.resnets.0.conv_shortcut.weight") == (128, 256, 1, 1, 1)
    assert shape("decoder.up_blocks.3.resnets.3.norm2.conv_y.conv.weight") == (128, 16, 1, 1, 1)
    assert shape("decoder.up_blocks.3.resnets.3.norm2.conv_b.conv.bias") == (128,)
    assert shape("decoder.up_blocks.2.upsamplers.0.conv.weight") == (256, 256, 3, 3)
    assert not any(k.startswith("decoder.up_blocks.3.upsamplers") for k in sd)
    assert "decoder.up_blocks.3.resnets.4.conv1.conv.weight" not in sd                                  # layers_per_block + 1 = 4 resnets
    assert shape("decoder.norm_out.conv_b.conv.weight") == (128, 16, 1, 1, 1)
    assert shape("decoder.conv_out.conv.weight") == (3, 128, 3, 3, 3)
    want = vd.seeded_decoder_state_dict()
    assert {k for k in sd if k.startswith("decoder.")} == set(want)
    assert all(shape(k) == tuple(v.shape) for k, v in want.items())
    assert {k for k in sd if not k.startswith("decoder.")} == set(vo.seeded_state_dict())           # the encoder's names as before
    assert vae.decoder.norm_out.norm_layer.eps == 1e-6


def test_the_default_module_is_unchanged():
    vae = AutoencoderKLCogVideoX(**NARROW)
    assert vae.decoder is None and all(k.startswith("encoder.") for k in vae.state_dict())
    with pytest.raises(NotImplementedError, match="with_decoder=True"):
        vae.decode(torch.zeros(1, 16, 1, 2, 2))
    with pytest.raises(NotImplementedError, match="with_decoder=True"):
        vae(torch.zeros(1, 3, 1, 16, 16))
    both = AutoencoderKLCogVideoX(with_decoder=True, **NARROW)
    assert "with_decoder" not in both.config and "with_decoder" not in vae.config and not hasattr(both.config, "with_decoder")
    assert both.num_latent_frames_batch_size == 2 and both.num_sample_frames_batch_size == 8
    assert AutoencoderKLCogVideoX(use_post_quant_conv=True, **NARROW).config.use_post_quant_conv      # accepted where nothing decodes
    with pytest.raises(NotImplementedError, match="use_post_quant_conv"):
        AutoencoderKLCogVideoX(with_decoder=True, use_post_quant_conv=True, **NARROW)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        both.requires_grad_(False).decode(torch.zeros(1, 16, 1, 2, 2))
    with pytest.raises(RuntimeError, match=r"\[B,16,F,h,w\]"):
        both.decode(torch.zeros(1, 8, 1, 2, 2))


@pytest.mark.parametrize("shards", [1, 2])
def test_loader_round_trip_keeps_the_decoder(tmp_path, shards):
    sd = _full_state_dict(**NARROW)
    _write_checkpoint(str(tmp_path / "vae"), sd, CONFIG, shards)
    vae = AutoencoderKLCogVideoX.from_pretrained(str(tmp_path), subfolder="vae", torch_dtype=torch.bfloat16, with_decoder=True)
    assert vae.dtype == torch.bfloat16 and not vae.training and "with_decoder" not in vae.config
    own = vae.state_dict()
    assert set(own) == set(sd)
    for k, v in sd.items():
        assert torch.equal(own[k].float(), v), k
    enc_only = AutoencoderKLCogVideoX.from_pretrained(str(tmp_path), subfolder="vae")               # the same files without the keyword
    assert set(enc_only.state_dict()) == {k for k in sd if k.startswith("encoder.")}


def test_loader_names_a_missing_a_misshaped_and_an_unexpected_decoder_tensor(tmp_path):
    sd = _full_state_dict(**NARROW)
    load = lambda d: AutoencoderKLCogVideoX.from_pretrained(str(tmp_path / d), with_decoder=True)
    missing = dict(sd)
    del missing["decoder.up_blocks.2.resnets.1.norm2.conv_b.conv.bias"]
    _write_checkpoint(str(tmp_path / "a"), missing, CONFIG)
    with pytest.raises(RuntimeError, match=r"missing: decoder\.up_blocks\.2\.resnets\.1\.norm2\.conv_b\.conv\.bias"):
        load("a")
    wrong = dict(sd)
    wrong["decoder.norm_out.conv_y.conv.weight"] = torch.zeros(32, 16, 1, 1)                            # 4-D where upstream stores 1x1x1
    _write_checkpoint(str(tmp_path / "b"), wrong, CONFIG)
    with pytest.raises(RuntimeError, match=r"shape mismatch: decoder\.norm_out\.conv_y\.conv\.weight"):
        load("b")
    extra = dict(sd)
    extra["decoder.up_blocks.3.upsamplers.0.conv.weight"] = torch.zeros(32, 32, 3, 3)                  # the last block has no up-sampler
    _write_checkpoint(str(tmp_path / "c"), extra, CONFIG)
    with pytest.raises(RuntimeError, match=r"unexpected: decoder\.up_blocks\.3\.upsamplers\.0\.conv\.weight"):
        load("c")
    _write_checkpoint(str(tmp_path / "d"), vo.seeded_state_dict(**NARROW), CONFIG)                    # an encoder-only checkpoint
    with pytest.raises(RuntimeError, match=r"missing: decoder\.conv_in\.conv\.bias"):
        load("d")


def test_latent_frame_batches():
    vae = AutoencoderKLCogVideoX(with_decoder=True, **NARROW)
    want = {1: [(0, 1)], 2: [(0, 2)], 3: [(0, 3)], 4: [(0, 2), (2, 4)], 5: [(0, 3), (3, 5)],
            13: [(0, 3), (3, 5), (5, 7), (7, 9), (9, 11), (11, 13)]}
    for frames, ranges in want.items():
        assert vae.latent_frame_batches(frames) == ranges, frames
        assert [(s, min(e, frames)) for s, e in vd.latent_frame_batches(frames)] == ranges, frames
    # frames out: a batch of t latent frames gives t (one frame), 4t (even) or 4t - 3 (odd: frame 0 is never doubled)
    out = lambda t: t if t == 1 else 4 * t - 3 if t % 2 else 4 * t
    assert sum(out(e - s) for s, e in want[13]) == 49 and sum(out(e - s) for s, e in want[5]) == 17 and out(2) == 8


def test_decode_tile_plan_at_60x90():
    vae = AutoencoderKLCogVideoX(with_decoder=True)
    plan = vae.decode_tile_plan(60, 90)
    assert plan["rows"] == [(0, 30), (25, 30), (50, 10)]
    assert plan["cols"] == [(0, 45), (36, 45), (72, 18)]
    assert plan["blend"] == (40, 72) and plan["keep"] == (200, 288)
    assert sum(min(8 * h, 200) for _, h in plan["rows"]) == 480 and sum(min(8 * w, 288) for _, w in plan["cols"]) == 720
    small = AutoencoderKLCogVideoX(with_decoder=True, sample_height=64, sample_width=96, **NARROW)      # the GPU test's size
    plan = small.decode_tile_plan(10, 14)
    assert plan["rows"] == [(0, 4), (3, 4), (6, 4), (9, 1)] and plan["cols"] == [(0, 6), (4, 6), (8, 6), (12, 2)]
    assert plan["blend"] == (5, 9) and plan["keep"] == (27, 39)


def test_new_entry_points_are_declared_and_bound():
    from videogpa_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "videogpa_hip.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
    for name in ("vae_upsample_f32", "spatial_norm_silu_f32", "vae_output"):
        assert callable(getattr(ops, name)), name
    assert [ops.vae_upsample_frames(t, True) for t in (1, 2, 3, 4, 5)] == [1, 4, 5, 8, 9]
    assert [ops.vae_upsample_frames(t, False) for t in (1, 2, 3)] == [1, 2, 3]


def test_generate_has_decode_latents_and_no_longer_calls_the_vae_third_party():
    from videogpa_amd import generate
    assert callable(generate.decode_latents)
    assert "outside the hot path: the caller passes prompt embeddings in and gets latents out" not in generate.__doc__


# ------------------------------------------------------------------------------------------------------------------ the oracle's own pieces
def test_oracle_upsampler_frame_counts_and_sources():
    from videogpa_amd import ops
    for t, want in ((1, 1), (2, 4), (3, 5), (5, 9)):
        assert ops.vae_upsample_frames(t, True) == want                      # what the device op allocates
        x = torch.arange(t, dtype=torch.float32).reshape(1, 1, t, 1, 1).expand(1, 1, t, 2, 3)
        up = vd.upsample_frames(x, compress_time=True)
        assert tuple(up.shape) == (1, 1, want, 4, 6), t
        src = [0] + [1 + (k - 1) // 2 for k in range(1, want)] if t % 2 and t > 1 else [k // 2 for k in range(want)] if t > 1 else [0]
        assert up[0, 0, :, 0, 0].tolist() == [float(s) for s in src], t
        assert tuple(vd.upsample_frames(x, compress_time=False).shape) == (1, 1, t, 4, 6)


def test_oracle_narrow_decoder_turns_13_latent_frames_into_49():
    sd = vd.seeded_decoder_state_dict(**NARROW, seed=3)
    z = torch.randn(1, 16, 13, 3, 4, generator=torch.Generator().manual_seed(1))
    frames = vd.batched_decoder(sd, z)
    assert tuple(frames.shape) == (1, 3, 49, 24, 32) and torch.isfinite(frames).all()
    vae = AutoencoderKLCogVideoX(with_decoder=True, **NARROW)
    assert {k for k in vae.state_dict() if k.startswith("decoder.")} == set(sd)                      # the module under test reads the same names
    assert len(vae.latent_frame_batches(13)) == 6 and 9 + 5 * 8 == frames.shape[2]
    assert float(frames.abs().max()) < 50 and float(frames.std()) > 0.05                              # O(1) activations


def test_oracle_spatial_norm_sees_the_odd_frame_split_at_five_frames():
    g = torch.Generator().manual_seed(2)
    sd = {k[len("decoder.norm_out."):]: v for k, v in vd.seeded_decoder_state_dict(**NARROW, seed=4).items() if k.startswith("decoder.norm_out.")}
    from videogpa_amd.vae import _SpatialNorm3D
    assert set(_SpatialNorm3D(32, 16, 32).state_dict()) == set(sd)
    sd = {"n." + k: v for k, v in sd.items()}
    f, zq = torch.randn(1, 32, 5, 6, 10, generator=g), torch.randn(1, 16, 3, 3, 5, generator=g)
    split, plain = vd.spatial_norm(sd, "n", f, zq, 32), vd.spatial_norm(sd, "n", f, zq, 32, split=False)
    # split: latent frames (0, 1, 1, 2, 2); plain: floor(k * 3 / 5) = (0, 0, 1, 1, 2) -- frames 1 and 3 differ
    same = [bool(torch.equal(split[:, :, k], plain[:, :, k])) for k in range(5)]
    assert same == [True, False, True, False, True]
    z4 = vd.resize_zq(zq, (4, 6, 10))
    assert torch.equal(z4[:, :, 1], z4[:, :, 0]) and torch.equal(z4[0, 0, 0, 1, 1], zq[0, 0, 0, 0, 0]) and torch.equal(z4[0, 0, 3, 5, 9], zq[0, 0, 2, 2, 4])
