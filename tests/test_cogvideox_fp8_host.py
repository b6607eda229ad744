"""Host side of CogVideoXTransformer3DModel.enable_fp8 (the opt-in e4m3 feed-forward): the switch, its default, the trainer's config key and the
refusals that need no GPU.  The kernels and the numbers are in tests/test_gpu_cogvideox_fp8.py."""
import pytest
import torch

from videogpa_amd import ops
from videogpa_amd.transformer import CogVideoXTransformer3DModel


def _tiny(num_layers=3):
    return CogVideoXTransformer3DModel(num_attention_heads=2, num_layers=num_layers, time_embed_dim=32, text_embed_dim=48,
                                       use_rotary_positional_embeddings=True).to(torch.bfloat16)


def test_enable_fp8_is_off_by_default_and_toggles_every_block():
    m = _tiny()
    assert len(m.transformer_blocks) == 3 and not any(b.fp8_ffn for b in m.transformer_blocks)
    assert m.enable_fp8() is m and all(b.fp8_ffn is True for b in m.transformer_blocks)
    m.enable_fp8(False)
    assert not any(b.fp8_ffn for b in m.transformer_blocks)
    m.enable_fp8(enabled=1)
    assert all(b.fp8_ffn is True for b in m.transformer_blocks)


def test_trainer_reads_fp8_ffn_from_its_config():
    from videogpa_amd.trainer import DEFAULT_CONFIG, CogVideoXDPOTrainer, variant_config
    assert DEFAULT_CONFIG["fp8_ffn"] is False
    assert all(variant_config(v)["fp8_ffn"] is False for v in ("t2v", "i2v", "1.5")) and variant_config("t2v", fp8_ffn=True)["fp8_ffn"] is True
    base = {"lora_rank": 4, "lora_alpha": 8}
    off = CogVideoXDPOTrainer(dict(base), transformer=_tiny(1))
    assert off.config["fp8_ffn"] is False and not any(b.fp8_ffn for b in off.transformer.get_base_model().transformer_blocks)
    on = CogVideoXDPOTrainer(dict(base, fp8_ffn=True), transformer=_tiny(2))
    blocks = on.transformer.get_base_model().transformer_blocks
    assert len(blocks) == 2 and all(b.fp8_ffn for b in blocks)
    # the adapters sit where the reference puts them: the feed-forward stays unwrapped, so the e4m3 path has frozen projections to run on
    assert all(not hasattr(b.ff.net[0].proj, "base_layer") and not hasattr(b.ff.net[2], "base_layer") for b in blocks)


def test_fp8_forward_has_no_cpu_fallback():
    m = _tiny(1).enable_fp8()
    x = torch.zeros(1, 1, 16, 4, 4, dtype=torch.bfloat16)
    txt = torch.zeros(1, 2, 48, dtype=torch.bfloat16)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, encoder_hidden_states=txt, timestep=torch.tensor([3]))
    D, inner = 128, 512
    z = torch.zeros(1, 4, D, dtype=torch.bfloat16)
    gates = torch.zeros(1, 2, D)
    w, b = torch.ones(D), torch.zeros(D)
    W1, b1 = torch.zeros(inner, D, dtype=torch.bfloat16), torch.zeros(inner, dtype=torch.bfloat16)
    W2, b2 = torch.zeros(D, inner, dtype=torch.bfloat16), torch.zeros(D, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ffn_tail_fp8(z, z, gates, w, b, None, W1, b1, W2, b2, gates, w, b)


def test_fp8_tail_refuses_trainable_and_lora_wrapped_feed_forward_weights():
    """checked before any kernel is reached, so it needs no GPU"""
    D, inner = 128, 512
    z = torch.zeros(1, 4, D, dtype=torch.bfloat16)
    gates = torch.zeros(1, 2, D)
    w, b = torch.ones(D), torch.zeros(D)
    W1, b1 = torch.zeros(inner, D, dtype=torch.bfloat16), torch.zeros(inner, dtype=torch.bfloat16)
    W2, b2 = torch.zeros(D, inner, dtype=torch.bfloat16), torch.zeros(D, dtype=torch.bfloat16)
    for trainable in ("W1", "b1", "W2", "b2"):
        args = {"W1": W1, "b1": b1, "W2": W2, "b2": b2}
        args[trainable] = args[trainable].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="frozen projections only"):
            ops.ffn_tail_fp8(z, z, gates, w, b, None, args["W1"], args["b1"], args["W2"], args["b2"], gates, w, b)
    from videogpa_amd.lora import LoraConfig, get_peft_model
    for target, name in (("ff.net.0.proj", r"ff\.net\.0\.proj"), ("ff.net.2", r"ff\.net\.2")):
        pm = get_peft_model(_tiny(1), LoraConfig(r=4, lora_alpha=8, target_modules=["to_q", target]))
        blk = pm.get_base_model().enable_fp8().transformer_blocks[0]
        with pytest.raises(RuntimeError, match=name + " is LoRA-wrapped"):
            blk._frozen_ff()
