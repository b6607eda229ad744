"""videogpa_amd.t5 without a GPU: the oracle tests/t5_ref.py against upstream's golden outputs, the delta -> bucket table, state-dict names, the
loader, every refusal, and the bounds of tests/t5_tol.py against float32 restatements of the kernels (right ones inside, wrong ones outside).

Measured here: t5_ref in fp64 is 2.9e-15 (no mask) and 3.1e-15 (mask) away from the golden outputs of tests/golden/t5_tiny.pt (max |out| 3.8 and 4.1);
the test asserts 100 x the larger figure, 3.2e-13, which is far below the 1e-9 max |out| ceiling."""
import json
import os

import numpy as np
import pytest
import torch

import t5_ref
import t5_tol
from videogpa_amd import t5

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_VS_GOLDEN = 3.2e-13          # 100 x the measured disagreement (module docstring)


@pytest.fixture(scope="module")
def tiny():
    return torch.load(os.path.join(GOLDEN, "t5_tiny.pt"))


@pytest.mark.parametrize("masked", [False, True])
def test_ref_fp64_reproduces_the_golden_outputs(tiny, masked):
    want = tiny["out_masked" if masked else "out"]
    got = t5_ref.forward(tiny["state_dict"], tiny["config"], tiny["input_ids"], tiny["attention_mask"] if masked else None, "fp64")
    err = float((got - want).abs().max())
    print(f"t5_ref fp64 vs golden ({'mask' if masked else 'no mask'}): max |diff| {err:.3e}, max |out| {float(want.abs().max()):.3f}")
    assert err <= REF_VS_GOLDEN and REF_VS_GOLDEN <= 1e-9 * float(want.abs().max())
    assert float((tiny["out"] - tiny["out_masked"]).abs().max()) > 1e-2          # the mask matters


def test_delta_bucket_table_is_upstreams(tiny):
    want = tiny["buckets"].long()
    assert torch.equal(t5.relative_position_bucket(tiny["deltas"]), want)
    assert torch.equal(t5.delta_buckets(512), want)
    for S in (1, 2, 40, 226):
        assert torch.equal(t5.delta_buckets(S), want[511 - (S - 1): 511 + S])
    assert t5.delta_buckets(226) is t5.delta_buckets(226)                          # built once per S
    try:
        from transformers.models.t5.modeling_t5 import T5Attention
    except Exception:
        return
    for S in (1, 226, 512):
        d = torch.arange(-(S - 1), S)
        assert torch.equal(t5.delta_buckets(S), T5Attention._relative_position_bucket(d, bidirectional=True, num_buckets=32, max_distance=128))
        i = torch.arange(S)
        full = T5Attention._relative_position_bucket(i[None, :] - i[:, None], bidirectional=True, num_buckets=32, max_distance=128)
        assert torch.equal(t5.delta_buckets(S)[(i[None, :] - i[:, None]) + S - 1], full)


def test_state_dict_names(tiny):
    with open(os.path.join(GOLDEN, "t5_names.json")) as f:
        want = json.load(f)
    m = t5.T5EncoderModel(tiny["config"])
    assert sorted(m.state_dict().keys()) == want == sorted(t5_ref.state_dict_names(tiny["config"]))
    assert m.encoder.embed_tokens.weight is m.shared.weight
    m.load_state_dict(tiny["state_dict"], strict=True)
    real = t5.T5Config()
    assert (real.num_layers, real.d_model, real.num_heads, real.d_kv, real.d_ff) == (24, 4096, 64, 64, 10240)


def _write_checkpoint(root, cfg, sd, shards):
    from safetensors.torch import save_file
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "config.json"), "w") as f:
        json.dump({**cfg, "architectures": ["T5EncoderModel"], "model_type": "t5", "dropout_rate": 0.1, "is_encoder_decoder": True}, f)
    sd = {k: v.contiguous().clone() for k, v in sd.items()}
    if shards == 1:
        save_file(sd, os.path.join(root, "model.safetensors"))
        return
    names = sorted(sd)
    cut = len(names) // 2
    wm = {}
    for i, part in enumerate((names[:cut], names[cut:])):
        fn = f"model-{i + 1:05d}-of-00002.safetensors"
        save_file({k: sd[k] for k in part}, os.path.join(root, fn))
        wm.update({k: fn for k in part})
    with open(os.path.join(root, "model.safetensors.index.json"), "w") as f:
        json.dump({"metadata": {}, "weight_map": wm}, f)


@pytest.mark.parametrize("shards", [1, 2])
def test_from_pretrained_round_trip(tiny, tmp_path, shards):
    cfg, sd = tiny["config"], dict(tiny["state_dict"])
    del sd["encoder.embed_tokens.weight"]                                          # filled from shared.weight
    sd["decoder.block.0.layer.0.SelfAttention.q.weight"] = torch.zeros(4, 4)       # a full T5 checkpoint: dropped
    sd["lm_head.weight"] = torch.zeros(4, 4)
    _write_checkpoint(str(tmp_path / "text_encoder"), cfg, sd, shards)
    m = t5.T5EncoderModel.from_pretrained(str(tmp_path), subfolder="text_encoder", torch_dtype=torch.bfloat16)
    got = m.state_dict()
    assert sorted(got) == sorted(tiny["state_dict"])
    for k, v in tiny["state_dict"].items():
        assert got[k].dtype == torch.bfloat16 and torch.equal(got[k], v), k
    assert m.encoder.embed_tokens.weight is m.shared.weight and not m.training
    assert t5.T5EncoderModel.from_pretrained(str(tmp_path / "text_encoder")).dtype == torch.float32
    with pytest.raises(FileNotFoundError):
        t5.T5EncoderModel.from_pretrained(str(tmp_path / "nowhere"))
    bad = dict(tiny["state_dict"])
    del bad["encoder.final_layer_norm.weight"]
    _write_checkpoint(str(tmp_path / "bad"), cfg, bad, 1)
    with pytest.raises(RuntimeError, match="final_layer_norm"):
        t5.T5EncoderModel.from_pretrained(str(tmp_path / "bad"))


def test_refusals(tiny):
    cfg = tiny["config"]
    with pytest.raises(NotImplementedError, match="is_decoder"):
        t5.T5EncoderModel({**cfg, "is_decoder": True})
    for ff in ("relu", "gated-relu", "gelu"):
        with pytest.raises(NotImplementedError, match="feed_forward_proj"):
            t5.T5EncoderModel({**cfg, "feed_forward_proj": ff})
    with pytest.raises(NotImplementedError, match="d_kv"):
        t5.T5EncoderModel({**cfg, "d_kv": 32})
    m = t5.T5EncoderModel(cfg).to(torch.bfloat16)
    ids = tiny["input_ids"]
    with pytest.raises(RuntimeError, match="512"):
        m(torch.zeros(1, 513, dtype=torch.long))
    with pytest.raises(ValueError, match="attention_mask"):
        m(ids, attention_mask=torch.ones(2, 39))
    with pytest.raises(NotImplementedError, match="fp16"):
        t5.T5EncoderModel(cfg).to(torch.float16)(ids)
    with pytest.raises(NotImplementedError, match="fp16"):
        m(ids, output_dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="inputs_embeds"):
        m(ids, inputs_embeds=torch.zeros(2, 40, 64))


def test_forward_without_a_gpu_raises(tiny):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from videogpa_amd import ops
    m = t5.T5EncoderModel(tiny["config"]).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(tiny["input_ids"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(tiny["input_ids"], attention_mask=tiny["attention_mask"])
    qkv = torch.zeros(1, 4, 3, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.t5_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], torch.zeros(2, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.t5_rms(torch.zeros(2, 64), torch.ones(64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.t5_embed_rms(torch.zeros(2, dtype=torch.long), torch.zeros(8, 64, dtype=torch.bfloat16), torch.ones(64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.t5_gated_gelu(torch.zeros(2, 32, dtype=torch.bfloat16))


def test_encode_prompt_is_exported():
    from videogpa_amd import generate
    assert callable(generate.encode_prompt)


# ---- the bounds of tests/t5_tol.py: the float32 restatement stays inside, a wrong variant does not
@pytest.mark.parametrize("D", [64, 192, 4096])
@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("out_bf16", [False, True])
def test_rms_bound_holds_the_restatement_and_not_a_wrong_variant(D, add, out_bf16):
    import row_tol as rt
    x, y, w, _, _ = t5_tol.rms_inputs(8, D)
    y = y if add else None
    x_new64 = x.double() + (y.double() if add else 0.0)
    ref = t5_ref.rms64(x_new64, w, 1e-6)
    tol = t5_tol.rms_tol(ref, D, add, out_bf16)
    xs, n = t5_tol.rms_f32(x, w, 1e-6, y, out_bf16)
    ratio, err, at = rt.worst(n, ref, tol)
    print(f"rms D {D} add {add} bf16 {out_bf16}: restatement err / bound {ratio:.3f} (|err| {err:.3e})")
    assert not rt.judge("rms_f32", n, ref, tol)
    assert not rt.judge("x_new", xs, x_new64, t5_tol.stream_tol(x_new64))
    for wrong in ("mean_sub", "eps_outside"):
        _, nw = t5_tol.rms_f32(x, w, 1e-6, y, out_bf16, wrong=wrong)
        assert rt.judge(wrong, nw, ref, tol), wrong


@pytest.mark.parametrize("F", [96, 10240])
def test_gated_gelu_bound_holds_the_restatement_and_not_a_wrong_variant(F):
    import row_tol as rt
    u = t5_tol.gelu_inputs(3, F)
    assert float(u.float().min()) == -12.0 and float(u.float().max()) == 12.0
    ref = t5_ref.gated_gelu64(u)
    tol = t5_tol.gated_gelu_tol(u, ref)
    got = t5_tol.gated_gelu_f32(u)
    ratio, err, _ = rt.worst(got, ref, tol)
    print(f"gated gelu F {F}: restatement err / bound {ratio:.3f} (|err| {err:.3e})")
    assert not rt.judge("gated_gelu_f32", got, ref, tol)
    for wrong in ("erf", "swapped"):
        assert rt.judge(wrong, t5_tol.gated_gelu_f32(u, wrong=wrong), ref, tol), wrong


def test_attention_reference_sums_agree_with_the_network_oracle(tiny):
    """attn_sums64 (the reference of the kernel test) is the attention of t5_ref.forward: same bias indexing, same mask"""
    g = torch.Generator().manual_seed(3)
    S, H = 37, 2
    q, k, v = (torch.randn(S, 64, generator=g, dtype=torch.float64) for _ in range(3))
    table = torch.randn(32, H, generator=g)
    keep = torch.ones(S, dtype=torch.bool)
    keep[11:] = False
    pb = t5_ref.position_bias(table.double(), S, 32, 128)[0, 1]
    s = q @ k.t() + pb + (1.0 - keep.double())[None, :] * torch.finfo(torch.float64).min
    want = torch.softmax(s, -1) @ v
    R = t5_ref.attn_sums64(q, k, v, t5_ref.bias_delta_from_table(table, S)[1], keep)
    assert float((R["o"] - want).abs().max()) < 1e-12
    assert np.isfinite(R["snorm"].numpy()).all()
