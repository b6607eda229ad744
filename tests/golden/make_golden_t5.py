"""Writes tests/golden/t5_names.json and tests/golden/t5_tiny.pt from transformers' T5EncoderModel (run once, by hand, where transformers is installed;
written with 5.15):  python tests/golden/make_golden_t5.py

t5_names.json   the state-dict names of a 2-layer T5EncoderModel, sorted
t5_tiny.pt      config (d_model 64, 2 heads x 64, d_ff 96, 2 layers, vocabulary 64, gated-gelu), the state dict (bf16; norm weights perturbed by +-30 %
                and the relative-position table N(0, 2): upstream's initialisation leaves them at 1 and near 0), input ids [2,40], an attention
                mask, upstream's fp64 outputs without and with the mask (the module cast to double, loaded with the bf16 values), and upstream's
                bucket of every relative position -511 .. 511.

One line of upstream is lifted for the fp64 run: T5LayerNorm.forward computes its variance from `hidden_states.to(torch.float32)` whatever the module's
type (a floor for half types), which leaves 1e-7 of fp32 noise in every norm of a double module.  Here the variance of a float64 input is taken in
float64; the rest of the forward is upstream's, line for line."""
import json
import math
import os

import torch
from transformers import T5Config, T5EncoderModel
from transformers.models.t5.modeling_t5 import T5Attention, T5LayerNorm

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = dict(vocab_size=64, d_model=64, d_kv=64, d_ff=96, num_layers=2, num_heads=2, relative_attention_num_buckets=32,
           relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")


def _layer_norm_fp64(self, hidden_states):
    """T5LayerNorm.forward with the variance in the input's own type when that is float64"""
    assert hidden_states.dtype == torch.float64
    variance = hidden_states.pow(2).mean(-1, keepdim=True)
    hidden_states = hidden_states * torch.rsqrt(variance + self.variance_epsilon)
    return self.weight * hidden_states


def main():
    torch.manual_seed(0)
    model = T5EncoderModel(T5Config(**CFG, dropout_rate=0.0, use_cache=False)).eval()
    names = sorted(model.state_dict().keys())
    g = torch.Generator().manual_seed(1)
    sd = {}
    for k, v in model.state_dict().items():
        if k.endswith("layer_norm.weight"):
            v = 1.0 + 0.3 * (2.0 * torch.rand(v.shape, generator=g) - 1.0)
        elif k.endswith("relative_attention_bias.weight"):
            v = math.sqrt(2.0) * torch.randn(v.shape, generator=g)
        sd[k] = v.to(torch.bfloat16)
    model = model.double()
    model.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    ids = torch.randint(0, CFG["vocab_size"], (2, 40), generator=g)
    mask = torch.ones(2, 40, dtype=torch.long)
    mask[0, 29:] = 0
    mask[1, 7:] = 0
    T5LayerNorm.forward = _layer_norm_fp64
    with torch.no_grad():
        out = model(input_ids=ids).last_hidden_state
        out_masked = model(input_ids=ids, attention_mask=mask).last_hidden_state
    assert out.dtype == torch.float64 and out_masked.dtype == torch.float64
    deltas = torch.arange(-511, 512, dtype=torch.long)
    buckets = T5Attention._relative_position_bucket(deltas, bidirectional=True, num_buckets=32, max_distance=128)
    with open(os.path.join(HERE, "t5_names.json"), "w") as f:
        json.dump(names, f, indent=0)
    torch.save({"config": CFG, "state_dict": sd, "input_ids": ids, "attention_mask": mask, "out": out, "out_masked": out_masked,
                "deltas": deltas, "buckets": buckets.to(torch.int16)}, os.path.join(HERE, "t5_tiny.pt"))
    print(len(names), "names;", os.path.getsize(os.path.join(HERE, "t5_tiny.pt")), "bytes")


if __name__ == "__main__":
    main()
