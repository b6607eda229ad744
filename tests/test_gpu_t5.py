"""videogpa_amd.t5 (transformers' T5EncoderModel on the device) and the three kernels of csrc/t5.hip against fp64 references on the CPU
(tests/t5_ref.py; nothing here reads transformers or the reference tree).  -m gpu only.

Bounds, none fitted to a device result; every test prints the device figure next to its bound:
    attention     per element, tests/attn_tol.py::o_tol over the sums of t5_ref.attn_sums64 (bf16 weights, normalised by the ROUNDED row sum, as the
                  kernel does; the score error of the fp32 MFMA accumulation plus one fp32 addition per score for the bias as `det`), and attn_tol's
                  rms(err) / rms(sigma) <= 1.25.  Bit for bit (torch.equal): k / v changed at masked positions, a sample alone against the sample in a
                  batch, no mask against an all-ones mask.
    RMS rows      per element, tests/t5_tol.py::rms_tol (unit-roundoff counts + the bf16 half ulp); the stream output to one fp32 rounding; the
                  gathered rows bit for bit
    gated GELU    per element, tests/t5_tol.py::gated_gelu_tol (row_tol's gelu value bound through the product and the bf16 store)
    whole network || device - o64 ||_2 / || o64 ||_2 <= 1.0 x the same quantity of t5_ref(mode="bf16") on the CPU, the reference's own arithmetic: the
                  device keeps an fp32 stream, so it has to be at least as accurate as the module it replaces.  The bf16 output equals the fp32
                  output rounded once (torch.equal).

Measured on an MI355X (every test prints its own figures next to its bound):
    attention     max err / bound 0.968 ... 0.977 at S = 2 ... 512 (the bf16 store at a mantissa next to 1.0 decides), 0 where a row keeps one key (S = 1, the
                  one-key sample); rms(err) / rms(sigma) 0.878 ... 0.939, 1.001 at S = 2 (bound 1.25)
    RMS rows      fp32 output 0.046 ... 0.30 of the bound (plain and with the add; 0.05 ... 0.11 at D = 4096), bf16 output and the gather 0.99 ... 1.00
                  (the half ulp of the store), the stream inside one rounding, the gathered rows equal
    gated GELU    0.996 (d_ff 96), 1.000 (d_ff 10240)
    whole network device / reference bf16 arithmetic, no mask | mask:
                  (a) 3 x 256, S 226      4.71e-3 / 8.26e-3 = 0.570 | 4.82e-3 / 8.44e-3 = 0.571
                  (b) 2 x 192, q x 8      1.47e-2 / 3.19e-2 = 0.461 | 1.58e-2 / 2.62e-2 = 0.603
                  (c) real width, 1 layer 3.32e-3 / 5.51e-3 = 0.602 | 3.44e-3 / 5.52e-3 = 0.624
                  upstream's tiny golden  4.54e-3 / 7.62e-3 = 0.595 | 4.70e-3 / 7.35e-3 = 0.639
The whole file takes 6 s; the CPU side of (a) 1.7 s and of (c) 1.1 s, once each."""
import functools
import os

import pytest
import torch

import attn_tol
import row_tol as rt
import t5_ref
import t5_tol

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------------------------ attention
ATT_B, ATT_H = 2, 3


@functools.lru_cache(maxsize=None)
def _attn_case(S):
    """qkv bf16 [B,S,3,H,64] (q 0.5 N(0,1): unscaled scores of std 4), the bias table N(0, 2) per bucket with bucket 3 of head 0 (relative position -3)
    at +40 -- from row 3 on every row of head 0 sits on one key -- and the mask: sample 0 keeps its first max(1, S // 3) keys, sample 1 keeps key S // 2"""
    g = torch.Generator().manual_seed(1000 + S)
    qkv = torch.randn(ATT_B, S, 3, ATT_H, 64, generator=g)
    qkv[:, :, 0] *= 0.5
    qkv = qkv.to(torch.bfloat16)
    table = (2.0 ** 0.5) * torch.randn(32, ATT_H, generator=g)
    table[3, 0] = 40.0
    bias = t5_ref.bias_delta_from_table(table, S)
    assert S < 3 or not torch.equal(bias, bias.flip(1))               # asymmetric in the sign of j - i: a transposed index cannot pass
    mask = torch.zeros(ATT_B, S, dtype=torch.uint8)
    mask[0, :max(1, S // 3)] = 1
    mask[1, S // 2] = 1
    return qkv, bias, mask


def _run_attn(qkv, bias, mask):
    from videogpa_amd import ops
    q = qkv.cuda()
    o = ops.t5_attention(q[:, :, 0], q[:, :, 1], q[:, :, 2], bias.cuda(), None if mask is None else mask.cuda())
    torch.cuda.synchronize()
    return o.cpu()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 226, 512])
def test_attention_inside_the_per_element_bound(S, masked):
    qkv, bias, mask = _attn_case(S)
    o = _run_attn(qkv, bias, mask if masked else None)
    assert tuple(o.shape) == (ATT_B, S, ATT_H * 64) and o.dtype == torch.bfloat16
    problems, worst_el, worst_rms = [], 0.0, 0.0
    for b in range(ATT_B):
        for h in range(ATT_H):
            R = t5_ref.attn_sums64(qkv[b, :, 0, h], qkv[b, :, 1, h], qkv[b, :, 2, h], bias[h], mask[b] if masked else None)
            tol, sigma = attn_tol.o_tol(R)
            pr, figs = attn_tol.compare("o", o[b, :, h * 64:(h + 1) * 64], R["o"], tol, sigma, where=f"S {S} b {b} h {h} masked {masked}")
            problems += pr
            worst_el, worst_rms = max(worst_el, figs["max_err_over_tol"]), max(worst_rms, figs["worst_block_rms_ratio"])
    print(f"t5 attention S {S} masked {masked}: max err / bound {worst_el:.3f} (bound 1), rms(err) / rms(sigma) {worst_rms:.3f} (bound {attn_tol.RMS_MAX})")
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("S", [65, 226])
def test_attention_bit_exact_properties(S):
    qkv, bias, mask = _attn_case(S)
    o_masked = _run_attn(qkv, bias, mask)
    g = torch.Generator().manual_seed(5)
    other = qkv.clone()
    gone = (mask == 0)[:, :, None, None].expand(-1, -1, ATT_H, 64)
    for i in (1, 2):                                                  # k and v at the masked positions
        other[:, :, i] = torch.where(gone, (37.0 * torch.randn(ATT_B, S, ATT_H, 64, generator=g)).to(torch.bfloat16), qkv[:, :, i])
    assert not torch.equal(other, qkv)
    assert torch.equal(_run_attn(other, bias, mask), o_masked), "k / v at masked positions reach the output"
    for b in range(ATT_B):
        assert torch.equal(_run_attn(qkv[b:b + 1], bias, mask[b:b + 1]), o_masked[b:b + 1]), f"sample {b} alone differs from the sample in the batch"
    o_none = _run_attn(qkv, bias, None)
    assert torch.equal(_run_attn(qkv, bias, torch.ones_like(mask)), o_none), "an all-ones mask differs from no mask"
    assert not torch.equal(o_none, o_masked)


def test_attention_refuses_more_than_512_tokens():
    from videogpa_amd import ops
    qkv = torch.zeros(1, 513, 3, 1, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="512"):
        ops.t5_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], torch.zeros(1, 1025, device="cuda"))


# ------------------------------------------------------------------------------------------------------------------ RMS rows
@functools.lru_cache(maxsize=None)
def _rms_case(M, D):
    x, y, w, table, ids = t5_tol.rms_inputs(M, D)
    xa = x.double() + y.double()
    return dict(x=x, y=y, w=w, table=table, ids=ids, xa=xa, n_plain=t5_ref.rms64(x, w, 1e-6), n_add=t5_ref.rms64(xa, w, 1e-6),
                n_gather=t5_ref.rms64(table[ids].float(), w, 1e-6))


RMS_SHAPES = [(M, D) for D in (64, 192, 4096) for M in (1, 3, 452)] + [(8200, 64)]          # 8200 rows: past the 2048 x 4 rows of one grid sweep


@pytest.mark.parametrize("M,D", RMS_SHAPES)
def test_rms_rows_inside_the_per_element_bound(M, D):
    from videogpa_amd import ops
    c = _rms_case(M, D)
    x, y, w = c["x"].cuda(), c["y"].cuda(), c["w"].cuda()
    problems = []
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        bf = dt == torch.bfloat16
        xs, n = ops.t5_rms(x, w, None, 1e-6, n_dtype=dt)
        assert xs is None and n.dtype == dt
        tol = t5_tol.rms_tol(c["n_plain"], D, False, bf)
        print(f"t5_rms plain {name} M {M} D {D}: err / bound {rt.worst(n.cpu(), c['n_plain'], tol)[0]:.3f} (bound 1)")
        problems += rt.judge(f"plain {name}", n.cpu(), c["n_plain"], tol)
        xs, n = ops.t5_rms(x, w, y, 1e-6, n_dtype=dt, keep_stream=bf)
        assert (xs is not None) == bf and n.dtype == dt
        tol = t5_tol.rms_tol(c["n_add"], D, True, bf)
        print(f"t5_rms add {name} M {M} D {D}: err / bound {rt.worst(n.cpu(), c['n_add'], tol)[0]:.3f} (bound 1)")
        problems += rt.judge(f"add {name}", n.cpu(), c["n_add"], tol)
        if bf:
            assert xs.dtype == torch.float32
            problems += rt.judge("x_new", xs.cpu(), c["xa"], t5_tol.stream_tol(c["xa"]))
    xs, n = ops.t5_embed_rms(c["ids"].cuda(), c["table"].cuda(), w, 1e-6)
    assert torch.equal(xs.cpu(), c["table"][c["ids"]].float()), "the gathered rows are not the table's"
    tol = t5_tol.rms_tol(c["n_gather"], D, False, True)
    print(f"t5_embed_rms M {M} D {D}: err / bound {rt.worst(n.cpu(), c['n_gather'], tol)[0]:.3f} (bound 1)")
    problems += rt.judge("gather", n.cpu(), c["n_gather"], tol)
    assert not problems, "\n".join(problems)


def test_rms_rows_refusals_and_bad_ids():
    from videogpa_amd import ops
    w = torch.ones(96, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 64"):
        ops.t5_rms(torch.zeros(2, 96, device="cuda"), w)
    with pytest.raises(RuntimeError, match="forward only"):
        with torch.enable_grad():
            ops.t5_rms(torch.zeros(2, 64, device="cuda", requires_grad=True), torch.ones(64, device="cuda"))
    table = torch.ones(8, 64, dtype=torch.bfloat16, device="cuda")
    x, n = ops.t5_embed_rms(torch.tensor([1, 8, -1, 7], device="cuda"), table, torch.ones(64, device="cuda"))
    bad = torch.isnan(x).all(-1).cpu()
    assert bad.tolist() == [False, True, True, False] and torch.isnan(n.float()).all(-1).cpu().tolist() == bad.tolist()


# ------------------------------------------------------------------------------------------------------------------ gated GELU
@pytest.mark.parametrize("F", [96, 10240])
def test_gated_gelu_inside_the_per_element_bound(F):
    from videogpa_amd import ops
    u = t5_tol.gelu_inputs(3, F)
    ref = t5_ref.gated_gelu64(u)
    tol = t5_tol.gated_gelu_tol(u, ref)
    g = ops.t5_gated_gelu(u.cuda())
    assert tuple(g.shape) == (3, F) and g.dtype == torch.bfloat16
    print(f"t5_gated_gelu d_ff {F}: err / bound {rt.worst(g.cpu(), ref, tol)[0]:.3f} (bound 1)")
    assert not rt.judge("gated_gelu", g.cpu(), ref, tol)


# ------------------------------------------------------------------------------------------------------------------ the whole network
NETS = {
    "a": dict(cfg=dict(num_layers=3, d_model=256, num_heads=4, d_ff=640, vocab_size=128), S=226, B=2, q_gain=1.0, seed=11),
    "b": dict(cfg=dict(num_layers=2, d_model=192, num_heads=3, d_ff=320, vocab_size=128), S=77, B=2, q_gain=8.0, seed=12),
    "c": dict(cfg=dict(num_layers=1, d_model=4096, num_heads=64, d_ff=10240, vocab_size=256), S=40, B=2, q_gain=1.0, seed=13),
}


def _net_mask(B, S):
    mask = torch.ones(B, S, dtype=torch.long)
    mask[0, (2 * S) // 3:] = 0
    if B > 1:
        mask[1, max(1, S // 4):] = 0
    return mask


@functools.lru_cache(maxsize=None)
def _net_case(name):
    """state dict (bf16 values, norm weights +-30 %, bias table N(0, 2)), ids, mask, and per mask the fp64 oracle and the error of the reference's bf16 arithmetic"""
    if name == "tiny":
        t = torch.load(os.path.join(GOLDEN, "t5_tiny.pt"))
        cfg, sd, ids, mask = t["config"], t["state_dict"], t["input_ids"], t["attention_mask"]
        o64 = {False: t["out"], True: t["out_masked"]}
    else:
        spec = NETS[name]
        cfg = t5_ref.make_cfg(**spec["cfg"])
        sd = t5_ref.seeded_state_dict(cfg, seed=spec["seed"], q_gain=spec["q_gain"])
        g = torch.Generator().manual_seed(spec["seed"])
        ids = torch.randint(0, cfg["vocab_size"], (spec["B"], spec["S"]), generator=g)
        mask = _net_mask(spec["B"], spec["S"])
        sd64 = t5_ref.prepare(sd, "fp64")
        o64 = {m: t5_ref.forward(sd64, cfg, ids, mask if m else None, "fp64", prepared=True) for m in (False, True)}
        del sd64
    e16 = {m: t5_ref.rel_err(t5_ref.forward(sd, cfg, ids, mask if m else None, "bf16"), o64[m]) for m in (False, True)}
    return cfg, sd, ids, mask, o64, e16


@functools.lru_cache(maxsize=None)
def _net_module(name):
    from videogpa_amd import t5
    cfg, sd = _net_case(name)[:2]
    with torch.device("meta"):
        m = t5.T5EncoderModel(cfg)
    m.load_state_dict({k: v.cuda() for k, v in sd.items()}, strict=True, assign=True)
    m.encoder.embed_tokens.weight = m.shared.weight
    return m


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", ["a", "b", "c", "tiny"])
def test_network_is_at_least_as_accurate_as_the_reference_bf16_module(name, masked):
    cfg, sd, ids, mask, o64, e16 = _net_case(name)
    m = _net_module(name)
    am = mask if masked else None
    out = m(ids, attention_mask=am)
    assert out.last_hidden_state is out[0] and out[0].dtype == torch.bfloat16 and tuple(out[0].shape) == tuple(o64[masked].shape)
    e_dev = t5_ref.rel_err(out[0].cpu(), o64[masked])
    print(f"T5 {name} masked {masked}: device {e_dev:.3e}, reference bf16 arithmetic {e16[masked]:.3e} (the bound), ratio {e_dev / e16[masked]:.3f}")
    out32 = m(ids.cuda(), attention_mask=None if am is None else am.cuda(), output_dtype=torch.float32)[0]
    assert out32.dtype == torch.float32 and torch.equal(out32.to(torch.bfloat16), out[0]), "the bf16 output is not the fp32 output rounded once"
    assert torch.isfinite(out32).all()
    assert e_dev <= 1.0 * e16[masked], (name, masked, e_dev, e16[masked])


# ------------------------------------------------------------------------------------------------------------------ generate
def test_encode_prompt_feeds_denoise_bit_for_bit():
    from oracle import cogvideox as ocv
    from videogpa_amd.generate import denoise, encode_prompt
    from videogpa_amd.scheduler import CogVideoXDPMScheduler
    from videogpa_amd.transformer import CogVideoXTransformer3DModel
    enc = _net_module("tiny")
    ids = _net_case("tiny")[2]
    pos_ids, neg_ids = ids[:1, :6], ids[1:, :6]
    nv = 2
    pos, neg = encode_prompt(enc, pos_ids, neg_ids, num_videos_per_prompt=nv)
    assert tuple(pos.shape) == tuple(neg.shape) == (nv, 6, 64) and pos.dtype == torch.bfloat16
    by_hand = enc(pos_ids)[0]
    assert torch.equal(pos[0], by_hand[0]) and torch.equal(pos[1], by_hand[0])          # repeated per video, in a row
    assert torch.equal(neg[0], enc(neg_ids)[0][0])
    two, none = encode_prompt(enc, ids[:, :6], None, num_videos_per_prompt=3, dtype=torch.float32)
    assert none is None and tuple(two.shape) == (6, 6, 64) and two.dtype == torch.float32
    assert torch.equal(two[0], two[2]) and torch.equal(two[3], two[5]) and not torch.equal(two[0], two[3])
    kw = dict(num_attention_heads=2, attention_head_dim=64, num_layers=1, time_embed_dim=32, text_embed_dim=64, sample_width=8, sample_height=8,
              sample_frames=9, max_text_seq_length=6)
    cfg = ocv.CogVideoXConfig(**kw)
    sd = {k: v.to(torch.bfloat16) for k, v in ocv.init_state_dict(cfg, seed=0, std=0.05, mod_std=0.2).items()}
    model = CogVideoXTransformer3DModel(use_rotary_positional_embeddings=True, **kw)
    model.load_state_dict(sd, strict=True)
    model = model.to(device="cuda", dtype=torch.bfloat16).eval()
    g = torch.Generator().manual_seed(77)
    lat0 = torch.randn(nv, 3, 16, 8, 8, generator=g).to(torch.bfloat16)
    noise = torch.randn(2, 2, nv, 3, 16, 8, 8, generator=g).to(torch.bfloat16)
    run = dict(latent_frames=3, height=8, width=8, num_inference_steps=2, guidance_scale=6.0, latents=lat0.cuda(), step_noise=noise.cuda())
    a = denoise(model, CogVideoXDPMScheduler(timestep_spacing="trailing"), pos, neg, **run)
    hand_pos = by_hand.repeat(1, nv, 1).view(nv, 6, -1)
    hand_neg = enc(neg_ids)[0].repeat(1, nv, 1).view(nv, 6, -1)
    b = denoise(model, CogVideoXDPMScheduler(timestep_spacing="trailing"), hand_pos, hand_neg, **run)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
