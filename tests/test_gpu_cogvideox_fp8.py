"""CogVideoXTransformer3DModel.enable_fp8: the frozen feed-forward on OCP-e4m3 operands written by their producers (csrc/residual_ln.hip
vgpa_residual_ln_{fwd,bwd}_q8, csrc/fp8.hip), ops.ffn_tail_fp8 as one autograd node, the model / trainer switch.  -m gpu only.

The reference (train/CogVideoX-5B/03_train.py) computes these products in bf16; e4m3 is an opt-in deviation, and test 5 below states how far it is."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cogvideox as ocv

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same_q8(q, sc, ref_q, ref_sc, what):
    """the project's contract for a fused e4m3 producer against the unfused chain (tests/test_gpu_wan_kernels.py): equal scales (or within 2^-7), <= 0.1 % of the
    bytes differ (another kernel may contract the same float expression differently: one bf16 ulp before quantisation), dequantised difference <= 0.13 x max"""
    assert torch.equal(sc, ref_sc) or (sc - ref_sc).abs().max().item() <= 2 ** -7 * ref_sc.abs().max().item(), what
    a, b = q.view(torch.uint8), ref_q.view(torch.uint8)
    frac = (a != b).float().mean().item()
    assert frac <= 1e-3, (what, frac)
    assert (q.float() * sc - ref_q.float() * ref_sc).abs().max().item() <= 0.13 * (ref_q.float() * ref_sc).abs().max().item(), what
    return frac


def _mods(B, D, g, std=0.3):
    """(mod [B, 4, D] = shift_v, 1 + scale_v, shift_t, 1 + scale_t ; gates [B, 2, D]) as CogVideoXLayerNormZero.modulation makes them"""
    mod = std * torch.randn(B, 4, D, device="cuda", generator=g)
    mod[:, 1] += 1
    mod[:, 3] += 1
    return mod.contiguous(), (std * torch.randn(B, 2, D, device="cuda", generator=g)).contiguous()


def _zero_rows(q, sc):
    """scale 1 and bytes that encode zero: 0x00, or 0x80 where the bf16 value was -0 (gate 0 times a negative dx), which is what quant_fp8_rows makes of it"""
    return torch.equal(sc, torch.ones_like(sc)) and not (q.view(torch.uint8) & 0x7F).any()


# (B, S, text_len, D): partial 32-row blocks in both ranges / no text, lanes past D (1920 = 3.75 x 512) / all text, NV = 1
PRODUCER_SHAPES = [(2, 75, 5, 3072), (1, 40, 0, 1920), (2, 33, 33, 512)]


@pytest.mark.parametrize("B,S,Lt,D", PRODUCER_SHAPES)
def test_residual_ln_q8_producers_match_the_unfused_chain(B, S, Lt, D):
    """vgpa_residual_ln_fwd_q8 / _bwd_q8  ==  vgpa_residual_ln_fwd / _bwd + vgpa_quant_fp8_rows; x_new, mean, rstd and dx are the bf16 entries' bits.
    Row magnitudes span 1e-3 .. 1e3; the last batch of the forward has modulation and bias chosen so that n == 0, the last batch of the backward gate 0
    so that dy == 0: scale 1, zero bytes."""
    from videogpa_amd import _lib, ops
    g = torch.Generator(device="cuda").manual_seed(100 + D)
    st = torch.cuda.current_stream().cuda_stream
    rows = B * S
    mag = 10.0 ** torch.linspace(-3, 3, rows, device="cuda").view(B, S, 1)
    x = (torch.randn(B, S, D, device="cuda", generator=g) * mag).bfloat16()
    y = (torch.randn(B, S, D, device="cuda", generator=g) * mag).bfloat16()
    mod, gates = _mods(B, D, g)
    ln_w = (1 + 0.2 * torch.randn(D, device="cuda", generator=g)).contiguous()
    ln_b = torch.zeros(D, device="cuda")                     # with a zero bias, 1 + scale == 0 and shift == 0 give n == 0 exactly
    zero_case = B > 1                                        # modulation and gates are per batch: the zero batch needs a second one beside it
    if zero_case:
        mod[B - 1].zero_()
    q = torch.empty(rows, D, dtype=torch.float8_e4m3fn, device="cuda")
    sc = torch.empty(rows, 1, device="cuda")

    # ---- forward
    x_ref, n_ref = ops.residual_ln(x, y, gates, ln_w, ln_b, mod, Lt, 1e-5)
    mean_ref, rstd_ref = torch.empty(B, S, device="cuda"), torch.empty(B, S, device="cuda")
    n2, x2 = torch.empty_like(x), torch.empty_like(x)
    _lib.call("vgpa_residual_ln_fwd", x, y, gates[:, 0], gates[:, 1], gates.stride(0), ln_w, ln_b, mod[:, 0], mod[:, 1], mod[:, 2], mod[:, 3], mod.stride(0),
              B, S, D, Lt, 1e-5, x2, n2, D, mean_ref, rstd_ref, st)
    assert torch.equal(n2, n_ref) and torch.equal(x2, x_ref)
    rq, rs = ops.quant_fp8_rows(n_ref.reshape(rows, D))
    xq, mean, rstd = torch.empty_like(x), torch.empty(B, S, device="cuda"), torch.empty(B, S, device="cuda")
    _lib.call("vgpa_residual_ln_fwd_q8", x, y, gates[:, 0], gates[:, 1], gates.stride(0), ln_w, ln_b, mod[:, 0], mod[:, 1], mod[:, 2], mod[:, 3], mod.stride(0),
              B, S, D, Lt, 1e-5, xq, q, sc, mean, rstd, st)
    assert torch.equal(xq, x_ref) and torch.equal(mean, mean_ref) and torch.equal(rstd, rstd_ref)
    f_fwd = _same_q8(q, sc, rq, rs, "residual_ln_fwd_q8")
    zr = slice((B - 1) * S, rows)
    if zero_case:
        assert not n_ref[B - 1].any()                                          # the case is what it claims to be
        assert _zero_rows(q[zr], sc[zr]) and not q[zr].view(torch.uint8).any()
    # no residual branch (y NULL): the LN-modulate of x alone
    _, n_plain = ops.residual_ln(x, None, None, ln_w, ln_b, mod, Lt, 1e-5)
    _lib.call("vgpa_residual_ln_fwd_q8", x, None, None, None, 0, ln_w, ln_b, mod[:, 0], mod[:, 1], mod[:, 2], mod[:, 3], mod.stride(0),
              B, S, D, Lt, 1e-5, None, q, sc, None, None, st)
    _same_q8(q, sc, *ops.quant_fp8_rows(n_plain.reshape(rows, D)), "residual_ln_fwd_q8 without y")

    # ---- backward (on the forward's saved x_new / mean / rstd)
    gates_b = gates.clone()
    if zero_case:
        gates_b[B - 1].zero_()                                                 # dy == 0 in the last batch
    dn = (torch.randn(B, S, D, device="cuda", generator=g) * mag.flip(1)).bfloat16()
    dres = (torch.randn(B, S, D, device="cuda", generator=g) * mag.flip(1)).bfloat16()
    f_bwd = 0.0
    for r in (dres, None):
        dx_ref, dy_ref = torch.empty_like(x), torch.empty_like(x)
        _lib.call("vgpa_residual_ln_bwd", dn, x_ref, mean_ref, rstd_ref, ln_w, mod[:, 1], mod[:, 3], mod.stride(0), gates_b[:, 0], gates_b[:, 1], gates_b.stride(0),
                  r, B, S, D, Lt, dx_ref, dy_ref, D, st)
        dx = torch.empty_like(x)
        _lib.call("vgpa_residual_ln_bwd_q8", dn, x_ref, mean_ref, rstd_ref, ln_w, mod[:, 1], mod[:, 3], mod.stride(0), gates_b[:, 0], gates_b[:, 1],
                  gates_b.stride(0), r, B, S, D, Lt, dx, q, sc, st)
        assert torch.equal(dx, dx_ref), "dres" if r is not None else "no dres"
        f_bwd = max(f_bwd, _same_q8(q, sc, *ops.quant_fp8_rows(dy_ref.reshape(rows, D)), "residual_ln_bwd_q8"))
        if zero_case:
            assert not dy_ref[B - 1].any() and _zero_rows(q[zr], sc[zr])
    print(json.dumps({"shape": [B, S, Lt, D], "bytes_differing_fwd": f_fwd, "bytes_differing_bwd": f_bwd}))


def test_residual_ln_q8_entries_reject_invalid_arguments():
    from videogpa_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    B, S, D = 1, 8, 512
    x = torch.zeros(B, S, 4104, dtype=torch.bfloat16, device="cuda")         # wide enough for every D tried below
    w = torch.ones(4104, device="cuda")
    q = torch.empty(B * S, 4104, dtype=torch.float8_e4m3fn, device="cuda")
    sc = torch.empty(B * S, 1, device="cuda")
    m = torch.zeros(B, S, device="cuda")

    def fwd(D=D, q=q, sc=sc):
        _lib.call("vgpa_residual_ln_fwd_q8", x, x, w, w, 0, w, w, None, None, None, None, 0, B, S, D, 0, 1e-5, x, q, sc, m, m, st)

    def bwd(D=D, q=q, sc=sc):
        _lib.call("vgpa_residual_ln_bwd_q8", x, x, m, m, w, None, None, 0, w, w, 0, None, B, S, D, 0, x, q, sc, st)
    for call in (fwd, bwd):
        for kw in ({"q": None}, {"sc": None}, {"D": 516}, {"D": 4104}):
            with pytest.raises(RuntimeError, match="invalid argument"):
                call(**kw)


def _tail_inputs(B=2, S=70, Lt=6, D=512, inner=2048, seed=5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = {"x": torch.randn(B, S, D, device="cuda", generator=g).bfloat16(), "a": torch.randn(B, S, D, device="cuda", generator=g).bfloat16()}
    t["mod2"], t["gates1"] = _mods(B, D, g)
    t["nmod"], t["gates2"] = _mods(B, D, g)
    for k in ("w2", "wn"):
        t[k] = (1 + 0.2 * torch.randn(D, device="cuda", generator=g)).contiguous()
    for k in ("b2", "bn"):
        t[k] = (0.1 * torch.randn(D, device="cuda", generator=g)).contiguous()
    t["W1"] = (torch.randn(inner, D, device="cuda", generator=g) / D ** 0.5).bfloat16()
    t["b1"] = (0.1 * torch.randn(inner, device="cuda", generator=g)).bfloat16()
    t["W2"] = (torch.randn(D, inner, device="cuda", generator=g) / inner ** 0.5).bfloat16()
    t["b2f"] = (0.1 * torch.randn(D, device="cuda", generator=g)).bfloat16()
    t["dx"] = torch.randn(B, S, D, device="cuda", generator=g).bfloat16()
    t["dn"] = torch.randn(B, S, D, device="cuda", generator=g).bfloat16()
    return t


def test_ffn_tail_fp8_equals_the_composed_ops_and_is_no_further_from_fp32():
    """ops.ffn_tail_fp8 (one node, operands written by their producers) against residual_ln -> frozen_linear_fp8 -> gelu_tanh -> frozen_linear_fp8 -> residual_ln,
    with LoRA tails behind n_next and behind the attention output's gradient: outputs and input gradients within the bounds of
    test_wan_ffn_fp8_branch_equals_the_composed_ops (max <= 2e-2 of max, relative Frobenius <= 1e-3), and no further from an fp32 torch evaluation of the
    branch than 1.1 x the composed chain's own distance (the 10 % covers the <= 0.1 % of operand bytes the producers may differ in)."""
    from videogpa_amd import ops
    B, S, Lt, D, n_pad, dy_pad = 2, 70, 6, 512, 64, 16
    t = _tail_inputs(B, S, Lt, D)

    def run(fused):
        x, a = t["x"].clone().requires_grad_(True), t["a"].clone().requires_grad_(True)
        if fused:
            xo, nn = ops.ffn_tail_fp8(x, a, t["gates1"], t["w2"], t["b2"], t["mod2"], t["W1"], t["b1"], t["W2"], t["b2f"], t["gates2"], t["wn"], t["bn"], t["nmod"],
                                      1e-5, Lt, 1e-5, n_pad=n_pad, dy_pad=dy_pad)
        else:
            x1, n2 = ops.residual_ln(x, a, t["gates1"], t["w2"], t["b2"], t["mod2"], Lt, 1e-5, dy_pad=dy_pad)
            f = ops.frozen_linear_fp8(ops.gelu_tanh(ops.frozen_linear_fp8(n2, t["W1"], t["b1"])), t["W2"], t["b2f"])
            xo, nn = ops.residual_ln(x1, f, t["gates2"], t["wn"], t["bn"], t["nmod"], Lt, 1e-5, n_pad=n_pad)
        assert ops._padded_base(nn.reshape(B * S, D), D + n_pad) is not None           # n_next is the head of a LoRA-tailed buffer either way
        torch.autograd.backward([xo, nn], [t["dx"], t["dn"]])
        assert ops._padded_base(a.grad.reshape(B * S, D), D + dy_pad) is not None or a.grad.shape == (B, S, D)
        return {"x_out": xo.detach().float(), "n_next": nn.detach().float(), "dx": x.grad.float(), "da": a.grad.float()}

    def fp32():
        x, a = t["x"].float().requires_grad_(True), t["a"].float().requires_grad_(True)

        def spread(v):                # [B, 2, D] (video, text) or the (v, t) pair of a mod -> per token
            return torch.cat([v[:, 1:2].expand(B, Lt, D), v[:, 0:1].expand(B, S - Lt, D)], dim=1)

        def lnm(h, w, b, mod):
            hn = torch.nn.functional.layer_norm(h, (D,), w, b, 1e-5)
            return hn * spread(mod[:, [1, 3]]) + spread(mod[:, [0, 2]])
        x1 = x + spread(t["gates1"]) * a
        u = lnm(x1, t["w2"], t["b2"], t["mod2"]) @ t["W1"].float().T + t["b1"].float()
        f = torch.nn.functional.gelu(u, approximate="tanh") @ t["W2"].float().T + t["b2f"].float()
        xo = x1 + spread(t["gates2"]) * f
        nn = lnm(xo, t["wn"], t["bn"], t["nmod"])
        torch.autograd.backward([xo, nn], [t["dx"].float(), t["dn"].float()])
        return {"x_out": xo.detach(), "n_next": nn.detach(), "dx": x.grad, "da": a.grad}

    fused, comp, ref = run(True), run(False), fp32()
    report = {}
    for k in ("x_out", "n_next", "dx", "da"):
        d = fused[k] - comp[k]
        e_f, e_c = ((fused[k] - ref[k]).norm() / ref[k].norm()).item(), ((comp[k] - ref[k]).norm() / ref[k].norm()).item()
        report[k] = {"max_over_max": d.abs().max().item() / comp[k].abs().max().item(), "rel_fro": (d.norm() / comp[k].norm()).item(),
                     "node_vs_fp32": e_f, "composed_vs_fp32": e_c}
    print(json.dumps(report))
    for k, r in report.items():
        assert r["max_over_max"] <= 2e-2 and r["rel_fro"] <= 1e-3, (k, r)
        assert r["node_vs_fp32"] <= 1.1 * r["composed_vs_fp32"], (k, r)


def _tiny_model(seed=0, r=8, b_std=0.05, heads=8):
    """D = 512, 2 blocks, r = 8 adapters on the reference's targets"""
    from videogpa_amd.lora import LoraConfig, get_peft_model
    from videogpa_amd.transformer import CogVideoXTransformer3DModel
    kw = dict(num_attention_heads=heads, attention_head_dim=64, num_layers=2, time_embed_dim=32, text_embed_dim=48, sample_width=8, sample_height=8,
              sample_frames=9, max_text_seq_length=6)
    cfg = ocv.CogVideoXConfig(**kw)
    sd = {k: v.to(torch.bfloat16) for k, v in ocv.init_state_dict(cfg, seed=seed, std=0.05, mod_std=0.2).items()}
    model = CogVideoXTransformer3DModel(use_rotary_positional_embeddings=True, **kw)
    model.load_state_dict(sd, strict=True)
    pm = get_peft_model(model.to(device="cuda", dtype=torch.bfloat16), LoraConfig(r=r, lora_alpha=2 * r, target_modules=["to_q", "to_k", "to_v", "to_out.0"]))
    own = pm.state_dict()
    for k, v in ocv.init_lora(cfg, r=r, seed=seed + 1, b_std=b_std).items():
        own[k[:-len(".weight")] + ".default.weight"].copy_(v)
    return cfg, pm


def _fwd_bwd(pm, cfg, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = (0.7 * torch.randn(2, 3, cfg.in_channels, 8, 8, generator=g)).to(torch.bfloat16).cuda()
    txt = (0.5 * torch.randn(2, 6, cfg.text_embed_dim, generator=g)).to(torch.bfloat16).cuda()
    dy = torch.randn(x.shape, generator=g).to(torch.bfloat16).cuda()
    pm.zero_grad(set_to_none=True)
    y = pm(x, encoder_hidden_states=txt, timestep=torch.tensor([417, 80]).cuda()).sample
    y.backward(dy)
    return y.detach(), {n: p.grad.clone() for n, p in pm.named_parameters() if "lora_" in n}


def test_enable_fp8_on_then_off_is_the_bf16_path_bit_for_bit():
    cfg, pm = _tiny_model()
    _, never = _tiny_model()
    base = pm.get_base_model()
    y_ref, g_ref = _fwd_bwd(never, cfg)
    base.enable_fp8(True)
    y8, g8 = _fwd_bwd(pm, cfg)
    assert y8.shape == y_ref.shape and torch.isfinite(y8.float()).all() and not torch.equal(y8, y_ref)          # the switch does something ...
    assert ((y8.float() - y_ref.float()).norm() / y_ref.float().norm()).item() < 0.1                          # ... and not much
    assert set(g8) == set(g_ref) and all(torch.isfinite(v.float()).all() and v.abs().max() > 0 for v in g8.values())
    base.enable_fp8(False)
    y_off, g_off = _fwd_bwd(pm, cfg)
    assert torch.equal(y_off, y_ref)
    assert all(torch.equal(g_off[k], g_ref[k]) for k in g_ref)
    # block recompute and lean activations (the cfg4 memory policy) give the same fp8 step: every producer is deterministic
    base.enable_fp8(True)
    base.enable_gradient_checkpointing()
    base.enable_lean_activations(True)
    pm.train()
    y_ck, g_ck = _fwd_bwd(pm, cfg)
    assert torch.equal(y_ck, y8) and all(torch.equal(g_ck[k], g8[k]) for k in g8)


def test_enable_fp8_refuses_trainable_or_lora_wrapped_feed_forward():
    from videogpa_amd.lora import LoraConfig, get_peft_model
    cfg, pm = _tiny_model()
    base = pm.get_base_model().enable_fp8()
    g = torch.Generator().manual_seed(1)
    x = (0.7 * torch.randn(1, 3, cfg.in_channels, 8, 8, generator=g)).to(torch.bfloat16).cuda()
    txt = (0.5 * torch.randn(1, 6, cfg.text_embed_dim, generator=g)).to(torch.bfloat16).cuda()
    base.transformer_blocks[1].ff.net[2].weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="frozen projections only"):
        pm(x, encoder_hidden_states=txt, timestep=torch.tensor([5]).cuda())
    base.transformer_blocks[1].ff.net[2].weight.requires_grad_(False)
    pm(x, encoder_hidden_states=txt, timestep=torch.tensor([5]).cuda())
    for target, name in (("ff.net.0.proj", r"ff\.net\.0\.proj"), ("ff.net.2", r"ff\.net\.2")):
        from videogpa_amd.transformer import CogVideoXTransformer3DModel
        m = CogVideoXTransformer3DModel(num_attention_heads=8, attention_head_dim=64, num_layers=2, time_embed_dim=32, text_embed_dim=48, sample_width=8,
                                        sample_height=8, sample_frames=9, max_text_seq_length=6, use_rotary_positional_embeddings=True)
        wrapped = get_peft_model(m.to(device="cuda", dtype=torch.bfloat16), LoraConfig(r=8, lora_alpha=16, target_modules=["to_q", target]))
        wrapped.get_base_model().enable_fp8()
        with pytest.raises(RuntimeError, match=name):
            wrapped(x, encoder_hidden_states=txt, timestep=torch.tensor([5]).cuda())


def test_generate_denoise_runs_with_fp8_and_keeps_no_backward_state():
    from videogpa_amd import ops
    from videogpa_amd.generate import denoise
    from videogpa_amd.scheduler import CogVideoXDPMScheduler
    cfg, pm = _tiny_model()
    merged = pm.merge_and_unload()
    merged.enable_fp8()
    saved = []
    orig = ops._FfnTailFp8Fn.forward

    def spy(ctx, *a):
        out = orig(ctx, *a)
        saved.append((torch.is_grad_enabled(), any(ctx.needs_input_grad), hasattr(ctx, "w")))
        return out
    ops._FfnTailFp8Fn.forward = staticmethod(spy)
    try:
        g = torch.Generator().manual_seed(77)
        pos = (0.5 * torch.randn(1, 6, cfg.text_embed_dim, generator=g)).to(torch.bfloat16)
        lat0 = torch.randn(1, 3, 16, 8, 8, generator=g).to(torch.bfloat16)
        noise = torch.randn(2, 2, 1, 3, 16, 8, 8, generator=g).to(torch.bfloat16)
        kw = dict(latent_frames=3, height=8, width=8, num_inference_steps=2, guidance_scale=6.0, latents=lat0.cuda(), step_noise=noise.cuda())
        out8 = denoise(merged, CogVideoXDPMScheduler(timestep_spacing="trailing"), pos.cuda(), torch.zeros_like(pos).cuda(), **kw)
    finally:
        ops._FfnTailFp8Fn.forward = orig
    assert len(saved) == 2 * 2 and not any(s[1] or s[2] for s in saved)          # 2 steps x 2 blocks through the node; nothing kept for a backward
    merged.enable_fp8(False)
    out = denoise(merged, CogVideoXDPMScheduler(timestep_spacing="trailing"), pos.cuda(), torch.zeros_like(pos).cuda(), **kw)
    # no closeness bound here: guidance 6 multiplies the difference of two predictions, and with it the e4m3 noise of either (the single forward is bounded above)
    assert out8.shape == out.shape and torch.isfinite(out8.float()).all() and not torch.equal(out8, out)


def test_engine_micro_step_with_fp8_ffn_gives_ln2_at_zero_lora_b():
    """fp8_ffn=True through the trainer's config; lora_B = 0: the policy and the adapter-off reference pass run the same e4m3 forward, so they agree bit for bit
    and the loss is ln 2 as exactly as on the bf16 path (tests/test_gpu_model.py, tests/test_gpu_fullmodel.py: 1e-6)."""
    from videogpa_amd.trainer import CogVideoXDPOTrainer, DPOEngine
    cfg, pm = _tiny_model(b_std=0.0)
    tr = CogVideoXDPOTrainer({"beta": 1.0, "fp8_ffn": True, "accumulate_grad_batches": 1, "learning_rate": 1e-3, "warmup_steps": 0, "max_steps": 4, "seed": 2},
                             transformer=pm)
    assert all(b.fp8_ffn for b in pm.get_base_model().transformer_blocks)
    tr.train()
    eng = DPOEngine(tr)
    g = torch.Generator().manual_seed(3)
    batch = {"x_pair": (0.7 * torch.randn(1, 2, 3, 16, 8, 8, generator=g)).to(torch.bfloat16).cuda(),
             "prompt_emb": (0.5 * torch.randn(1, 6, 48, generator=g)).to(torch.bfloat16).cuda()}
    calls = []
    from videogpa_amd import ops
    orig = ops.ffn_tail_fp8
    ops.ffn_tail_fp8 = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        logs = eng.micro_step(batch)
    finally:
        ops.ffn_tail_fp8 = orig
    eng.flush()
    assert len(calls) == 2 * 2                                                   # reference + policy pass, 2 blocks each: the e4m3 path really ran
    assert abs(float(logs["train/loss"]) - math.log(2.0)) < 1e-6, float(logs["train/loss"])
    gb = [p.grad for n, p in pm.named_parameters() if "lora_B" in n]
    assert all(v is not None and torch.isfinite(v.float()).all() for v in gb)


# Measured on MI355X (profiles/cogvideox_fp8_cfg1_parity.json), variant r64, against the fp32 golden's 256 samples per tensor:
#   e4m3 feed-forward   worst relative error 0.2589 (block 1 to_q.lora_A), lowest cosine 0.96664; block 0 adapters 5.9-10.8 %, block 1 to_q / to_k 17-26 %,
#                       the others 7-13 %; loss 0.693581 against 0.693454; predictions within 4.7 % of their range, norms within 0.5 %
#   bf16 path, same run worst relative error 0.0718, lowest cosine 0.99743; loss 0.693361; predictions within 0.9 % of their range
# Asserted: 1.25 x the measured worst error, and the cosine's distance from 1 widened by the same factor (hipBLASLt may pick another fp8 solution on another
# machine, which changes the accumulation order).  The worst tensor is beyond twice the bf16 path's 10 % bound: a finding, stated in DESIGN section 5.
E8_MEASURED, C8_MEASURED = 0.2589, 0.96664


def test_cfg1_pair_step_with_fp8_ffn_against_the_fp32_golden(tmp_path):
    """BASELINE configs[0] geometry (D = 3072, 2 blocks, S = 13 538, tests/cfg1_common.py, variant r64) with enable_fp8, against tests/golden/cfg1_r64.pt (the fp32
    oracle's loss, prediction samples / norms and, per LoRA gradient, 256 samples and the norm), next to the bf16 path on the same inputs.
    Measured (E8_MEASURED / C8_MEASURED above): worst per-tensor relative error 25.9 %, lowest cosine 0.9666 with e4m3, against 7.2 % /
    0.9974 for the bf16 path in the same run; asserted at 1.25 x: relative error <= 32.4 %, cosine >= 0.9583."""
    import cfg1_common as c1
    from videogpa_amd.lora import LoraConfig, get_peft_model
    from videogpa_amd.trainer import CogVideoXDPOTrainer
    from videogpa_amd.transformer import COGVIDEOX_5B, CogVideoXTransformer3DModel
    variant = "r64"
    gold = torch.load(os.path.join(HERE, "golden", f"cfg1_{variant}.pt"), weights_only=False)
    cfg = c1.config()
    model = CogVideoXTransformer3DModel(**dict(COGVIDEOX_5B, num_layers=cfg.num_layers, sample_height=c1.HEIGHT, sample_width=c1.WIDTH))
    model.load_state_dict(c1.base_state_dict(cfg), strict=True)
    model = model.to(device="cuda", dtype=torch.bfloat16)
    lora, r = c1.lora_state_dict(cfg, variant)
    pm = get_peft_model(model, LoraConfig(r=r, lora_alpha=2 * r, target_modules=["to_q", "to_k", "to_v", "to_out.0"]))
    own = pm.state_dict()
    for k, v in lora.items():
        own[k[:-len(".weight")] + ".default.weight"].copy_(v)
    tr = CogVideoXDPOTrainer({"beta": 1.0, "lean_activations": False}, transformer=pm)
    tr.train()
    x_win, x_lose, prompt, t, noise = c1.inputs()
    batch = {"x_win": x_win.cuda(), "x_lose": x_lose.cuda(), "prompt_emb": prompt.cuda()}
    named = dict(pm.named_parameters())

    def step(fp8):
        model.enable_fp8(fp8)
        pm.zero_grad(set_to_none=True)
        preds = []
        orig = tr.transformer.forward

        def spy(*a, **k):
            out = orig(*a, **k)
            preds.append(out.sample.detach())
            return out
        tr.transformer.forward = spy
        try:
            out = tr._shared_step(batch, timesteps=t.cuda(), noise=noise.cuda())
        finally:
            tr.transformer.forward = orig
        out.loss.backward()
        torch.cuda.synchronize()
        rep = {"loss": out.loss.item(), "loss_golden": float(gold["loss"]), "per_tensor": {}}
        v_ref, v_pol = preds
        for k, v in (("v_win", v_pol[0:1]), ("v_lose", v_pol[1:2]), ("v_win_ref", v_ref[0:1]), ("v_lose_ref", v_ref[1:2])):
            v = v.float().cpu()
            ref = gold[k + "_samples"].float()
            rep[k + "_err_over_range"] = (v.flatten()[c1.sample_index(v.numel(), k)] - ref).abs().max().item() / ref.abs().max().item()
            rep[k + "_norm_rel"] = abs(v.double().norm().item() / float(gold[k + "_norm"]) - 1)
        worst_e, worst_c, worst_n = 0.0, 1.0, 0.0
        for k in lora:
            gr = named[k[:-len(".weight")] + ".default.weight"].grad.detach().double().cpu()
            gs = gold["lora_grads"][k]
            a, b = gr.flatten()[c1.sample_index(gr.numel(), k)], gs["samples"].double()
            e = float((a - b).norm() / b.norm())
            c = float((a * b).sum() / (a.norm() * b.norm()).clamp_min(1e-300))
            n = abs(gr.norm().item() / float(gs["norm"]) - 1)
            rep["per_tensor"][k.replace("base_model.model.transformer_blocks.", "")] = {"rel_err": round(e, 5), "cos": round(c, 6), "norm_rel": round(n, 5)}
            worst_e, worst_c, worst_n = max(worst_e, e), min(worst_c, c), max(worst_n, n)
        rep.update(worst_rel_err=worst_e, worst_cos=worst_c, worst_norm_rel=worst_n)
        return rep

    bf16 = step(False)
    fp8 = step(True)
    report = {"variant": variant, "reference": "fp32 golden samples (256 per tensor) and norms", "fp8_ffn": fp8, "bf16": bf16,
              "asserted": {"rel_err": 1.25 * E8_MEASURED, "cos": 1 - 1.25 * (1 - C8_MEASURED)}}
    out_dir = os.environ.get("VGPA_REPORT_DIR") or str(tmp_path)       # the full report; profiles/cogvideox_fp8_cfg1_parity.json is a copy of one
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "cogvideox_fp8_cfg1_parity.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "per_tensor"} if isinstance(v, dict) else v) for k, v in report.items()}))
    assert math.isfinite(fp8["loss"]) and fp8["worst_rel_err"] <= 1.25 * E8_MEASURED, (fp8["worst_rel_err"], E8_MEASURED)
    assert fp8["worst_cos"] >= 1 - 1.25 * (1 - C8_MEASURED), (fp8["worst_cos"], C8_MEASURED)
