"""Kernels of the Wan2.2-TI2V-5B attention shapes (BASELINE.json configs[5]): head_dim-128 attention with separate query and key
lengths (self-attention, cross-attention over the 512 text tokens), against an fp64 torch reference on the same bf16 inputs.
bf16 outputs: within 2 % of the tensor's range and cosine >= 0.9995 for the output and every gradient."""
import pytest
import torch

import attn_tol
from attn_ref64 import attn_ref64

pytestmark = pytest.mark.gpu


def _ref(q, k, v, do, scale):
    q, k, v = (t.double().requires_grad_(True) for t in (q, k, v))
    p = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
    o = p @ v
    o.backward(do.double())
    return o, q.grad, k.grad, v.grad


def _close(got, ref, what, tol=0.02):
    got, ref = got.detach().double().cpu(), ref.detach().cpu()
    err = (got - ref).abs().max().item()
    if ref.abs().max().item() == 0.0:        # one key: P = 1, so dq and dk vanish identically
        assert err <= 1e-4, (what, err)
        return
    cos = float((got.flatten() @ ref.flatten()) / (got.norm() * ref.norm()).clamp_min(1e-300))
    assert err <= tol * ref.abs().max().item() and cos >= 0.9995, (what, err, ref.abs().max().item(), cos)


@pytest.mark.parametrize("B,H,Sq,Skv", [(1, 2, 128, 128), (2, 3, 300, 300), (1, 2, 257, 64), (1, 4, 200, 512), (1, 1, 64, 77), (1, 2, 1, 130), (1, 1, 130, 1)])
def test_attention128_forward_backward_vs_fp64(B, H, Sq, Skv):
    from videogpa_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = torch.Generator(device="cuda").manual_seed(Sq * 1000 + Skv)
    q = torch.randn(B, H, Sq, 128, device="cuda", generator=g).bfloat16()
    k = torch.randn(B, H, Skv, 128, device="cuda", generator=g).bfloat16()
    v = torch.randn(B, H, Skv, 128, device="cuda", generator=g).bfloat16()
    do = torch.randn(B, H, Sq, 128, device="cuda", generator=g).bfloat16()
    scale = 128 ** -0.5
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = ops.attention128(qg, kg, vg, scale)
    o.backward(do)
    ro, rq, rk, rv = _ref(q, k, v, do, scale)
    _close(o, ro, "o")
    _close(qg.grad, rq, "dq")
    _close(kg.grad, rk, "dk")
    _close(vg.grad, rv, "dv")
    # per element, inside the derived bounds of tests/attn_tol.py (bf16 weights, fp32 row sum of the unrounded ones, delta from the completed output)
    problems = []
    for b in range(B):
        for h in range(H):
            R = attn_ref64(q[b, h], k[b, h], v[b, h], do[b, h], smul=scale * attn_tol.LOG2E, dq_mul=scale, dk_mul=scale, rounded_rowsum=False)
            got = {"o": o[b, h].detach(), "dq": qg.grad[b, h], "dk": kg.grad[b, h], "dv": vg.grad[b, h]}
            problems += attn_tol.judge(got, R, where=f"[{Sq} x {Skv} b{b} h{h}]")[0]
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("B,H,Sq,Skv", [(1, 2, 256, 1024), (1, 3, 700, 1500), (2, 2, 1030, 1091), (1, 1, 64, 4096), (1, 2, 1500, 1024), (1, 1, 2048, 130)])
def test_attention128_w1_forward_long_keys_vs_fp64(B, H, Sq, Skv):
    """Skv >= 1024: the forward runs on the one-wave-per-SIMD / LDS-DMA kernel (row-bound shift, generated loop); ragged query and key tails"""
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(Sq + Skv)
    q = torch.randn(B, H, Sq, 128, device="cuda", generator=g).bfloat16()
    k = torch.randn(B, H, Skv, 128, device="cuda", generator=g).bfloat16()
    v = torch.randn(B, H, Skv, 128, device="cuda", generator=g).bfloat16()
    do = torch.randn(B, H, Sq, 128, device="cuda", generator=g).bfloat16()
    scale = 128 ** -0.5
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = ops.attention128(qg, kg, vg, scale)
    o.backward(do)
    ro, rq, rk, rv = _ref(q, k, v, do, scale)
    _close(o, ro, "o")
    _close(qg.grad, rq, "dq")
    _close(kg.grad, rk, "dk")
    _close(vg.grad, rv, "dv")
    # the log-sum-exp the backward consumed: recompute the forward's lse2 through a second call and compare P row sums implicitly via dv above;
    # and the two forward kernels agree with each other
    import os
    ops.ATTN128_W1 = False
    try:
        o2 = ops.attention128(q, k, v, scale)
    finally:
        ops.ATTN128_W1 = True
    assert (o.float() - o2.float()).abs().max().item() <= 2 ** -7 * ro.abs().max().item()


@pytest.mark.parametrize("Sq,Skv,f8", [(300, 512, False), (1100, 1500, False), (1100, 1500, True), (130, 77, False)])
def test_attention128_output_res8_and_precise_delta(Sq, Skv, f8):
    """"Precise delta" at head_dim 128: every forward kernel of csrc/attention_hd128.hip -- the compiler-scheduled one (short key
    sweeps: the cross-attention), the w1 kernel and the e4m3 kernel -- also writes eight further mantissa bits of its output (uint8 o_res8, csrc/common.h
    res8), and vgpa_attn128_bwd forms delta = rowsum(dO o O) from the completed output.  Diffuse attention over values with a large mean (|O| ~ 2):
    (i) bf16 kernels: the completed output is >= 4x closer to the fp64 output than the bf16 one; every kernel: the residual never exceeds half an ulp and
    was written; (ii) the delta the backward forms (read from its workspace) = rowsum(dO o O_completed) to fp32 rounding, and differs from the plain one;
    (iii) bf16 kernels: dQ is >= 3x closer to the fp64 gradient with the bytes than without (k carries a mean, so sum_j P_ij K_j is not small)."""
    from videogpa_amd import _lib, ops
    g = torch.Generator(device="cuda").manual_seed(Sq * 3 + Skv + int(f8))
    B, H = 1, 2
    tm = lambda t: t.bfloat16().permute(0, 2, 1, 3)                       # token-major storage, [B, H, S, 128] view -- the model's layout
    q = tm(0.3 * torch.randn(B, Sq, H, 128, device="cuda", generator=g))
    k = tm(torch.randn(B, Skv, H, 128, device="cuda", generator=g) + 1.0)
    v = tm(torch.randn(B, Skv, H, 128, device="cuda", generator=g) + 2.0)
    do = tm(torch.randn(B, Sq, H, 128, device="cuda", generator=g))
    scale = 128 ** -0.5
    o_res8 = torch.full((B, Sq, H * 128), 7, dtype=torch.uint8, device="cuda")
    o, lse = ops.attention128_fwd_raw(q, k, v, scale, f8=f8, o_res8=o_res8)
    rv = o_res8.unflatten(-1, (H, 128)).permute(0, 2, 1, 3)
    o_full = ops.res8_decode(o, rv).double()
    res = o_full - o.double()
    assert (res.abs() <= 2.0 ** -8 * o.double().abs() + 1e-30).all()
    assert res.abs().mean().item() > 2.0 ** -12 * o.double().abs().mean().item()
    ro, rq, rk, rvg = _ref(q, k, v, do, scale)
    if not f8:
        e_plain, e_res = (o.double() - ro).abs().max().item(), (o_full - ro).abs().max().item()
        assert e_plain > 2e-3 and e_res < 0.25 * e_plain, (e_plain, e_res)
    errs = {}
    for tag, r8 in (("plain", None), ("res8", o_res8)):
        dq, dk, dv = (torch.empty(B, S_, H, 128, dtype=torch.bfloat16, device="cuda").permute(0, 2, 1, 3) for S_ in (Sq, Skv, Skv))
        ws_bytes = _lib.query("vgpa_attn128_bwd_workspace_bytes", B, H, Sq)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        st = ops._bhs_strides
        _lib.call("vgpa_attn128_bwd", q, k, v, o, do, lse, dq, dk, dv, st(q), st(k), st(v), st(o), st(do), st(dq), st(dk), st(dv),
                  None if r8 is None else rv, None if r8 is None else st(rv), B, H, Sq, Skv, float(scale), -1, ws, ws_bytes, ops._stream())
        delta = ws[: B * H * Sq * 4].view(torch.float32).view(B, H, Sq).double()
        want = (do.double() * (o.double() if r8 is None else o_full)).sum(-1)
        assert (delta - want).abs().max().item() < 1e-4 * want.abs().max().item() + 1e-5, tag
        errs[tag] = float((dq.double() - rq).norm() / rq.norm())
        if not f8:
            _close(dk, rk, tag + " dk", tol=0.03)
            _close(dv, rvg, tag + " dv", tol=0.03)
    if not f8:
        assert errs["res8"] < 0.05 and errs["res8"] < errs["plain"] / 3, errs
    print({"Sq": Sq, "Skv": Skv, "f8": f8, "dq_rel_err_plain_then_res8": errs})


def _ref_e4m3(q, k, v, scale):
    """fp64 attention on the operands the e4m3 forward really multiplies: q * scale * log2(e), k and v rounded to e4m3 after a power-of-two scale per
    (batch, head) and tensor (csrc/attention_hd128.hip attn128_f8_quant_kernel); P is left unquantised (its e4m3 rounding is the remaining difference)"""
    c = scale * 1.4426950408889634

    def q8(t, mul=1.0):
        t = t.float() * mul
        amax = t.abs().amax(dim=(2, 3), keepdim=True)
        e = torch.ceil(torch.log2(amax / 448.0))
        sc = torch.exp2(e)
        return (t / sc).to(torch.float8_e4m3fn).double() * sc.double()
    s2 = q8(q, c) @ q8(k).transpose(-1, -2)                       # log2 units
    p = torch.softmax(s2 * 0.6931471805599453, dim=-1)
    return p @ q8(v), torch.logsumexp(s2 * 0.6931471805599453, -1) / 0.6931471805599453


@pytest.mark.parametrize("B,H,Sq,Skv,qmul,vmean", [(1, 2, 1024, 1024, 1.0, 0.0), (1, 3, 700, 1500, 1.0, 0.0), (2, 2, 1030, 1091, 1.0, 0.0), (1, 1, 64, 4096, 1.0, 0.0),
                                                   (1, 2, 512, 4096, 0.1, 2.0), (1, 2, 300, 2048, 3.0, 0.5)])
def test_attention128_e4m3_forward_vs_fp64(B, H, Sq, Skv, qmul, vmean):
    """vgpa_attn128_fwd_f8 (BASELINE configs[4] "fp8 MFMA path": both products of the forward as v_mfma_scale_f32_32x32x64_f8f6f4) at self-attention
    shapes with ragged query / key tails, on the model's token-major views.  Two references, two stated tolerances:
      (a) fp64 attention over the SAME e4m3-rounded q, k, v (power-of-two scale per head): what is left is the e4m3 rounding of the softmax weights
          (2^-4 relative per weight: 2.6 % of a noise-like output, measured) and fp32 accumulation -- output within 6 % of the tensor's range, cosine
          >= 0.9993, lse2 (made from the unquantised weights) within 2e-3;
      (b) plain fp64 attention on the bf16 inputs: the price of e4m3 itself -- with unit-normal q and k a score carries an error of ~0.05 (|q| |k| d^-1/2
          times 2^-4 / sqrt(d)), i.e. ~5 % per weight: output cosine >= 0.995 and relative error <= 12 % for random v (a noise-like sum), <= 1 % for the
          diffuse case with a coherent v."""
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(Sq * 7 + Skv)
    q = (qmul * torch.randn(B, Sq, H, 128, device="cuda", generator=g)).bfloat16().permute(0, 2, 1, 3)
    k = torch.randn(B, Skv, H, 128, device="cuda", generator=g).bfloat16().permute(0, 2, 1, 3)
    v = (torch.randn(B, Skv, H, 128, device="cuda", generator=g) + vmean).bfloat16().permute(0, 2, 1, 3)
    scale = 128 ** -0.5
    o, lse = ops.attention128_fwd_raw(q, k, v, scale, f8=True)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all() and o.permute(0, 2, 1, 3).is_contiguous()
    r8, l8 = _ref_e4m3(q, k, v, scale)
    ro = torch.softmax((q.double() @ k.double().transpose(-1, -2)) * scale, dim=-1) @ v.double()

    def rel(a, r):
        return float((a.double() - r).norm() / r.norm())

    def cos(a, r):
        a, r = a.double().flatten(), r.flatten()
        return float(a @ r / (a.norm() * r.norm()))
    assert (o.double() - r8).abs().max().item() <= 0.06 * r8.abs().max().item() and cos(o, r8) >= 0.9993, ((o.double() - r8).abs().max().item() / r8.abs().max().item(), cos(o, r8))
    assert (lse.double() - l8).abs().max().item() <= 2e-3, (lse.double() - l8).abs().max().item()
    assert cos(o, ro) >= 0.995 and rel(o, ro) <= (0.01 if vmean >= 2.0 else 0.12), (cos(o, ro), rel(o, ro))
    # the same call is deterministic (atomicMax statistics only): the frozen-reference pass and the policy pass at B = 0 must agree bit for bit
    o2, lse2 = ops.attention128_fwd_raw(q, k, v, scale, f8=True)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("gain,expect", [(1.0, "none"), (2.5, "none"), (3.0, "few"), (4.0, "any")])
def test_attention128_e4m3_forward_keeps_sharp_rows_on_the_e4m3_kernel(gain, expect):
    """Round 6: the e4m3 forward's shift follows a sampled row maximum too (M' = bound - floor(bound - (sampled maximum + 64)): an integer step off the bound, so
    the per-tile E8M0 of P moves with it and the P8 bits stay those of the bound-shifted model).  With RMS-normed q / k at a gain of 2.5 (what `bench.py --config cfg5
    --weights trained_like` runs) every row lies > 100 log2 units under |q8| max|k8|: the bound-shifted kernel flagged EVERY strip and the launch took 14.3 ms instead
    of 4.1 (profiles/r06_bench_cfg5_trained_like.json, before).  Asserted, against fp64 attention over the operands the kernel itself dequantised (so that only the
    e4m3 rounding of the weights -- 2^-4 per weight, clamped at 448 -- and the matrix pipe's accumulation are left): lse2 (from the unquantised weights), output cosine
    >= 0.999 and within 0.15 of the value range per element (a one-hot row carries its weight's rounding whole); the injected oracle model (oracle/wan.py::_F8Attn,
    which restates the shift) as close; and the fraction of strips handed to the bf16 redo pass."""
    from oracle import wan as ow
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(int(gain * 10))
    B, H, S = 1, 3, 2304

    def rms(t):
        return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-6)
    w = gain * (1 + 0.2 * torch.randn(H, 1, 128, device="cuda", generator=g))
    w[..., :3] *= 3.0
    q = (rms(torch.randn(B, H, S, 128, device="cuda", generator=g)) * w).bfloat16()
    k = (rms(torch.randn(B, H, S, 128, device="cuda", generator=g)) * w).bfloat16()
    # every query is matched to one key (cosine 0.6), as a trained attention row is: the row maximum stands far above the sampled keys
    idx = torch.randperm(S, device="cuda", generator=g)
    k = (0.8 * k.float() + 0.6 * q.float()[:, :, idx]).bfloat16()
    v = torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16()
    scale = 128 ** -0.5
    rep = {}
    deq = tuple(torch.empty(B, S, H * 128, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    o, lse = ops.attention128_fwd_raw(q, k, v, scale, f8=True, deq=deq, report=rep)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    qd, kd, vd = (t.unflatten(-1, (H, 128)).permute(0, 2, 1, 3).double() for t in deq)
    s2 = qd @ kd.transpose(-1, -2)                                     # log2 units: q_deq is pre-scaled
    r8 = torch.softmax(s2 * 0.6931471805599453, dim=-1) @ vd
    l8 = torch.logsumexp(s2 * 0.6931471805599453, -1) / 0.6931471805599453

    def cos(a, r):
        a, r = a.double().flatten(), r.flatten()
        return float(a @ r / (a.norm() * r.norm()))
    # lse2: the scaled e4m3 MFMA sums each 64-term block (srcC = -M' included) with ~13 bits relative to the largest addend -- measured 2.7e-3 at |M'| ~ 25 (gain 1),
    # 3.1e-2 at ~130 (gain 2.5): 2^-12 |M'|, the same with the bound as the shift (there |M| is larger still); stated as 1e-3 + 5e-4 max|lse2|
    lerr = (lse.double() - l8).abs().max().item()
    assert lerr <= 1e-3 + 5e-4 * l8.abs().max().item(), (lerr, l8.abs().max().item())
    assert cos(o, r8) >= 0.999 and (o.double() - r8).abs().max().item() <= 0.15 * vd.abs().max().item(), (cos(o, r8), (o.double() - r8).abs().max().item())
    model = ow._F8Attn.apply(q.double(), k.double(), v.double(), True, True)
    assert cos(model, r8) >= 0.995 and cos(o, model) >= 0.995, (cos(model, r8), cos(o, model))      # the model quantises in fp64: ties fall differently on a few operands
    f = rep["redo_fraction"]
    # gain 4 at head_dim 128 is the cliff (the matched key stands > ~180 log2 units above the 64 sampled ones in every strip: all redone in bf16, results as exact)
    assert f == 0.0 if expect == "none" else (f <= 0.5 if expect == "few" else True), (gain, f)
    print(f"e4m3 forward, gain {gain}: redo fraction {f:.4f}, lse2 error {lerr:.2e} at max|lse2| {l8.abs().max().item():.1f}, cos vs fp64 on its operands {cos(o, r8):.5f}, oracle model {cos(model, r8):.5f}")


def test_attention128_e4m3_forward_hands_its_backward_the_operands_it_used():
    """the backward of the e4m3 forward is the straight-through gradient of THAT forward.  vgpa_attn128_fwd_f8 also writes the operands its
    products ran on, dequantised to bf16 (deq) -- exactly: an e4m3 value times a power of two is a bf16 number; the bf16 backward kernels run on them.
    (i) q_deq / k_deq / v_deq equal the oracle's e4m3 operands bit for bit (oracle/wan.py f8_operands: the same power-of-two scales, round to nearest even; q_deq is
    the query PRE-SCALED by d^-1/2 log2 e); (ii) softmax weights recomputed from (q_deq, k_deq) against the forward's lse2 sum to one within 1e-4 per row (what is
    left is fp32 accumulation and the fp32 log2 / exp2; round 5 handed over q8 / c rounded to bf16: 5e-3 worst here, tens of per cent on rows with scores of
    hundreds of log2 units) -- from the bf16 q, k they miss by several percent; (iii) dq / dk / dv of vgpa_attn128_bwd_prescaled on the dequantised operands
    follow the fp64 model of forward + backward (oracle/wan.py::_F8Attn): cosine >= 0.999, norm within 2 %."""
    from oracle import wan as ow
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(91)
    B, H, S = 2, 3, 1300
    tm = lambda t: t.bfloat16().permute(0, 2, 1, 3)
    q = tm(torch.randn(B, S, H, 128, device="cuda", generator=g) + 0.3)
    k = tm(torch.randn(B, S, H, 128, device="cuda", generator=g) + 0.5)
    v = tm(torch.randn(B, S, H, 128, device="cuda", generator=g) + 1.0)
    do = tm(torch.randn(B, S, H, 128, device="cuda", generator=g))
    scale = 128 ** -0.5
    deq = tuple(torch.full((B, S, H * 128), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(3))
    o_res8 = torch.empty(B, S, H * 128, dtype=torch.uint8, device="cuda")
    o, lse = ops.attention128_fwd_raw(q, k, v, scale, f8=True, o_res8=o_res8, deq=deq)
    o_plain, lse_plain = ops.attention128_fwd_raw(q, k, v, scale, f8=True)
    assert torch.equal(o, o_plain) and torch.equal(lse, lse_plain)                    # the extra outputs change nothing else
    qd, kd, vd = (t.unflatten(-1, (H, 128)).permute(0, 2, 1, 3) for t in deq)
    q8, k8, v8, c = ow.f8_operands(q.double(), k.double(), v.double())
    assert torch.equal(kd.double(), k8) and torch.equal(vd.double(), v8)
    # q8 carries the fp32 product q * (scale log2 e) rounded to e4m3: a value that sits on a rounding boundary can land one e4m3 step off the fp64 oracle's
    assert ((qd.double() - q8).abs() <= 2.0 ** -3 * q8.abs() + 1e-30).all() and (qd.double() != q8).double().mean().item() < 0.01
    LOG2E = 1.4426950408889634
    rows_deq = torch.exp2(qd.double() @ kd.double().transpose(-1, -2) - lse.double()[..., None]).sum(-1)
    rows_bf16 = torch.exp2((q.double() @ k.double().transpose(-1, -2)) * (scale * LOG2E) - lse.double()[..., None]).sum(-1)
    assert (rows_deq - 1).abs().max().item() <= 1e-4, ((rows_deq - 1).abs().max().item(), (rows_deq - 1).abs().mean().item())
    assert (rows_bf16 - 1).abs().max().item() > 5 * (rows_deq - 1).abs().max().item()
    dq, dk, dv = (torch.empty(B, S, H, 128, dtype=torch.bfloat16, device="cuda").permute(0, 2, 1, 3) for _ in range(3))
    ops.attention128_bwd_raw(qd, kd, vd, o, do, lse, dq, dk, dv, scale, o_res8=o_res8, q_prescaled=True)
    qr, kr, vr = (t.double().detach().requires_grad_(True) for t in (q, k, v))
    ow._F8Attn.apply(qr, kr, vr, True, True).backward(do.double())
    worst = {}
    for name, got, ref in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        a, r = got.double().flatten(), ref.flatten()
        cos, nrm = float(a @ r / (a.norm() * r.norm())), abs(float(a.norm() / r.norm()) - 1)
        worst[name] = (round(cos, 6), round(nrm, 5))
        assert cos >= 0.999 and nrm <= 0.02, (name, cos, nrm)
    print({"e4m3 forward + backward on its dequantised operands vs the fp64 model": worst, "row sum error deq / bf16": ((rows_deq - 1).abs().max().item(), (rows_bf16 - 1).abs().max().item())})
    # argument errors: the three buffers come together, with the right shapes and dtype, and only the e4m3 kernel writes them
    from videogpa_amd import _lib
    st = ops._bhs_strides
    ws_bytes = _lib.query("vgpa_attn128_fwd_f8_workspace_bytes", B, H, S, S)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="invalid argument"):           # q_deq without k_deq / v_deq
        _lib.call("vgpa_attn128_fwd_f8", q, k, v, o, lse, st(q), st(k), st(v), st(o), None, None, qd, None, None, st(qd), None, None, B, H, S, S, float(scale),
                  ws, ws_bytes, ops._stream())
    with pytest.raises(TypeError):
        ops.attention128_fwd_raw(q, k, v, scale, f8=True, deq=(deq[0], deq[1], deq[2].float()))
    with pytest.raises(ValueError):
        ops.attention128_fwd_raw(q, k, v, scale, f8=False, deq=deq)


@pytest.mark.parametrize("B,H,Sq,Skv", [(2, 24, 2560, 512), (1, 3, 2100, 77), (1, 2, 4000, 130), (1, 1, 2048, 1), (1, 2, 2049, 500)])
def test_attention128_many_queries_over_short_key_sweeps_vs_fp64(B, H, Sq, Skv):
    """Many query rows over a short key sweep (the Wan2.2 cross-attention: 18 480 x 512), at more tasks than CUs, with ragged key tails (77, 130, 500, a single
    key), a ragged last query tile and token-major views: output, lse2 and the res8 bytes against fp64, and the backward that consumes them (dq / dk / dv through
    ops.attention128)."""
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(Sq * 5 + Skv)
    tm = lambda t: t.bfloat16().permute(0, 2, 1, 3)
    q = tm(torch.randn(B, Sq, H, 128, device="cuda", generator=g))
    k = tm(torch.randn(B, Skv, H, 128, device="cuda", generator=g) + 0.5)
    v = tm(torch.randn(B, Skv, H, 128, device="cuda", generator=g) + 1.0)
    do = tm(torch.randn(B, Sq, H, 128, device="cuda", generator=g))
    scale = 128 ** -0.5
    o_res8 = torch.full((B, Sq, H * 128), 7, dtype=torch.uint8, device="cuda")
    o, lse = ops.attention128_fwd_raw(q, k, v, scale, o_res8=o_res8)
    ro, rq, rk, rv = _ref(q, k, v, do, scale)
    _close(o, ro, "o")
    want_lse = torch.logsumexp((q.double() @ k.double().transpose(-1, -2)) * scale, dim=-1) / 0.6931471805599453
    assert (lse.double() - want_lse).abs().max().item() <= 2e-3
    o_full = ops.res8_decode(o, o_res8.unflatten(-1, (H, 128)).permute(0, 2, 1, 3)).double()
    assert ((o_full - o.double()).abs() <= 2.0 ** -8 * o.double().abs() + 1e-30).all()
    assert (o_full - ro).abs().max().item() <= 0.3 * max((o.double() - ro).abs().max().item(), 1e-3)        # the bytes really complete the output
    o2, lse2 = ops.attention128_fwd_raw(q, k, v, scale)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)                                                      # deterministic; res8 changes nothing else
    qg, kg, vg = (t.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for t in (q, k, v))
    ops.attention128(qg, kg, vg, scale).backward(do)
    _close(qg.grad, rq, "dq", tol=0.03)
    _close(kg.grad, rk, "dk", tol=0.03)
    _close(vg.grad, rv, "dv", tol=0.03)


def test_attention128_e4m3_flagged_strips_are_redone_on_the_dequantised_operands():
    """a strip the e4m3 kernel flags is recomputed by the bf16 running-max kernel; with deq buffers supplied that pass runs on the dequantised operands
    (q_deq pre-scaled: c = 1 there), so the recomputed softmax rows of (q_deq, k_deq) against lse2 sum to one on the flagged rows like on all others, and the output
    there is the softmax of (q_deq, k_deq, v_deq) to bf16 accuracy.  Since round 6 the shift follows a sampled row maximum, so a strip is flagged only when a row's
    true maximum stands > ~180 log2 units above the sampled one: here one head carries a 100 x key at a position the 64-key sample does not visit (scores of +-400
    log2 units: every strip of that head has such rows).  Rows that stay on the e4m3 kernel are held to the e4m3 tolerance."""
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(92)
    B, H, S = 1, 2, 1280
    tm = lambda t: t.bfloat16().permute(0, 2, 1, 3)
    q = tm(torch.randn(B, S, H, 128, device="cuda", generator=g))
    kk = torch.randn(B, S, H, 128, device="cuda", generator=g)
    assert 707 % (S // 64) != 0
    kk[:, 707, 1] *= 100.0                                   # head 1: one huge key the sample misses
    k = tm(kk)
    v = tm(torch.randn(B, S, H, 128, device="cuda", generator=g))
    scale = 128 ** -0.5
    deq = tuple(torch.full((B, S, H * 128), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(3))
    rep = {}
    o, lse = ops.attention128_fwd_raw(q, k, v, scale, f8=True, deq=deq, report=rep)
    flags = rep["strip_flags"]                               # [B, H, 5]
    assert not flags[:, 0].any() and flags[:, 1].float().mean().item() >= 0.6, flags
    qd, kd, vd = (t.unflatten(-1, (H, 128)).permute(0, 2, 1, 3).double() for t in deq)
    LOG2E = 1.4426950408889634
    s2 = qd @ kd.transpose(-1, -2)                            # q_deq is pre-scaled by scale * log2 e
    rows = torch.exp2(s2 - lse.double()[..., None]).sum(-1)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    assert (rows - 1).abs().max().item() <= 2e-3, (rows - 1).abs().max().item()        # redone rows (bf16 kernel on the exact operands) and e4m3 rows alike
    ref = torch.softmax(s2 / LOG2E, dim=-1) @ vd
    got = o.double()                                       # attention128_fwd_raw returns the [B,H,S,128] view of its token-major storage
    redone = flags.repeat_interleave(256, dim=-1)[..., :S]                                          # [B, H, S]
    err = (got - ref).abs()
    assert (err[redone] <= 0.03 + 0.03 * ref[redone].abs()).all(), err[redone].max().item()         # bf16 accuracy where the bf16 kernel ran
    assert (err[~redone] <= 0.08 * ref.abs().max()).all(), err[~redone].max().item()                # e4m3 weights elsewhere


@pytest.mark.parametrize("gap,f8", [(126.5, False), (104.0, False), (90.0, False), (126.5, True)])
def test_attention128_row_between_overflow_of_o_and_overflow_of_l(gap, f8):
    """as tests/test_gpu_kernels.py::test_attention_row_between_overflow_of_o_and_overflow_of_l, for the head_dim-128 forwards (same sampled shift): one key the
    64-key sample does not see lifts a row's maximum `gap` log2 units above M' -- the row sum stays finite, the O accumulators overflow; the strip has to be
    flagged and redone (gap 90: stays on the fast path and must be right there).  The e4m3 forward is run on the same operands (its shift is the row bound)."""
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1280 + int(gap))
    B, H, S = 1, 2, 1280
    q, k, v = (torch.randn(B, H, S, 128, device="cuda", generator=g).bfloat16() for _ in range(3))
    scale = 128 ** -0.5
    LOG2E = 1.4426950408889634
    row, key = 5, 7
    assert key % (S // 64) != 0
    s_row = (q[0, 1, row].double() @ k[0, 1].double().t()) * (scale * LOG2E)
    ms = s_row[torch.arange(64, device="cuda") * (S // 64)].max().item()
    want = ms + 64.0 + gap
    k[0, 1, key] = (q[0, 1, row].float() * (want / (float(q[0, 1, row].double() @ q[0, 1, row].double()) * scale * LOG2E))).bfloat16()
    v[0, 1, key] = (8.0 * torch.sign(v[0, 1, key].float())).bfloat16()
    s2 = (q.double() @ k.double().transpose(-1, -2)) * (scale * LOG2E)
    bound = q[0, 1, row].double().norm() * k[0, 1].double().norm(dim=-1).max() * (scale * LOG2E)
    got_gap = s2[0, 1, row].max().item() - min(bound.item(), ms + 64.0)
    assert abs(got_gap - gap) < 1.0, got_gap
    o, lse = ops.attention128_fwd_raw(q, k, v, scale, f8=f8)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    w = torch.softmax(s2 / LOG2E, dim=-1)
    ref = w @ v.double()
    lse_ref = torch.logsumexp(s2 / LOG2E, dim=-1) * LOG2E
    if f8:          # e4m3 operands: the one-hot row is exact to e4m3's rounding of v (8 is representable), the others to the e4m3 model's accuracy
        assert ((o.double() - ref)[0, 1, row].abs() <= 0.05 + 0.07 * ref[0, 1, row].abs()).all()
        a, r = o.double().flatten(), ref.flatten()
        assert float(a @ r / (a.norm() * r.norm())) >= 0.99
    else:
        assert ((o.double() - ref).abs() <= 0.02 + 0.008 * ref.abs()).all(), (o.double() - ref).abs().max().item()
        assert ((lse.double() - lse_ref).abs() <= 2e-3 + 2e-5 * lse_ref.abs()).all()


def test_attention128_e4m3_outlier_rows_and_short_sweeps():
    """a 40x query row, a 40x key row, and a 512-key sweep (below ATTN128_F8_MIN_KEYS: the bf16 kernels serve it -- the Wan2.2 cross-attention over the text
    tokens).  Until round 6 both outlier cases ended in the bf16 redo pass (the shift was the row bound, and a 40x key makes every bound loose); with the sampled
    shift they stay on the e4m3 kernel, and the 40x key shows what e4m3 SCORES cost there: the score error grows with |q| |k| (two e4m3 roundings over 128
    terms: ~2 log2 units against that key), so rows whose weight on it is marginal come out differently -- cosine 0.993 against plain fp64 attention where the
    diffuse case holds 0.995 (the accuracy of the e4m3 forward scales with the score range)."""
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(78)
    B, H, Sq, Skv = 1, 2, 600, 1200
    scale = 128 ** -0.5
    for which in ("q", "k"):
        q = torch.randn(B, H, Sq, 128, device="cuda", generator=g).bfloat16()
        k = torch.randn(B, H, Skv, 128, device="cuda", generator=g).bfloat16()
        v = torch.randn(B, H, Skv, 128, device="cuda", generator=g).bfloat16()
        if which == "q":
            q[0, 0, 300] *= 40
        else:
            k[0, 1, 17] *= 40
        o, _ = ops.attention128_fwd_raw(q, k, v, scale, f8=True)
        ro = torch.softmax((q.double() @ k.double().transpose(-1, -2)) * scale, dim=-1) @ v.double()
        assert torch.isfinite(o).all()
        a, r = o.double().flatten(), ro.flatten()
        assert float(a @ r / (a.norm() * r.norm())) >= (0.995 if which == "q" else 0.99), which
    q = torch.randn(1, 2, 300, 128, device="cuda", generator=g).bfloat16()
    k, v = (torch.randn(1, 2, 512, 128, device="cuda", generator=g).bfloat16() for _ in range(2))
    o8, l8 = ops.attention128_fwd_raw(q, k, v, scale, f8=True)
    ob, lb = ops.attention128_fwd_raw(q, k, v, scale)
    assert torch.equal(o8, ob) and torch.equal(l8, lb)


def test_attention128_w1_kernels_on_token_major_views():
    """the layout the Wan model uses: [B, S, H, 128] storage (projection outputs) viewed as [B, H, S, 128], long enough for all three w1 kernels"""
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(123)
    B, H, Sq, Skv = 2, 3, 1100, 1200
    q = torch.randn(B, Sq, H, 128, device="cuda", generator=g).bfloat16().permute(0, 2, 1, 3)
    kv = torch.randn(B, Skv, 2, H, 128, device="cuda", generator=g).bfloat16()
    k, v = kv[:, :, 0].permute(0, 2, 1, 3), kv[:, :, 1].permute(0, 2, 1, 3)
    do = torch.randn(B, Sq, H, 128, device="cuda", generator=g).bfloat16().permute(0, 2, 1, 3)
    qg, kg, vg = (t.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for t in (q, k, v))
    assert not qg.is_contiguous() and qg.stride(3) == 1
    o = ops.attention128(qg, kg, vg, 128 ** -0.5)
    assert o.permute(0, 2, 1, 3).is_contiguous()                       # token-major storage behind the view
    o.backward(do)
    assert qg.grad.shape == q.shape
    ro, rq, rk, rv = _ref(q, k, v, do, 128 ** -0.5)
    _close(o, ro, "o")
    _close(qg.grad, rq, "dq")
    _close(kg.grad, rk, "dk")
    _close(vg.grad, rv, "dv")


def test_attention128_w1_outlier_rows_take_the_redo_path():
    """a query row 40x larger than the rest: its bound M exceeds 160 -> the strip is flagged and redone with the running-max kernel; a key
    40x larger makes EVERY bound loose (sums underflow) -> all strips redone.  Results must stay within the usual tolerance either way."""
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(77)
    B, H, Sq, Skv = 1, 2, 600, 1200
    for which in ("q", "k"):
        q = torch.randn(B, H, Sq, 128, device="cuda", generator=g).bfloat16()
        k = torch.randn(B, H, Skv, 128, device="cuda", generator=g).bfloat16()
        v = torch.randn(B, H, Skv, 128, device="cuda", generator=g).bfloat16()
        if which == "q":
            q[0, 0, 300] *= 40
        else:
            k[0, 1, 17] *= 40
        o = ops.attention128(q, k, v, 128 ** -0.5)
        ro = torch.softmax((q.double() @ k.double().transpose(-1, -2)) * 128 ** -0.5, dim=-1) @ v.double()
        assert torch.isfinite(o).all()
        _close(o, ro, "o " + which)


def test_attention128_strided_views_and_sharp_softmax():
    """[B, S, H, 128] storage viewed as [B, H, S, 128] (how the projection leaves q/k/v), and scores large enough that the running max
    moves tile to tile (scale 1.0 on unit-variance rows of 128: |s| up to ~40)."""
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    B, H, Sq, Skv = 2, 3, 190, 333
    qs = torch.randn(B, Sq, H, 128, device="cuda", generator=g).bfloat16()
    kvs = torch.randn(B, Skv, 2, H, 128, device="cuda", generator=g).bfloat16()
    q, k, v = qs.permute(0, 2, 1, 3), kvs[:, :, 0].permute(0, 2, 1, 3), kvs[:, :, 1].permute(0, 2, 1, 3)
    do = torch.randn(B, H, Sq, 128, device="cuda", generator=g).bfloat16()
    qg, kg, vg = (t.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for t in (q, k, v))
    assert not qg.is_contiguous()
    o = ops.attention128(qg, kg, vg, 1.0)
    o.backward(do)
    ro, rq, rk, rv = _ref(q, k, v, do, 1.0)
    _close(o, ro, "o")
    _close(qg.grad, rq, "dq", 0.03)
    _close(kg.grad, rk, "dk", 0.03)
    _close(vg.grad, rv, "dv", 0.03)


# ------------------------------------------------------------------------------------------------ row kernels of the block (csrc/wan.hip)
def _tab(G, n, C, g):
    return (torch.randn(G, n, C, device="cuda", generator=g) * 0.5).contiguous()


@pytest.mark.parametrize("xdt,affine,mod,rnd", [(torch.float32, False, True, False), (torch.bfloat16, False, True, True), (torch.float32, True, False, False)])
def test_wan_ln_mod_forward_backward(xdt, affine, mod, rnd):
    from videogpa_amd.wan_model import ln_mod
    g = torch.Generator(device="cuda").manual_seed(1)
    rows, C, G = 300, 3072, 3
    x = (torch.randn(rows, C, device="cuda", generator=g) * 2 + 0.3).to(xdt)
    gid = torch.randint(0, G, (rows,), device="cuda", generator=g).int()
    tab = _tab(G, 6, C, g)
    w = torch.randn(C, device="cuda", generator=g) if affine else None
    b = torch.randn(C, device="cuda", generator=g) if affine else None
    dy = torch.randn(rows, C, device="cuda", generator=g).bfloat16()
    xg = x.clone().requires_grad_(True)
    out = ln_mod(xg, gid if mod else None, w, b, tab[:, 3] if mod else None, tab[:, 4] if mod else None, 1e-6, round_xhat=rnd)
    out.backward(dy)
    xr = x.double().requires_grad_(True)
    h = torch.nn.functional.layer_norm(xr, (C,), None, None, 1e-6)
    if rnd:
        h = h + (h.detach().bfloat16().double() - h.detach())           # value rounded, gradient straight through (.type_as)
    if affine:
        h = h * w.double() + b.double()
    if mod:
        h = h * (1 + tab[:, 4].double()[gid.long()]) + tab[:, 3].double()[gid.long()]
    h.backward(dy.double())
    assert out.dtype == torch.bfloat16 and (out.double() - h.detach()).abs().max().item() <= 2 ** -8 * h.detach().abs().max().item()
    assert xg.grad.dtype == xdt
    tol = 1e-5 if xdt == torch.float32 else 2 ** -8
    assert (xg.grad.double() - xr.grad).abs().max().item() <= tol * xr.grad.abs().max().item()
    # per element (tests/row_tol.py): the reference is the unrounded expression, round_xhat's half ulp is part of the bound; mean and rstd are judged, and the
    # gradient is held to the expression evaluated from them.  The C entry is called once more for them: the same kernel on the same input writes the same bits
    import row_tol
    from videogpa_amd import _lib
    a = (x, gid if mod else None, w, b, tab[:, 3] if mod else None, tab[:, 4] if mod else None, 1e-6)
    mean, rstd, o2 = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda"), torch.empty_like(out)
    _lib.call("vgpa_wan_ln_mod_fwd", x, 0 if xdt == torch.float32 else 1, None, None, None, a[1], w, b, a[4], a[5], tab.stride(0), rows, C, 1e-6, int(rnd), o2, 1, C,
              None, None, mean, rstd, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(o2, out.detach())
    ref = row_tol.wan_ln_fwd_ref64(*a)
    tols = row_tol.wan_ln_fwd_tol(*a, rnd, ref[0])
    for name, got, r, t in zip(("out", "mean", "rstd"), (out.detach(), mean, rstd), ref, tols):
        assert not row_tol.judge(f"wan ln_mod {name}", got, r, t)
    g64, cg = row_tol.wan_ln_bwd_g64(dy, a[1], w, a[5])
    gref, rest = row_tol.ln_bwd_ref64(g64, x, mean, rstd), row_tol.ln_bwd_rest(g64, x, mean, rstd, cg)
    assert not row_tol.judge("wan ln_mod dx", xg.grad, gref, rest if xdt == torch.float32 else row_tol.bf16_tol(gref, rest))


@pytest.mark.parametrize("rows,C", [(5, 264), (9, 3072), (6, 4096)])
def test_wan_ln_mod_fp32_result_forward_backward(rows, C):
    """the output head's form -- fp32 x, fp32 result, fp32 incoming gradient, modulation only -- through ln_mod(out_dtype=torch.float32): rows that do not
    fill the four waves of a workgroup with a partly filled first chunk, six full chunks, all eight chunks; against the fp64 expression, fp32 bound"""
    from videogpa_amd.wan_model import ln_mod
    g = torch.Generator(device="cuda").manual_seed(5)
    G = 2
    x = torch.randn(rows, C, device="cuda", generator=g) * 2 + 0.3
    gid = (torch.arange(rows, device="cuda") % G).int()
    tab = _tab(G, 2, C, g)
    dy = torch.randn(rows, C, device="cuda", generator=g)
    xg = x.clone().requires_grad_(True)
    out = ln_mod(xg, gid, None, None, tab[:, 0], tab[:, 1], 1e-6, out_dtype=torch.float32)
    out.backward(dy)
    xr = x.double().requires_grad_(True)
    h = torch.nn.functional.layer_norm(xr, (C,), None, None, 1e-6) * (1 + tab[:, 1].double()[gid.long()]) + tab[:, 0].double()[gid.long()]
    h.backward(dy.double())
    assert out.dtype == torch.float32 and xg.grad.dtype == torch.float32
    eo = (out.double() - h.detach()).abs().max().item() / h.detach().abs().max().item()
    eg = (xg.grad.double() - xr.grad).abs().max().item() / xr.grad.abs().max().item()
    print(f"ln_mod fp32 result {rows}x{C}: out {eo:.3g} grad {eg:.3g}")
    assert eo <= 1e-5 and eg <= 1e-5, (eo, eg)


def test_wan_ln_mod_entries_reject_combinations_no_kernel_is_built_for():
    """vgpa_wan_ln_mod_fwd / _bwd take the arguments of six former entries; a combination none of those accepted is VGPA_ERR_INVALID before any launch.
    Every buffer holds fp32 [rows, D + 64], so a call accepted by mistake would still be a valid launch."""
    from videogpa_amd import _lib
    lib = _lib.load()
    rows, D, F32, BF16 = 8, 256, 0, 1
    st = torch.cuda.current_stream().cuda_stream
    buf = lambda: torch.zeros(rows, D + 64, device="cuda")
    x, y, gate, xo, gid, w, b, sh, sc, out, q8, q8s, mean, rstd, dy, dres, dx, dyp = (buf() for _ in range(18))

    def fwd(x_dtype=F32, y=None, gate=None, x_out=None, ln_w=None, ln_b=None, round_xhat=0, out=out, out_dtype=BF16, q8=None, q8_scale=None):
        p = lambda t: None if t is None else t.data_ptr()
        return lib.vgpa_wan_ln_mod_fwd(p(x), x_dtype, p(y), p(gate), p(x_out), p(gid), p(ln_w), p(ln_b), p(sh), p(sc), D + 64, rows, D, 1e-6, round_xhat,
                                       p(out), out_dtype, D + 64, p(q8), p(q8_scale), p(mean), p(rstd), st)

    def bwd(dy_dtype=BF16, x_dtype=F32, ln_w=None, dres=None, gate_prev=None, dy_prev=None):
        p = lambda t: None if t is None else t.data_ptr()
        return lib.vgpa_wan_ln_mod_bwd(p(dy), dy_dtype, p(x), x_dtype, p(mean), p(rstd), p(gid), p(ln_w), p(sc), D + 64, rows, D, p(dres), p(dx), p(gate_prev),
                                       p(dy_prev), D + 64, st)

    assert fwd() == 0 and fwd(y=y, gate=gate, x_out=xo) == 0 and fwd(out_dtype=F32) == 0            # the three forms themselves are accepted
    assert bwd() == 0 and bwd(gate_prev=gate, dy_prev=dyp) == 0 and bwd(dy_dtype=F32) == 0
    rejected = {
        "y with bf16 x": fwd(x_dtype=BF16, y=y, x_out=xo),
        "y with round_xhat": fwd(y=y, x_out=xo, round_xhat=1),
        "gate without y": fwd(gate=gate),
        "x_out without y": fwd(x_out=xo),
        "y without x_out": fwd(y=y, gate=gate),
        "y with fp32 result": fwd(y=y, x_out=xo, out_dtype=F32),
        "fp32 result with bf16 x": fwd(x_dtype=BF16, out_dtype=F32),
        "fp32 result with q8": fwd(out_dtype=F32, q8=q8, q8_scale=q8s),
        "fp32 result with affine": fwd(out_dtype=F32, ln_w=w, ln_b=b),
        "fp32 result with round_xhat": fwd(out_dtype=F32, round_xhat=1),
        "fp32 result without out": fwd(out=None, out_dtype=F32, q8=q8, q8_scale=q8s),
        "unknown x dtype": fwd(x_dtype=2),
        "unknown out dtype": fwd(out_dtype=2),
        "dy_prev with bf16 x": bwd(x_dtype=BF16, dy_prev=dyp),
        "dy_prev with fp32 dy": bwd(dy_dtype=F32, dy_prev=dyp),
        "gate_prev without dy_prev": bwd(gate_prev=gate),
        "fp32 dy with bf16 x": bwd(dy_dtype=F32, x_dtype=BF16),
        "fp32 dy with ln_w": bwd(dy_dtype=F32, ln_w=w),
        "fp32 dy with dres": bwd(dy_dtype=F32, dres=dres),
        "unknown dy dtype": bwd(dy_dtype=2),
    }
    assert all(rc == -1 for rc in rejected.values()), rejected
    torch.cuda.synchronize()
    from videogpa_amd.wan_model import ln_mod
    with pytest.raises(ValueError, match="fp32 result"):          # the Python entry says so before any node is built
        ln_mod(x[:, :D].contiguous(), None, None, None, sh[0, :D], sc[0, :D], 1e-6, passthrough=True, out_dtype=torch.float32)


def test_wan_gate_residual_forward_backward():
    from videogpa_amd.wan_model import gate_residual
    g = torch.Generator(device="cuda").manual_seed(2)
    rows, C, G = 257, 3072, 2
    x = torch.randn(rows, C, device="cuda", generator=g)
    y = torch.randn(rows, C, device="cuda", generator=g).bfloat16()
    gid = torch.randint(0, G, (rows,), device="cuda", generator=g).int()
    tab = _tab(G, 6, C, g)
    dout = torch.randn(rows, C, device="cuda", generator=g)
    for gate in (tab[:, 2], None):
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        out = gate_residual(xg, yg, gid if gate is not None else None, gate)
        out.backward(dout)
        gt = gate[gid.long()] if gate is not None else torch.ones_like(x)
        assert out.dtype == torch.float32 and torch.equal(out, torch.addcmul(x, y.float(), gt)) or (out - (x + y.float() * gt)).abs().max().item() <= 1e-6 * 8
        assert torch.equal(xg.grad, dout)
        assert torch.equal(yg.grad, (dout * gt).bfloat16())


@pytest.mark.parametrize("rope", [True, False])
def test_wan_rms_rope_forward_backward(rope):
    from oracle import wan as ow
    from videogpa_amd.wan_model import rms_rope, rope_tables
    g = torch.Generator(device="cuda").manual_seed(3)
    B, grid, n, d = 2, (3, 4, 5), 24, 128
    L, C = grid[0] * grid[1] * grid[2], n * d
    u = (torch.randn(B, L, C, device="cuda", generator=g) * 1.7).bfloat16()
    w = (1 + 0.2 * torch.randn(C, device="cuda", generator=g)).bfloat16()
    dout = torch.randn(B, L, C, device="cuda", generator=g).bfloat16()
    cos, sin = rope_tables(grid, d, "cuda") if rope else (None, None)
    ug = u.clone().requires_grad_(True)
    out = rms_rope(ug, w, cos, sin, d, 1e-6)
    out.backward(dout)
    ur = u.double().requires_grad_(True)
    r = ow.rms_norm(ur, w.double(), 1e-6)
    if rope:
        freqs = torch.cat([ow.rope_params(1024, d - 4 * (d // 6), device="cuda"), ow.rope_params(1024, 2 * (d // 6), device="cuda"), ow.rope_params(1024, 2 * (d // 6), device="cuda")], dim=1)
        r = ow.rope_apply(r.view(B, L, n, d), grid, freqs).reshape(B, L, C)
    r.backward(dout.double())
    assert (out.double() - r.detach()).abs().max().item() <= 1.5 * 2 ** -8 * r.detach().abs().max().item()      # two bf16 roundings + the output's
    assert (ug.grad.double() - ur.grad).abs().max().item() <= 2.5 * 2 ** -8 * ur.grad.abs().max().item()
    # per element (tests/row_tol.py): each intermediate bf16 rounding's half ulp carried through |w|, |cos|, |sin|; rstd judged; the gradient from the device's rstd
    import row_tol
    from videogpa_amd import _lib
    u2, d2, st = u.view(B * L, C), dout.view(B * L, C), torch.cuda.current_stream().cuda_stream
    rs, o2 = torch.empty(B * L, device="cuda"), torch.empty_like(u2)
    _lib.call("vgpa_wan_rms_rope_fwd", u2, C, w, cos, sin, L, d, B * L, C, 1e-6, o2, C, rs, st)
    assert torch.equal(o2, out.detach().view(B * L, C))
    ref, rs_ref = row_tol.rms_rope_ref64(u2, w, cos, sin, L, d, 1e-6)
    tol, tol_rs = row_tol.rms_rope_fwd_tol(u2, w, cos, sin, L, d, 1e-6, ref)
    assert not row_tol.judge("rms_rope out", o2, ref, tol) and not row_tol.judge("rms_rope rstd", rs, rs_ref, tol_rs)
    gref = row_tol.rms_rope_bwd_ref64(d2, u2, rs, w, cos, sin, L, d)
    assert not row_tol.judge("rms_rope du", ug.grad.view(B * L, C), gref, row_tol.rms_rope_bwd_tol(d2, u2, rs, w, cos, sin, L, d, gref))


# ------------------------------------------------------------------------------------------------ fp8 operands (csrc/fp8.hip)
def test_quant_fp8_rows_bit_exact_vs_torch_cast():
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(8)
    for (M, K) in [(5, 64), (130, 3072), (33, 14336)]:
        x = (torch.randn(M, K, device="cuda", generator=g) * torch.rand(M, 1, device="cuda", generator=g) * 30).bfloat16()
        x[0] = 0                                                     # all-zero row: scale 1
        x[1, :8] = torch.tensor([1e-30, -1e-30, 448.0, -448.0, 1e4, -1e4, 0.0, 3.0], device="cuda").bfloat16()
        q, sc = ops.quant_fp8_rows(x)
        amax = x.float().abs().amax(dim=1, keepdim=True)
        ref_sc = torch.where(amax > 0, amax / torch.full_like(amax, 448.0), torch.ones_like(amax))   # tensor / tensor: a true division (tensor / python scalar multiplies by 1/448)
        ref_q = (x.float() / ref_sc).clamp(-448, 448).to(torch.float8_e4m3fn)
        assert torch.equal(sc, ref_sc)
        assert torch.equal(q.view(torch.uint8), ref_q.view(torch.uint8)), (M, K)
        xs = torch.cat([x, x], dim=1)[:, :K]                          # a column slice: row stride 2K
        q2, sc2 = ops.quant_fp8_rows(xs)
        assert torch.equal(q2.view(torch.uint8), q.view(torch.uint8)) and torch.equal(sc2, sc)


def test_frozen_linear_fp8_forward_backward_against_fp32():
    """e4m3 has 3 mantissa bits: each operand carries ~3.6 % rms rounding noise per element, which averages down over K in the product;
    the GEMM result must sit within 4 % (relative Frobenius error) of fp32 -- the figure tools/fp8_probe.py measures for hipBLASLt alone."""
    from videogpa_amd import ops
    g = torch.Generator(device="cuda").manual_seed(9)
    M, K, N = 512, 3072, 1024
    x = torch.randn(M, K, device="cuda", generator=g).bfloat16().requires_grad_(True)
    W = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).bfloat16()
    b = torch.randn(N, device="cuda", generator=g).bfloat16()
    dy = torch.randn(M, N, device="cuda", generator=g).bfloat16()
    y = ops.frozen_linear_fp8(x, W, b)
    y.backward(dy)
    ry = x.detach().float() @ W.float().T + b.float()
    rdx = dy.float() @ W.float()
    assert y.dtype == torch.bfloat16 and ((y.float() - ry).norm() / ry.norm()).item() < 0.04
    assert ((x.grad.float() - rdx).norm() / rdx.norm()).item() < 0.04


def _same_q8(q, sc, ref_q, ref_sc, what):
    """fused producers against the unfused chain: identical scales; identical bytes (the float expressions are the same source, but the compiler
    may contract them differently inside a different kernel, so a 1-ulp-of-bf16 difference before quantisation is tolerated on <= 0.1 % of the bytes)"""
    assert torch.equal(sc, ref_sc) or (sc - ref_sc).abs().max().item() <= 2 ** -7 * ref_sc.abs().max().item(), what
    a, b = q.view(torch.uint8), ref_q.view(torch.uint8)
    frac = (a != b).float().mean().item()
    assert frac <= 1e-3, (what, frac)
    assert (q.float() * sc - ref_q.float() * ref_sc).abs().max().item() <= 0.13 * (ref_q.float() * ref_sc).abs().max().item(), what


def test_fp8_operands_written_by_their_producers_match_the_unfused_chain():
    """vgpa_wan_ln_mod_fwd(q8), vgpa_gelu_tanh_{fwd,bwd}_q8, vgpa_wan_gate_bwd_q8  ==  bf16 producer + vgpa_quant_fp8_rows"""
    from videogpa_amd import _lib, ops
    from videogpa_amd.wan_model import ln_mod
    g = torch.Generator(device="cuda").manual_seed(21)
    st = torch.cuda.current_stream().cuda_stream
    rows, C, F, G = 203, 3072, 14336, 3
    x = torch.randn(rows, C, device="cuda", generator=g) * 2 + 0.3
    gid = torch.randint(0, G, (rows,), device="cuda", generator=g).int()
    tab = _tab(G, 6, C, g)
    # LN + modulation
    h = ln_mod(x, gid, None, None, tab[:, 3], tab[:, 4], 1e-6)
    rq, rs = ops.quant_fp8_rows(h)
    q = torch.empty(rows, C, dtype=torch.float8_e4m3fn, device="cuda"); sc = torch.empty(rows, 1, device="cuda")
    mean = torch.empty(rows, device="cuda"); rstd = torch.empty(rows, device="cuda")
    h2 = torch.empty(rows, C + 64, dtype=torch.bfloat16, device="cuda")
    _lib.call("vgpa_wan_ln_mod_fwd", x, 0, None, None, None, gid, None, None, tab[:, 3], tab[:, 4], tab.stride(0), rows, C, 1e-6, 0, h2, 1, C + 64, q, sc,
              mean, rstd, st)
    assert torch.equal(h2[:, :C], h)                                     # strided bf16 output next to the e4m3 one
    _same_q8(q, sc, rq, rs, "ln_mod")
    # GELU forward / backward
    u = (torch.randn(rows, F, device="cuda", generator=g) * 1.5).bfloat16()
    dy = torch.randn(rows, F, device="cuda", generator=g).bfloat16()
    ug = u.clone().requires_grad_(True)
    a = ops.gelu_tanh(ug)
    a.backward(dy)
    _same_q8(*ops.gelu_tanh_fwd_q8(u), *ops.quant_fp8_rows(a.detach()), "gelu fwd")
    _same_q8(*ops.gelu_tanh_bwd_q8(u, dy), *ops.quant_fp8_rows(ug.grad), "gelu bwd")
    # gate backward
    dout = torch.randn(rows, C, device="cuda", generator=g)
    ref = (dout * tab[:, 5][gid.long()]).bfloat16()
    _lib.call("vgpa_wan_gate_bwd_q8", dout, gid, tab[:, 5], tab.stride(0), rows, C, q, sc, st)
    _same_q8(q, sc, *ops.quant_fp8_rows(ref), "gate bwd")
    z = torch.zeros(4, C, device="cuda")
    _lib.call("vgpa_wan_gate_bwd_q8", z, None, None, 0, 4, C, q[:4], sc[:4], st)
    assert torch.equal(sc[:4], torch.ones(4, 1, device="cuda")) and not q[:4].view(torch.uint8).any()      # all-zero rows: scale 1


def test_wan_ffn_fp8_branch_equals_the_composed_ops():
    """_FfnFp8Fn (one autograd node, operands quantised by their producers, residual gradient added inside the LN backward) against the same
    branch composed from ln_mod / frozen_linear_fp8 / gelu_tanh / gate_residual: output and input gradient to fp32 rounding of the one add that moved."""
    from videogpa_amd import ops
    from videogpa_amd.wan_model import ffn_fp8, gate_residual, ln_mod
    g = torch.Generator(device="cuda").manual_seed(22)
    rows, C, F, G = 260, 1024, 2048, 2
    x = torch.randn(rows, C, device="cuda", generator=g)
    gid = torch.randint(0, G, (rows,), device="cuda", generator=g).int()
    tab = _tab(G, 6, C, g)
    W1 = (torch.randn(F, C, device="cuda", generator=g) / C ** 0.5).bfloat16(); b1 = (0.1 * torch.randn(F, device="cuda", generator=g)).bfloat16()
    W2 = (torch.randn(C, F, device="cuda", generator=g) / F ** 0.5).bfloat16(); b2 = (0.1 * torch.randn(C, device="cuda", generator=g)).bfloat16()
    dout = torch.randn(rows, C, device="cuda", generator=g)
    xa = x.clone().requires_grad_(True)
    ya = ffn_fp8(xa, gid, tab[:, 3], tab[:, 4], tab[:, 5], 1e-6, W1, b1, W2, b2)
    ya.backward(dout)
    xb = x.clone().requires_grad_(True)
    h = ln_mod(xb, gid, None, None, tab[:, 3], tab[:, 4], 1e-6)
    y = ops.frozen_linear_fp8(ops.gelu_tanh(ops.frozen_linear_fp8(h, W1, b1)), W2, b2)
    yb = gate_residual(xb, y, gid, tab[:, 5])
    yb.backward(dout)
    assert (ya - yb).abs().max().item() <= 2e-2 * yb.abs().max().item() and ((ya - yb).norm() / yb.norm()).item() <= 1e-3
    assert ((xa.grad - xb.grad).norm() / xb.grad.norm()).item() <= 1e-3


def test_wan_self_attention_core_on_the_fused_qkv_buffer():
    """_SelfAttnFn (q / k normalised from strided slices of the fused projection output, v read in place, gradients written into one padded
    [B, L, 3 D + pad] buffer) against rms_rope + attention128 on separate contiguous tensors: identical kernels, identical results"""
    from videogpa_amd import ops
    from videogpa_amd.wan_model import _SelfAttnFn, rms_rope, rope_tables
    g = torch.Generator(device="cuda").manual_seed(23)
    B, grid, H, d = 2, (3, 6, 8), 2, 128
    L, D = grid[0] * grid[1] * grid[2], H * d
    qkv = (torch.randn(B, L, 3 * D, device="cuda", generator=g) * 1.3).bfloat16()
    wq = (1 + 0.2 * torch.randn(D, device="cuda", generator=g)).bfloat16(); wk = (1 + 0.2 * torch.randn(D, device="cuda", generator=g)).bfloat16()
    do = torch.randn(B, L, D, device="cuda", generator=g).bfloat16()
    cos, sin = rope_tables(grid, d, "cuda")
    a = qkv.clone().requires_grad_(True)
    oa = _SelfAttnFn.apply(a, wq, wk, cos, sin, H, 1e-6, 16, 48, False, "int8")      # the same "Precise delta" mode as attention128's default below
    assert ops._padded_base(oa.reshape(B * L, D), D + 16) is not None
    oa.backward(do)
    assert ops._padded_base(a.grad.reshape(B * L, 3 * D), 3 * D + 48) is not None or a.grad.shape == (B, L, 3 * D)
    b = qkv.clone().requires_grad_(True)
    q, k, v = b[:, :, :D].contiguous(), b[:, :, D:2 * D].contiguous(), b[:, :, 2 * D:].contiguous()
    hd = lambda t: t.view(B, L, H, d).permute(0, 2, 1, 3)
    ob = ops.attention128(hd(rms_rope(q, wq, cos, sin, d, 1e-6)), hd(rms_rope(k, wk, cos, sin, d, 1e-6)), hd(v)).permute(0, 2, 1, 3).reshape(B, L, D)
    ob.backward(do)
    assert torch.equal(oa, ob)
    assert torch.equal(a.grad, b.grad)


def test_wan_ln_mod_passthrough_adds_the_residual_gradient_in_the_kernel():
    """h, xp = ln_mod(x, passthrough=True); loss through both outputs: dx = LN-backward(dh) + dxp, equal to autograd's own sum of the two paths"""
    from videogpa_amd.wan_model import ln_mod
    g = torch.Generator(device="cuda").manual_seed(31)
    rows, C, G = 130, 3072, 2
    x = torch.randn(rows, C, device="cuda", generator=g)
    gid = torch.randint(0, G, (rows,), device="cuda", generator=g).int()
    tab = _tab(G, 6, C, g)
    dh = torch.randn(rows, C, device="cuda", generator=g).bfloat16()
    dxp = torch.randn(rows, C, device="cuda", generator=g)
    a = x.clone().requires_grad_(True)
    h, xp = ln_mod(a, gid, None, None, tab[:, 3], tab[:, 4], 1e-6, passthrough=True)
    torch.autograd.backward([h, xp], [dh, dxp])
    b = x.clone().requires_grad_(True)
    h2 = ln_mod(b, gid, None, None, tab[:, 3], tab[:, 4], 1e-6)
    torch.autograd.backward([h2, b * 1.0], [dh, dxp])
    assert torch.equal(h, h2) and torch.equal(xp, x)
    # the same two fp32 terms added once inside the kernel (contracted into an fma) and once by autograd: one rounding apart
    assert (a.grad - b.grad).abs().max().item() <= 1e-6 * b.grad.abs().max().item()
    c = x.clone().requires_grad_(True)
    h3, xp3 = ln_mod(c, gid, None, None, tab[:, 3], tab[:, 4], 1e-6, passthrough=True)
    xp3.backward(dxp)                                        # LN output unused: the residual gradient passes through
    assert torch.equal(c.grad, dxp)


@pytest.mark.parametrize("mode", ["gate+affine", "plain+mod"])
def test_wan_gate_ln_is_bit_identical_to_gate_residual_then_ln_mod(mode):
    """gate_ln (csrc/wan.hip GR / GB forms: a block's [gated residual add -> LayerNorm] pair in one pass each way) against the two-node chain it replaces,
    in both shapes the block uses: self-attention branch (per-token gate, affine norm3, LoRA tails on both sides) and cross-attention branch (no gate, the
    feed-forward's modulated LayerNorm).  Forward outputs bit-identical; dx and dy bit-identical to the chain (the same kernel arithmetic), also when only
    the residual output carries a gradient."""
    from videogpa_amd.wan_model import gate_ln, gate_residual, ln_mod
    g = torch.Generator(device="cuda").manual_seed(41)
    rows, C, G = 133, 3072, 2
    x = torch.randn(rows, C, device="cuda", generator=g)
    y = torch.randn(rows, C, device="cuda", generator=g).bfloat16()
    gid = torch.randint(0, G, (rows,), device="cuda", generator=g).int()
    tab = _tab(G, 6, C, g)
    w, b = 1 + 0.1 * torch.randn(C, device="cuda", generator=g), 0.1 * torch.randn(C, device="cuda", generator=g)
    dh = torch.randn(rows, C, device="cuda", generator=g).bfloat16()
    dxp = torch.randn(rows, C, device="cuda", generator=g)
    if mode == "gate+affine":
        kw = dict(gid=gid, gate=tab[:, 2], ln_w=w, ln_b=b, shift=None, scale=None, pad=64, dy_pad=64)
    else:
        kw = dict(gid=gid, gate=None, ln_w=None, ln_b=None, shift=tab[:, 3], scale=tab[:, 4], pad=0, dy_pad=64)

    def chain(xa, ya):
        xs = gate_residual(xa, ya, kw["gid"] if kw["gate"] is not None else None, kw["gate"], dy_pad=kw["dy_pad"])
        return ln_mod(xs, kw["gid"] if kw["shift"] is not None else None, kw["ln_w"], kw["ln_b"], kw["shift"], kw["scale"], 1e-6, pad=kw["pad"], passthrough=True)

    xa, ya = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    h, xp = gate_ln(xa, ya, eps=1e-6, **kw)
    xb, yb = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    h2, xp2 = chain(xb, yb)
    assert torch.equal(h, h2) and torch.equal(xp, xp2)
    assert h.stride(0) == C + kw["pad"]
    torch.autograd.backward([h, xp], [dh, dxp])
    torch.autograd.backward([h2, xp2], [dh, dxp])
    # dx: the same fp32 expression compiled in two kernel instantiations (fma contraction may differ): one rounding apart at most; dy = bf16(dx * gate)
    assert (xa.grad - xb.grad).abs().max().item() <= 1e-6 * xb.grad.abs().max().item()
    assert ((ya.grad.float() - yb.grad.float()).abs() <= 2.0 ** -7 * yb.grad.float().abs() + 1e-30).all() and (ya.grad != yb.grad).float().mean().item() < 1e-3
    xc, yc = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    _, xp3 = gate_ln(xc, yc, eps=1e-6, **kw)
    xp3.backward(dxp)                                        # LN output unused
    xd, yd = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    gate_residual(xd, yd, kw["gid"] if kw["gate"] is not None else None, kw["gate"], dy_pad=kw["dy_pad"]).backward(dxp)
    assert torch.equal(xc.grad, xd.grad) and torch.equal(yc.grad, yd.grad)
