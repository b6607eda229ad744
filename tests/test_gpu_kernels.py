"""HIP kernels (through the C-ABI) vs the CPU oracle on the same seeded inputs.  -m gpu only."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import attn_tol
import lora_tol
import row_tol
from attn_ref64 import attn_ref64
from attn_tol import lse2_tol
from oracle import cogvideox as ocv
from oracle import dpo as odpo
from oracle import scheduler as osch


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops as _ops
    return _ops


def dev(t):
    return t.cuda()


# ------------------------------------------------------------------------------------------ DPO loss
def test_dpo_loss_golden(ops, golden_dir):
    """fp32 inputs from the reference goldens (train/loss.py outputs).  Tolerance: 2e-6 rel on the scalars
    (fp64 tree reduction here vs torch fp32 reduction there), grads 1e-5 rel of max."""
    cases = torch.load(os.path.join(golden_dir, "dpo_loss.pt"), weights_only=False)
    for c in cases:
        ins = [dev(x).requires_grad_(i < 2) for i, x in enumerate(c["inputs"])]
        loss, margin, wr, lr, acc, errs = ops.dpo_loss(*ins, beta=c["beta"], label_smoothing=c["label_smoothing"], loss_type=c["loss_type"])
        # logits are beta * (difference of O(1) fp32 means): absolute error scales with beta * eps_fp32
        tol = 5e-6 * max(1.0, c["beta"])
        assert abs(loss.item() - c["loss"].item()) <= tol * max(1.0, abs(c["loss"].item())), (c["beta"], c["loss_type"], loss.item(), c["loss"].item())
        assert abs(margin.item() - c["reward_margin"].item()) < 2e-6
        assert abs(wr.item() - c["winner_reward"].item()) < 5e-6 * abs(c["winner_reward"].item())
        assert abs(lr.item() - c["loser_reward"].item()) < 5e-6 * abs(c["loser_reward"].item())
        assert acc.item() == c["accuracy"].item()
        if c["grad_v_win"] is not None:
            loss.backward()
            for g, ref in ((ins[0].grad, c["grad_v_win"]), (ins[1].grad, c["grad_v_lose"])):
                ref = ref.cuda()
                scale = ref.abs().max().item() + 1e-30
                assert (g - ref).abs().max().item() <= max(1e-5, 50 * tol) * scale


def test_dpo_loss_ln2_and_bf16(ops):
    g = torch.Generator().manual_seed(5)
    shape = (2, 13, 16, 12, 18)
    v = [torch.randn(shape, generator=g).to(torch.bfloat16) for _ in range(4)]
    out = ops.dpo_loss(dev(v[0]), dev(v[1]), dev(v[0]).clone(), dev(v[1]).clone(), dev(v[2]), dev(v[3]), beta=500.0)
    assert abs(out[0].item() - math.log(2.0)) < 1e-6
    # bf16 inputs vs oracle on the same (bf16-rounded) values in fp64
    t = [torch.randn(shape, generator=g).to(torch.bfloat16) for _ in range(6)]
    ins = [dev(x).requires_grad_(i < 2) for i, x in enumerate(t)]
    out = ops.dpo_loss(*ins, beta=3.0)
    ref_in = [x.double().requires_grad_(i < 2) for i, x in enumerate(t)]
    ref = odpo.dpo_loss(*ref_in, beta=3.0)
    assert abs(out[0].item() - ref["loss"].item()) < 1e-5
    out[0].backward()
    ref["loss"].backward()
    for a, b in ((ins[0].grad, ref_in[0].grad), (ins[1].grad, ref_in[1].grad)):
        assert a.dtype == torch.bfloat16
        sc = b.abs().max().item()
        assert (a.double().cpu() - b).abs().max().item() < 1e-2 * sc  # bf16 output rounding (2^-8 rel)


# ------------------------------------------------------------------------------------------ noise / velocity
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_noise_velocity_bit_exact(ops, dtype):
    g = torch.Generator().manual_seed(11)
    B, shape = 3, (5, 16, 6, 10)
    x = (torch.randn(B, 2, *shape, generator=g) * 0.7).to(dtype)
    eps = torch.randn(B, *shape, generator=g).to(dtype)
    t = torch.tensor([0, 417, 999])
    abar = osch.alphas_cumprod()
    a = abar.to(dtype)[t]           # diffusers casts the table to the sample dtype first
    sa, sb = a ** 0.5, (1 - a) ** 0.5
    sa_tab = torch.zeros(1000, dtype=torch.float32)
    sb_tab = torch.zeros(1000, dtype=torch.float32)
    ad = abar.to(dtype)
    sa_tab[:] = (ad ** 0.5).float()
    sb_tab[:] = ((1 - ad) ** 0.5).float()
    xt, v = ops.noise_velocity_paired(dev(x), dev(eps), dev(t), dev(sa_tab), dev(sb_tab))
    bc = (B, 1, 1, 1, 1)
    for p in range(2):
        ref_xt = sa.view(bc) * x[:, p] + sb.view(bc) * eps
        ref_v = sa.view(bc) * eps - sb.view(bc) * x[:, p]
        assert torch.equal(xt[:, p].cpu(), ref_xt)
        assert torch.equal(v[:, p].cpu(), ref_v)


# ------------------------------------------------------------------------------------------ AdaLN pieces
@pytest.mark.parametrize("impl", ["fused", "v1"])
@pytest.mark.parametrize("D,text_len", [(128, 6), (3072, 5), (512, 0)])
def test_ln_modulate_fwd_bwd(ops, D, text_len, impl):
    g = torch.Generator().manual_seed(D)
    B, S = 2, 37
    x = torch.randn(B, S, D, generator=g).to(torch.bfloat16)
    w = 1 + 0.1 * torch.randn(D, generator=g)
    b = 0.1 * torch.randn(D, generator=g)
    mod = 0.3 * torch.randn(B, 4, D, generator=g)
    mod[:, 1] += 1
    mod[:, 3] += 1
    dy = torch.randn(B, S, D, generator=g).to(torch.bfloat16)
    lnm = ops.ln_modulate if impl == "fused" else ops.ln_modulate_v1
    xd = dev(x).requires_grad_(True)
    y = lnm(xd, dev(w), dev(b), dev(mod), text_len, 1e-5)
    y.backward(dev(dy))
    xr = x.double().requires_grad_(True)
    n = F.layer_norm(xr, (D,), w.double(), b.double(), 1e-5)
    sc = torch.cat([mod[:, 3:4].expand(B, text_len, D), mod[:, 1:2].expand(B, S - text_len, D)], 1).double()
    sh = torch.cat([mod[:, 2:3].expand(B, text_len, D), mod[:, 0:1].expand(B, S - text_len, D)], 1).double()
    yr = n * sc + sh
    yr.backward(dy.double())
    assert (y.double().cpu() - yr).abs().max().item() < 0.03          # bf16 output rounding of O(4) values
    assert (y.double().cpu() - yr.detach().to(torch.bfloat16).double()).abs().max().item() <= 0.032
    gerr = (xd.grad.double().cpu() - xr.grad).abs().max().item()
    assert gerr < 0.02 * xr.grad.abs().max().item() + 1e-3
    # plain LN (no modulation)
    y2 = lnm(dev(x), dev(w), dev(b), None, 0, 1e-5)
    assert (y2.double().cpu() - n.detach()).abs().max().item() < 0.03
    # per element (tests/row_tol.py): the bf16 half ulp of each result plus the counted fp32 error; mean and rstd are judged too, and the gradient is held to the
    # expression evaluated from them.  The C entry behind `lnm` is called once more for them: the same kernel on the same input writes the same bits
    from videogpa_amd import _lib
    md, st = dev(mod), torch.cuda.current_stream().cuda_stream
    mean, rstd, n2 = torch.empty(B, S, device="cuda"), torch.empty(B, S, device="cuda"), torch.empty_like(y)
    if impl == "fused":
        _lib.call("vgpa_residual_ln_fwd", xd.detach(), None, None, None, 0, dev(w), dev(b), md[:, 0], md[:, 1], md[:, 2], md[:, 3], md.stride(0), B, S, D, text_len, 1e-5,
                  None, n2, D, mean, rstd, st)
    else:
        _lib.call("vgpa_ln_modulate_fwd", xd.detach(), dev(w), dev(b), md[:, 0], md[:, 1], md[:, 2], md[:, 3], md.stride(0), B, S, D, text_len, 1e-5, n2, mean, rstd, st)
    assert torch.equal(n2, y.detach())
    s1p, shf = row_tol.cog_rows(mod[:, 1], mod[:, 3], B, S, text_len), row_tol.cog_rows(mod[:, 0], mod[:, 2], B, S, text_len)
    ref = row_tol.cog_ln_fwd_ref64(x, w, b, s1p, shf, 1e-5)
    tols = row_tol.cog_ln_fwd_tol(x, w, b, s1p, shf, 1e-5, ref[0])
    for name, got, r, t in zip(("n", "mean", "rstd"), (y.detach().cpu(), mean.cpu(), rstd.cpu()), ref, tols):
        assert not row_tol.judge(f"ln_modulate {name}", got, r, t)
    gg = dy.double() * w.double() * s1p.double()
    gref = row_tol.ln_bwd_ref64(gg, x, mean.cpu(), rstd.cpu())
    assert not row_tol.judge("ln_modulate dx", xd.grad.cpu(), gref, row_tol.bf16_tol(gref, row_tol.ln_bwd_rest(gg, x, mean.cpu(), rstd.cpu(), 2.0)))
    pref = row_tol.cog_ln_fwd_ref64(x, w, b, None, None, 1e-5)
    assert not row_tol.judge("plain LN", y2.cpu(), pref[0], row_tol.cog_ln_fwd_tol(x, w, b, None, None, 1e-5, pref[0])[0])


def test_gate_residual_and_gelu(ops):
    g = torch.Generator().manual_seed(3)
    B, S, D, Lt = 2, 19, 256, 4
    x = torch.randn(B, S, D, generator=g).to(torch.bfloat16)
    y = torch.randn(B, S, D, generator=g).to(torch.bfloat16)
    gates = torch.randn(B, 2, D, generator=g).to(torch.bfloat16).float()
    xd, yd = dev(x).requires_grad_(True), dev(y).requires_grad_(True)
    out = ops.gate_residual(xd, yd, dev(gates), Lt)
    gfull = torch.cat([gates[:, 1:2].expand(B, Lt, D), gates[:, 0:1].expand(B, S - Lt, D)], 1).to(torch.bfloat16)
    ref = x + gfull * y                      # torch bf16 semantics: round(g*y) then round(x + .)
    assert torch.equal(out.cpu(), ref)
    dout = torch.randn(B, S, D, generator=g).to(torch.bfloat16)
    out.backward(dev(dout))
    assert torch.equal(xd.grad.cpu(), dout)
    assert torch.equal(yd.grad.cpu(), gfull * dout)

    u = (3 * torch.randn(4, 33, 64, generator=g)).to(torch.bfloat16)
    ud = dev(u).requires_grad_(True)
    o = ops.gelu_tanh(ud)
    ur = u.double().requires_grad_(True)
    orf = F.gelu(ur, approximate="tanh")
    assert (o.double().cpu() - orf).abs().max().item() < 0.04
    do = torch.randn(4, 33, 64, generator=g).to(torch.bfloat16)
    o.backward(dev(do))
    orf.backward(do.double())
    assert (ud.grad.double().cpu() - ur.grad).abs().max().item() < 0.03
    # per element: the bf16 half ulp of each result plus the counted fp32 error (tests/row_tol.py), where 0.04 absolute said nothing about the small outputs
    val, der = row_tol.gelu_ref64(u, do)
    assert not row_tol.judge("gelu", o.detach().cpu(), val, row_tol.gelu_fwd_tol(u, val))
    assert not row_tol.judge("dgelu", ud.grad.cpu(), der, row_tol.gelu_bwd_tol(u, do, der))


# ------------------------------------------------------------------------------------------ attention
def _attn_ref(q, k, v, do=None):
    """fp64 softmax(QK^T/8)V on bf16-valued inputs [B,H,S,64]."""
    q, k, v = (t.double().requires_grad_(do is not None) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) / 8.0
    o = torch.softmax(s, -1) @ v
    if do is None:
        return o
    o.backward(do.double())
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("B,H,S", [(1, 2, 64), (1, 1, 128), (2, 3, 200), (1, 2, 333), (1, 1, 1000)])
def test_attention_fwd_bwd_raw(ops, B, H, S):
    g = torch.Generator().manual_seed(S)
    q, k, v, do = (torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16) for _ in range(4))
    q = q * 1.5   # sharper softmax
    qd, kd, vd = dev(q), dev(k), dev(v)
    o, lse = ops.attention_fwd_raw(qd, kd, vd)
    o_ref, dq_ref, dk_ref, dv_ref = _attn_ref(q, k, v, do)
    o_bhsd = o.view(B, S, H, 64).permute(0, 2, 1, 3).double().cpu()
    err = (o_bhsd - o_ref).abs().max().item()
    assert err < 0.02, f"attention fwd max err {err}"
    s = (q.double() @ k.double().transpose(-1, -2)) / 8.0
    lse_ref = torch.logsumexp(s, -1) / math.log(2.0)
    # raw API: q is re-rounded to bf16 after the scale*log2(e) pre-multiply (the fused path folds it into QK-norm)
    assert (lse.double().cpu() - lse_ref).abs().max().item() < 1.5e-2
    dq, dk, dv = (torch.empty(B, H, S, 64, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    ov = o.view(B, S, H, 64).permute(0, 2, 1, 3)
    ops.attention_bwd_raw(qd, kd, vd, ov, dev(do), lse, dq, dk, dv)
    for name, a, r in (("dq", dq, dq_ref), ("dk", dk, dk_ref), ("dv", dv, dv_ref)):
        e = (a.double().cpu() - r).abs().max().item()
        assert e < 0.03 * r.abs().max().item() + 2e-3, f"{name} max err {e} (ref max {r.abs().max().item()})"
    # per element, inside the derived bounds of tests/attn_tol.py (w1 forward: row sum of the rounded weights; no residual handed over: the textbook delta)
    problems, dod = [], dev(do)
    for b in range(B):
        for h in range(H):
            qs = (qd[b, h].float() * (64 ** -0.5 * attn_tol.LOG2E)).to(torch.bfloat16)          # the kernels' contract: one bf16 rounding of q * scale * log2 e
            R = attn_ref64(qs, kd[b, h], vd[b, h], dod[b, h], smul=1.0, dq_mul=64 ** -0.5, dk_mul=attn_tol.LN2, rounded_rowsum=True)
            problems += attn_tol.judge({"o": ov[b, h], "lse2": lse[b, h], "dq": dq[b, h], "dk": dk[b, h], "dv": dv[b, h]}, R, delta=None, where=f"[S {S} b{b} h{h}]")[0]
    assert not problems, "\n".join(problems)


def test_attention_online_softmax_rescale(ops):
    """Force a late, large running-max jump (a spiked key in the last tile) -- guide rule 26."""
    g = torch.Generator().manual_seed(77)
    B, H, S = 1, 1, 256
    q, k, v = (torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16) for _ in range(3))
    k[0, 0, 250] = (q[0, 0, 17].float() * 4).to(torch.bfloat16)
    o, _ = ops.attention_fwd_raw(dev(q), dev(k), dev(v))
    o_ref = _attn_ref(q, k, v)
    err = (o.view(B, S, H, 64).permute(0, 2, 1, 3).double().cpu() - o_ref).abs().max().item()
    assert err < 0.03, err


@pytest.mark.parametrize("use_rope", [False, True])
def test_qknorm_attention_fused(ops, use_rope):
    g = torch.Generator().manual_seed(9)
    B, H, Lt, Fr, gh, gw = 2, 2, 6, 2, 4, 5
    Sv = Fr * gh * gw
    S = Lt + Sv
    qkv = torch.randn(B, S, 3 * H * 64, generator=g).to(torch.bfloat16)
    wq, wk = (1 + 0.2 * torch.randn(64, generator=g) for _ in range(2))
    bq, bk = (0.2 * torch.randn(64, generator=g) for _ in range(2))
    rope = ocv.rope_3d_tables(Fr, gh, gw, 64) if use_rope else None
    do = torch.randn(B, S, H * 64, generator=g).to(torch.bfloat16)
    qd = dev(qkv).requires_grad_(True)
    o = ops.qknorm_attention(qd, dev(wq), dev(bq), dev(wk), dev(bk), H, Lt, None if rope is None else (dev(rope[0]), dev(rope[1])))
    o.backward(dev(do))

    x = qkv.double().requires_grad_(True)
    q, k, v = (x.view(B, S, 3, H, 64)[:, :, i].transpose(1, 2) for i in range(3))
    q = F.layer_norm(q, (64,), wq.double(), bq.double(), 1e-6)
    k = F.layer_norm(k, (64,), wk.double(), bk.double(), 1e-6)
    if use_rope:
        cos, sin = rope[0].double(), rope[1].double()

        def rot(t):
            tr, ti = t.reshape(*t.shape[:-1], -1, 2).unbind(-1)
            t_rot = torch.stack([-ti, tr], dim=-1).flatten(3)
            return t * cos + t_rot * sin
        q = torch.cat([q[:, :, :Lt], rot(q[:, :, Lt:])], 2)
        k = torch.cat([k[:, :, :Lt], rot(k[:, :, Lt:])], 2)
    orf = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, S, H * 64)
    orf.backward(do.double())
    assert (o.double().cpu() - orf).abs().max().item() < 0.03
    e = (qd.grad.double().cpu() - x.grad).abs().max().item()
    assert e < 0.03 * x.grad.abs().max().item() + 2e-3, e


# ------------------------------------------------------------------------------------------ LoRA MFMA kernels
@pytest.mark.parametrize("M,K,r,n", [(200, 128, 4, 3), (333, 256, 64, 3), (1000, 3072, 64, 1), (130, 192, 8, 1)])
def test_lora_kernels_raw(ops, M, K, r, n):
    g = torch.Generator().manual_seed(M + r)
    rp = ops._pad_rank(r)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    a_cat = torch.zeros(n * rp, K)
    for j in range(n):
        a_cat[j * rp:j * rp + r] = torch.randn(r, K, generator=g) / K ** 0.5
    a_cat = a_cat.to(torch.bfloat16)
    t = ops.lora_down(dev(x), dev(a_cat))
    t_ref = x.double() @ a_cat.double().t()
    assert (t.double().cpu() - t_ref).abs().max().item() < 0.02 * t_ref.abs().max().item() + 1e-3
    assert not lora_tol.judge("down", t.cpu(), t_ref, lora_tol.down_tol(t_ref, x.double().abs() @ a_cat.double().abs().t(), K))     # per element: tests/lora_tol.py
    # up_add into a column slice of a wider buffer
    N = 96
    y = torch.randn(M, n * N, generator=g).to(torch.bfloat16)
    yd = dev(y).clone()
    for j in range(n):
        bw = torch.zeros(N, rp)
        bw[:, :r] = torch.randn(N, r, generator=g)
        bw = bw.to(torch.bfloat16)
        ops.lora_up_add(yd[:, j * N:(j + 1) * N], t[:, j * rp:(j + 1) * rp], dev(bw), 2.0)
        ref = y[:, j * N:(j + 1) * N].double() + 2.0 * (t[:, j * rp:(j + 1) * rp].double().cpu() @ bw.double().t())
        err = (yd[:, j * N:(j + 1) * N].double().cpu() - ref).abs().max().item()
        assert err < 0.02 * ref.abs().max().item() + 1e-3, err
        ref_j, dot, S = lora_tol.up_ref64(y[:, j * N:(j + 1) * N], t[:, j * rp:(j + 1) * rp].cpu(), bw, 2.0)
        assert not lora_tol.judge(f"up_add {j}", yd[:, j * N:(j + 1) * N].cpu(), ref_j, lora_tol.up_tol(ref_j, dot, S, 2.0, rp, True))
    # grad: fp32 U^T V over tokens
    u = torch.randn(M, n * rp, generator=g).to(torch.bfloat16)
    gr = ops.lora_grad(dev(u), dev(x), 0.5)
    ref = 0.5 * (u.double().t() @ x.double())
    assert gr.dtype == torch.float32 and tuple(gr.shape) == (n * rp, K)
    assert (gr.double().cpu() - ref).abs().max().item() < 2e-3 * ref.abs().max().item() + 1e-4
    assert not lora_tol.judge("grad", gr.cpu(), ref, lora_tol.grad_tol(ref, lora_tol.grad_ref64(u, x, 0.5)[1], 0.5, M))
    gr2 = ops.lora_grad(dev(x)[:, :64], dev(u), 1.0)          # strided U (column slice)
    ref2 = x[:, :64].double().t() @ u.double()
    assert (gr2.double().cpu() - ref2).abs().max().item() < 2e-3 * ref2.abs().max().item() + 1e-4
    assert not lora_tol.judge("grad, U a column slice", gr2.cpu(), ref2, lora_tol.grad_tol(ref2, lora_tol.grad_ref64(x[:, :64], u, 1.0)[1], 1.0, M))


def test_lora_grad_is_bit_reproducible_at_the_headline_shape(ops):
    """The token-contracted adapter gradients (dB = s dy^T T, dA = dT^T x at M = 2 x 17 776 rows) go through per-row-range partials and
    an ordered merge (vgpa_lora_grad_ws): repeated launches must agree bit for bit (the atomics form did not), and with fp64."""
    g = torch.Generator(device="cuda").manual_seed(9)
    M = 2 * 17776
    dy = torch.randn(M, 3072, generator=g, device="cuda").to(torch.bfloat16)
    t = torch.randn(M, 192, generator=g, device="cuda").to(torch.bfloat16)
    a = [ops.lora_grad(dy, t[:, 64:128], 2.0) for _ in range(3)]
    b = [ops.lora_grad(t, dy) for _ in range(3)]
    assert all(torch.equal(a[0], x) for x in a[1:]) and all(torch.equal(b[0], x) for x in b[1:])
    ref = 2.0 * (dy[:, :256].double().t() @ t[:, 64:128].double())
    assert (a[0][:256].double() - ref).abs().max().item() < 1e-3 * ref.abs().max().item()
    for name, got, (ref, S), sc in (("dB", a[0], lora_tol.grad_ref64(dy, t[:, 64:128], 2.0), 2.0), ("dA", b[0], lora_tol.grad_ref64(t, dy, 1.0), 1.0)):
        assert not lora_tol.judge(name, got, ref, lora_tol.grad_tol(ref, S, sc, M))          # every element, fp64 on the device


def test_linear_lora_function_vs_torch(ops):
    g = torch.Generator().manual_seed(5)
    Bt, S, K, Dn, r = 2, 77, 128, 128, 8
    x = torch.randn(Bt, S, K, generator=g).to(torch.bfloat16)
    W = (torch.randn(3 * Dn, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(3 * Dn, generator=g).to(torch.bfloat16)
    As = [torch.randn(r, K, generator=g) / K ** 0.5 for _ in range(3)]
    Bs = [torch.randn(Dn, r, generator=g) * 0.3 for _ in range(3)]
    dy = torch.randn(Bt, S, 3 * Dn, generator=g).to(torch.bfloat16)
    xd = dev(x).requires_grad_(True)
    Ad = [dev(a).requires_grad_(True) for a in As]
    Bd = [dev(b_).requires_grad_(True) for b_ in Bs]
    loras = [(Ad[0], Bd[0], 2.0), None, (Ad[2], Bd[2], 2.0)]
    y = ops.linear_lora(xd, dev(W), dev(b), loras)
    y.backward(dev(dy))
    xr = x.double().requires_grad_(True)
    Ar = [a.to(torch.bfloat16).double().requires_grad_(True) for a in As]
    Br = [b_.to(torch.bfloat16).double().requires_grad_(True) for b_ in Bs]
    yr = F.linear(xr, W.double(), b.double())
    parts = list(yr.split(Dn, dim=-1))
    for i in (0, 2):
        parts[i] = parts[i] + 2.0 * F.linear(F.linear(xr, Ar[i]), Br[i])
    yr = torch.cat(parts, -1)
    yr.backward(dy.double())
    assert (y.double().cpu() - yr).abs().max().item() < 0.03 * yr.abs().max().item()
    assert (xd.grad.double().cpu() - xr.grad).abs().max().item() < 0.03 * xr.grad.abs().max().item()
    for i in (0, 2):
        assert Ad[i].grad.dtype == torch.float32
        assert (Ad[i].grad.double().cpu() - Ar[i].grad).abs().max().item() < 0.03 * Ar[i].grad.abs().max().item()
        assert (Bd[i].grad.double().cpu() - Br[i].grad).abs().max().item() < 0.03 * Br[i].grad.abs().max().item()
    assert Ad[1].grad is None and Bd[1].grad is None
    # dA, dB per element against fp64 of the device's OWN bf16 intermediates (T = lora_down(x, bf16(A)), dT = lora_down(dy_i, bf16(float(bf16(B)) s)^T)): the adapter-gradient
    # kernel alone, without the vendor GEMM's rounding or the 3 % of the maximum above
    rp, M = ops._pad_rank(r), Bt * S
    x2, dy2 = dev(x).reshape(M, K), dev(dy).reshape(M, 3 * Dn)
    for i in (0, 2):
        a_pad, sbt = torch.zeros(rp, K, dtype=torch.bfloat16, device="cuda"), torch.zeros(rp, Dn, dtype=torch.bfloat16, device="cuda")
        a_pad[:r] = Ad[i].detach().to(torch.bfloat16)
        sbt[:r] = (Bd[i].detach().to(torch.bfloat16).float() * 2.0).to(torch.bfloat16).t()
        T, dT = ops.lora_down(x2, a_pad)[:, :r], ops.lora_down(dy2[:, i * Dn:(i + 1) * Dn], sbt)[:, :r]
        ref, Sm = lora_tol.grad_ref64(dy2[:, i * Dn:(i + 1) * Dn], T, 2.0)
        assert not lora_tol.judge(f"dB[{i}]", Bd[i].grad, ref, lora_tol.grad_tol(ref, Sm, 2.0, M))
        ref, Sm = lora_tol.grad_ref64(dT, x2, 1.0)
        assert not lora_tol.judge(f"dA[{i}]", Ad[i].grad, ref, lora_tol.grad_tol(ref, Sm, 1.0, M))


# ------------------------------------------------------------------------------------------ edge cases / error codes
@pytest.mark.parametrize("S", [1, 7, 63, 64, 65, 129])
def test_attention_tiny_and_boundary_lengths(ops, S):
    g = torch.Generator().manual_seed(S)
    B, H = 2, 1
    q, k, v, do = (torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16) for _ in range(4))
    o, lse = ops.attention_fwd_raw(dev(q), dev(k), dev(v))
    o_ref, dq_ref, dk_ref, dv_ref = _attn_ref(q, k, v, do)
    assert (o.view(B, S, H, 64).permute(0, 2, 1, 3).double().cpu() - o_ref).abs().max().item() < 0.02
    dq, dk, dv = (torch.empty(B, H, S, 64, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    ops.attention_bwd_raw(dev(q), dev(k), dev(v), o.view(B, S, H, 64).permute(0, 2, 1, 3), dev(do), lse, dq, dk, dv)
    for a, r in ((dq, dq_ref), (dk, dk_ref), (dv, dv_ref)):
        assert (a.double().cpu() - r).abs().max().item() < 0.03 * r.abs().max().item() + 2e-3
    assert torch.isfinite(o).all() and torch.isfinite(dq).all() and torch.isfinite(dk).all() and torch.isfinite(dv).all()


def test_attention_outlier_scores_late_rescale_many_tiles(ops):
    """Spikes far above the running max in several late tiles, in both half-lanes, must go through the slow path."""
    g = torch.Generator().manual_seed(4)
    B, H, S = 1, 1, 1000
    q, k, v = (torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16) for _ in range(3))
    for key, row, gain in ((300, 5, 3.0), (700, 40, 6.0), (905, 5, 9.0), (999, 77, 12.0)):
        k[0, 0, key] = (q[0, 0, row].float() * gain / 8).to(torch.bfloat16)
    o, lse = ops.attention_fwd_raw(dev(q), dev(k), dev(v))
    o_ref = _attn_ref(q, k, v)
    assert (o.view(B, S, H, 64).permute(0, 2, 1, 3).double().cpu() - o_ref).abs().max().item() < 0.03
    assert torch.isfinite(lse).all()


@pytest.mark.parametrize("S", [130, 1000])
def test_attention_extreme_outliers_strip_redo(ops, S):
    """Scores that outgrow the running max by more than the optimistic exp2 can represent (> 2^64, and > 2^128 = inf) in
    late tiles: the forward has to notice and redo the query strip with the plain online softmax.  Also an early huge
    score followed by ordinary ones (everything after it underflows against the new max)."""
    g = torch.Generator().manual_seed(S)
    B, H = 1, 2
    q, k, v = (torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16) for _ in range(3))
    for key, row, gain in ((S - 3, 5, 70.0), (S - 60, 40, 130.0), (70, 9, 200.0)):
        k[0, 0, key] = (q[0, 0, row].float() * gain / 8).to(torch.bfloat16)
    # scores of +-100 nats make the result ill-conditioned in the bf16 rounding of q*scale*log2(e): hand the kernel the
    # pre-scaled q (its documented contract) and build the fp64 reference from exactly those values
    qp = (q.float() * (0.125 * 1.4426950408889634)).to(torch.bfloat16)
    o, lse = ops.attention_fwd_raw(dev(qp), dev(k), dev(v), q_prescaled=True)
    s2 = qp.double() @ k.double().transpose(-1, -2)                      # log2 units
    mx = s2.max(-1, keepdim=True).values
    p = torch.exp2(s2 - mx)
    w = p / p.sum(-1, keepdim=True)
    o_ref = w @ v.double()
    lse_ref = (mx + torch.log2(p.sum(-1, keepdim=True))).squeeze(-1)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    err = (o.view(B, S, H, 64).permute(0, 2, 1, 3).double().cpu() - o_ref).abs()
    assert (err <= 0.02 + 0.008 * o_ref.abs()).all(), err.max().item()   # 0.008 |o|: bf16 rounding of one-hot rows (|v| up to ~4)
    # rows the w1 kernel keeps sum the bf16-rounded weights (tests/attn_tol.py); the redone strips sum in fp32
    lerr = (lse.double().cpu() - lse_ref).abs()
    assert (lerr <= lse2_tol(w, lse_ref)).all(), (lerr / lse2_tol(w, lse_ref)).max().item()


@pytest.mark.parametrize("S,gap,split", [(1000, 126.5, 0), (1000, 118.0, 0), (1000, 104.0, 0), (2100, 126.5, 3), (1000, 90.0, 0)])
def test_attention_row_between_overflow_of_o_and_overflow_of_l(ops, S, gap, split):
    """Round 6, found by `bench.py --weights trained_like` (tools/attn_fault_repro.py: one row of block 38 of the cfg2 model at QK-norm gain 2.5): the w1 forward
    shifts a row by M' = min(bound, sampled maximum + 64).  A key the sample missed whose score lies `gap` = 100-128 log2 units above M' gives a weight 2^gap: the
    row SUM stays finite (2^gap < 2^128), the O accumulators do not (2^gap |v| overflows) -- a strip must be flagged on the size of l (>= 2^118) and on the
    accumulators themselves, not only on l = inf.  gap 90 stays on the fast path and has to be right there."""
    g = torch.Generator().manual_seed(S + int(gap))
    B, H = 1, 2
    q, k, v = (torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16) for _ in range(3))
    row, key = 5, 7                                            # key 7 is not a multiple of S // 64: the sample does not see it
    assert key % (S // 64) != 0
    qp = (q.float() * (0.125 * 1.4426950408889634)).to(torch.bfloat16)
    s_row = qp[0, 1, row].double() @ k[0, 1].double().t()
    ms = s_row[torch.arange(64) * (S // 64)].max().item()
    want = ms + 64.0 + gap                                     # the score key 7 gets
    k[0, 1, key] = (q[0, 1, row].float() * (want / float(qp[0, 1, row].double() @ q[0, 1, row].double()))).to(torch.bfloat16)
    v[0, 1, key] = 8.0 * torch.sign(v[0, 1, key].float()).to(torch.bfloat16)
    s2 = qp.double() @ k.double().transpose(-1, -2)
    bound = qp[0, 1, row].double().norm() * k[0, 1].double().norm(dim=-1).max()
    got_gap = s2[0, 1, row].max().item() - min(bound.item(), ms + 64.0)
    assert abs(got_gap - gap) < 1.0, got_gap                    # the row really sits where the test says (bf16 rounding of k moves it a little)
    o, lse = ops.attention_fwd_raw(dev(qp), dev(k), dev(v), q_prescaled=True, split_mode=split)
    mx = s2.max(-1, keepdim=True).values
    p = torch.exp2(s2 - mx)
    w = p / p.sum(-1, keepdim=True)
    o_ref = w @ v.double()
    lse_ref = (mx + torch.log2(p.sum(-1, keepdim=True))).squeeze(-1)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    err = (o.view(B, S, H, 64).permute(0, 2, 1, 3).double().cpu() - o_ref).abs()
    assert (err <= 0.02 + 0.008 * o_ref.abs()).all(), err.max().item()
    lerr = (lse.double().cpu() - lse_ref).abs()
    assert (lerr <= lse2_tol(w, lse_ref)).all(), (lerr / lse2_tol(w, lse_ref)).max().item()


@pytest.mark.parametrize("S,split", [(1000, 4), (1000, 8), (2100, 3), (641, 5)])
def test_attention_fwd_key_range_split_matches_single_launch(ops, S, split):
    """The launcher's tail treatment (tasks cut into key-range chunks + merge, vgpa_attn_fwd_w1_res) against the single launch
    and the fp64 reference, incl. a spiked key in a late chunk and a ragged last tile."""
    g = torch.Generator().manual_seed(S + split)
    B, H = 1, 3
    q, k, v = (torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16) for _ in range(3))
    k[0, 1, S - 70] = (q[0, 1, 11].float() * 2.0).to(torch.bfloat16)
    o0, lse0 = ops.attention_fwd_raw(dev(q), dev(k), dev(v), split_mode=0)
    o1, lse1 = ops.attention_fwd_raw(dev(q), dev(k), dev(v), split_mode=split)
    o_ref = _attn_ref(q, k, v)
    assert (o1.view(B, S, H, 64).permute(0, 2, 1, 3).double().cpu() - o_ref).abs().max().item() < 0.02
    assert (o1.float() - o0.float()).abs().max().item() < 0.02          # both round the same value to bf16: <= 1 ulp apart
    w = torch.softmax(q.double() @ k.double().transpose(-1, -2) / 8.0, -1)
    tol = lse2_tol(w, lse0.double().cpu())
    assert ((lse1 - lse0).abs().double().cpu() <= 2.0 * tol + 1e-3).all()      # each launch rounds its own weights (every chunk of a row shifts by the same sampled M')


@pytest.mark.parametrize("B,H,S,split", [(1, 2, 1000, 4), (1, 2, 1100, 7), (1, 2, 641, 3), (1, 2, 513, 4), (2, 3, 769, 6)],
                         ids=["1000-4", "1100-7", "641-3", "513-4", "769-6"])
def test_attention_bwd_range_split_matches_single_launch(ops, B, H, S, split):
    """dK/dV split along the query tiles and dQ split along the key tiles (fp32 partials + merge) against the single launches
    and the fp64 reference.  S = 513 and 769 are one row past a multiple of the 256-row task, where vgpa_attn_bwd_split_workspace_bytes is
    tightest against what a forced split needs (a short workspace would be VGPA_ERR_WORKSPACE, raised by the call)."""
    g = torch.Generator().manual_seed(S * split)
    q, k, v, do = (torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16) for _ in range(4))
    qd, kd, vd, dod = dev(q), dev(k), dev(v), dev(do)
    o, lse = ops.attention_fwd_raw(qd, kd, vd, split_mode=0)
    ov = o.view(B, S, H, 64).permute(0, 2, 1, 3)
    outs = []
    for sm in (0, split):
        dq, dk, dv = (torch.zeros(B, H, S, 64, dtype=torch.bfloat16, device="cuda") for _ in range(3))
        ops.attention_bwd_raw(qd, kd, vd, ov, dod, lse, dq, dk, dv, split_mode=sm)
        outs.append((dq, dk, dv))
    _, dq_ref, dk_ref, dv_ref = _attn_ref(q, k, v, do)
    for name, a0, a1, r in (("dq", outs[0][0], outs[1][0], dq_ref), ("dk", outs[0][1], outs[1][1], dk_ref), ("dv", outs[0][2], outs[1][2], dv_ref)):
        tol = 0.03 * r.abs().max().item() + 2e-3
        assert (a1.double().cpu() - r).abs().max().item() < tol, name
        assert (a1.float() - a0.float()).abs().max().item() < 0.5 * tol, name     # same sums, different fp32 association


def test_cabi_rejects_bad_arguments(ops):
    from videogpa_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    x = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
    assert lib.vgpa_gelu_tanh_fwd(None, 64, x.data_ptr(), st) == -1                    # null pointer
    assert lib.vgpa_gelu_tanh_fwd(x.data_ptr(), 60, x.data_ptr(), st) == -1            # n % 8 != 0
    import ctypes
    s3 = (ctypes.c_int64 * 3)(64, 64, 64)
    f = torch.zeros(8, dtype=torch.float32, device="cuda")
    wb = lib.vgpa_attn_fwd_w1_workspace_bytes(1, 1, 1)
    aws = torch.zeros(wb, dtype=torch.uint8, device="cuda")

    def fwd(strides, head_dim, wsp):
        return lib.vgpa_attn_fwd_w1_res(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 0, f.data_ptr(), strides, s3, s3, s3, None, 1, 1, 1, head_dim, 0.1, 0,
                                        wsp, wb, st)
    assert fwd(s3, 128, aws.data_ptr()) == -1                                          # head_dim
    bad = (ctypes.c_int64 * 3)(64, 64, 60)
    assert fwd(bad, 64, aws.data_ptr()) == -1                                          # stride
    assert fwd(s3, 64, None) == -1                                                     # the workspace is mandatory
    ws = torch.zeros(16, dtype=torch.uint8, device="cuda")
    assert lib.vgpa_dpo_loss_fwd(*([x.data_ptr()] * 6), 1, 64, 64, 64, 64, 1, 1.0, 0.0, 0, 0, f.data_ptr(), f.data_ptr(), None, ws.data_ptr(), 16, st) == -3
    with pytest.raises(ValueError, match="Unknown loss type"):
        ops.dpo_loss(x.view(1, 64), x.view(1, 64), x.view(1, 64), x.view(1, 64), x.view(1, 64), x.view(1, 64), loss_type="nope")


def test_ln_modulate_max_width_and_batch_boundaries(ops):
    g = torch.Generator().manual_seed(8)
    B, S, D, Lt = 3, 5, 4096, 2          # rows-per-wave groups straddle batch and text/video boundaries
    x = torch.randn(B, S, D, generator=g).to(torch.bfloat16)
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    mod = 0.3 * torch.randn(B, 4, D, generator=g)
    y = ops.ln_modulate(dev(x), dev(w), dev(b), dev(mod), Lt, 1e-5)
    n = F.layer_norm(x.double(), (D,), w.double(), b.double(), 1e-5)
    sc = torch.cat([mod[:, 3:4].expand(B, Lt, D), mod[:, 1:2].expand(B, S - Lt, D)], 1).double()
    sh = torch.cat([mod[:, 2:3].expand(B, Lt, D), mod[:, 0:1].expand(B, S - Lt, D)], 1).double()
    assert (y.double().cpu() - (n * sc + sh)).abs().max().item() < 0.04
    # per element (tests/row_tol.py), where 0.04 absolute said nothing about which modulation row a token took; this test's tables hold scale, not 1 + scale
    s1p, shf = row_tol.cog_rows(mod[:, 1], mod[:, 3], B, S, Lt), row_tol.cog_rows(mod[:, 0], mod[:, 2], B, S, Lt)
    ref = row_tol.cog_ln_fwd_ref64(x, w, b, s1p, shf, 1e-5)
    assert not row_tol.judge("ln_modulate D 4096", y.cpu(), ref[0], row_tol.cog_ln_fwd_tol(x, w, b, s1p, shf, 1e-5, ref[0])[0])


@pytest.mark.parametrize("B,S,D,Lt", [(2, 37, 128, 6), (1, 300, 3072, 226), (3, 21, 512, 0), (2, 33, 256, 33)])
def test_residual_ln_fused_equals_composition(ops, B, S, D, Lt):
    """x' = x + gate*y ; n = LN-mod(x')  fused in one pass, against gate_residual + ln_modulate_v1 run separately, forward
    and backward (with a gradient arriving on BOTH outputs)."""
    g = torch.Generator().manual_seed(S * D)
    x = torch.randn(B, S, D, generator=g).to(torch.bfloat16)
    y = torch.randn(B, S, D, generator=g).to(torch.bfloat16)
    gates = torch.randn(B, 2, D, generator=g).to(torch.bfloat16).float()
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    mod = 0.3 * torch.randn(B, 4, D, generator=g)
    mod[:, 1] += 1
    mod[:, 3] += 1
    dxn = torch.randn(B, S, D, generator=g).to(torch.bfloat16)
    dn = torch.randn(B, S, D, generator=g).to(torch.bfloat16)
    outs = []
    for fused in (True, False):
        xd, yd = dev(x).requires_grad_(True), dev(y).requires_grad_(True)
        if fused:
            xn, n = ops.residual_ln(xd, yd, dev(gates), dev(w), dev(b), dev(mod), Lt, 1e-5)
        else:
            xn = ops.gate_residual(xd, yd, dev(gates), Lt)
            n = ops.ln_modulate_v1(xn, dev(w), dev(b), dev(mod), Lt, 1e-5)
        torch.autograd.backward([xn, n], [dev(dxn), dev(dn)])
        outs.append((xn.detach(), n.detach(), xd.grad, yd.grad))
    f, u = outs
    assert torch.equal(f[0], u[0])                                        # residual stream: same bf16 rounding order
    assert (f[1].float() - u[1].float()).abs().max().item() <= 0.032      # LN output: <= 1 bf16 ulp of O(4) values
    for i in (2, 3):
        sc = u[i].float().abs().max().item()
        assert (f[i].float() - u[i].float()).abs().max().item() <= 0.02 * sc, i


def test_flow_matching_noise_velocity_bit_exact(ops):
    """Wan2.2 flow-matching step inputs (train/Wan2.2-TI2V-5B/03_train.py:103-116,203-207,235-236), bit-exact vs the torch
    expressions of the reference incl. its fp32 promotion of x_t."""
    g = torch.Generator().manual_seed(21)
    B, shape = 3, (48, 5, 6, 8)                                   # Wan latents are [C,F,H,W]
    x = torch.randn(B, 2, *shape, generator=g).to(torch.bfloat16)
    eps = torch.randn(B, *shape, generator=g).to(torch.bfloat16)
    t = torch.tensor([1, 500, 999])
    sigma = ops.flow_sigma(t, 1000, 5.0)
    s_ref = t.float() / 1000
    s_ref = 5.0 * s_ref / (1 + (5.0 - 1) * s_ref)
    assert torch.equal(sigma, s_ref)
    xt, v = ops.flow_noise_velocity_paired(dev(x), dev(eps), dev(sigma))
    sg = s_ref.view(B, 1, 1, 1, 1)
    for p in range(2):
        ref_xt = (1.0 - sg) * x[:, p] + sg * eps
        assert ref_xt.dtype == torch.float32 and xt.dtype == torch.float32
        assert torch.equal(xt[:, p].cpu(), ref_xt)
        assert torch.equal(v[:, p].cpu(), eps - x[:, p])


def test_linear_lora_ext_padded_zero_copy_and_reference_pass(ops):
    """The K-extension layout: LN output produced as the head of a [.., K+R] buffer is used in place (no copy), the adapter-off
    pass (zero tail) equals the adapter-on pass with B = 0 BIT FOR BIT (policy == reference at initialisation -> loss = ln 2), and
    the padded gradient buffers of residual_ln / qknorm_attention are recognised."""
    g = torch.Generator().manual_seed(9)
    Bt, S, K, N, r = 2, 50, 128, 256, 8
    rp = 16
    x = dev(torch.randn(Bt, S, K, generator=g).to(torch.bfloat16))
    w, b = dev(1 + 0.1 * torch.randn(K, generator=g)), dev(0.1 * torch.randn(K, generator=g))
    n = ops.ln_modulate(x, w, b, None, 0, 1e-5, n_pad=rp)
    assert n.shape == (Bt, S, K) and n.stride() == (S * (K + rp), K + rp, 1)
    base = ops._padded_base(n.reshape(-1, K), K + rp)
    assert base is not None and base.data_ptr() == n.data_ptr()
    n_plain = ops.ln_modulate(x, w, b, None, 0, 1e-5)
    assert torch.equal(n, n_plain)
    W = dev((torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16))
    bias = dev(torch.randn(N, generator=g).to(torch.bfloat16))
    A = dev(torch.randn(r, K, generator=g) / K ** 0.5)
    B0 = torch.zeros(N, r, device="cuda")
    B1 = dev(torch.randn(N, r, generator=g) * 0.3)
    ext = ops.LoraExt()
    y_off = ops.linear_lora_ext(n, W, bias, ext, [(A, B1, 2.0)], enabled=False)
    ext0 = ops.LoraExt()
    y_b0 = ops.linear_lora_ext(n, W, bias, ext0, [(A, B0, 2.0)], enabled=True)
    assert torch.equal(y_off, y_b0)
    y_on = ops.linear_lora_ext(n, W, bias, ext, [(A, B1, 2.0)], enabled=True)
    ref = F.linear(n.double().cpu(), W.double().cpu(), bias.double().cpu()) + 2.0 * F.linear(
        F.linear(n.double().cpu(), A.to(torch.bfloat16).double().cpu()), B1.to(torch.bfloat16).double().cpu())
    assert (y_on.double().cpu() - ref).abs().max().item() < 0.02 * ref.abs().max().item()
    # adapter values changed in place through raw pointers (the AdamW kernel): refreshed after bump_adapter_epoch()
    B1.data.mul_(0.0)
    ops.bump_adapter_epoch()
    assert torch.equal(ops.linear_lora_ext(n, W, bias, ext, [(A, B1, 2.0)], enabled=True), y_b0)


@pytest.mark.parametrize("r,n_slices", [(8, 1), (64, 3), (12, 3)])
def test_lora_ext_refresh_kernel_is_bit_exact_with_pefts_rounding(ops, r, n_slices):
    """vgpa_lora_ext_refresh (one launch per adapter after an optimizer step) against the torch statements it replaces, which follow PEFT's forward
    (peft/tuners/lora/layer.py: the adapter is cast to the activation dtype, then scaled): A_cat = bf16(A); sB = bf16(float(bf16(B)) * s) into the
    [N, K + R] operand's tail columns and into sBt; A^T into the [K, N + R] operand's tail columns.  Bit-exact, padding columns stay zero, a fused
    q/k/v projection (3 slices) addresses every adapter's own rows / columns; the refresh after an in-place update sees the new values."""
    g = torch.Generator().manual_seed(100 + r)
    K, Dn = 192, 128
    N = n_slices * Dn
    W = dev((torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16))
    loras = [(dev(torch.randn(r, K, generator=g) / K ** 0.5), dev(torch.randn(Dn, r, generator=g) * 0.3), 2.0 * (i + 1) / 3.0) for i in range(n_slices)]
    ext = ops.LoraExt().refresh(W, n_slices, loras)
    rp, R = ext.rp, ext.R
    assert R == n_slices * rp and ext.W_ext.shape == (N, K + R) and ext.Wt_ext.shape == (K, N + R)

    def expect():
        W_ext = torch.zeros(N, K + R, dtype=torch.bfloat16, device="cuda")
        W_ext[:, :K] = W
        A_cat = torch.zeros(R, K, dtype=torch.bfloat16, device="cuda")
        sBt = torch.zeros(n_slices, rp, Dn, dtype=torch.bfloat16, device="cuda")
        for j, (A, Bm, sc) in enumerate(loras):
            A_cat[j * rp:j * rp + r] = A.to(torch.bfloat16)
            sB = (Bm.to(torch.bfloat16).float() * sc).to(torch.bfloat16)
            W_ext[j * Dn:(j + 1) * Dn, K + j * rp:K + j * rp + r] = sB
            sBt[j, :r] = sB.t()
        Wt_ext = torch.zeros(K, N + R, dtype=torch.bfloat16, device="cuda")
        Wt_ext[:, :N] = W.t()
        Wt_ext[:, N:] = A_cat.t()
        return W_ext, Wt_ext, A_cat, sBt
    for got, want, name in zip((ext.W_ext, ext.Wt_ext, ext.A_cat, ext.sBt), expect(), ("W_ext", "Wt_ext", "A_cat", "sBt")):
        assert torch.equal(got, want), name
    for A, Bm, _ in loras:           # what the AdamW kernel does: values change behind autograd's back, the epoch is bumped
        A.data.mul_(1.5)
        Bm.data.add_(0.25)
    ops.bump_adapter_epoch()
    ext.refresh(W, n_slices, loras)
    for got, want, name in zip((ext.W_ext, ext.Wt_ext, ext.A_cat, ext.sBt), expect(), ("W_ext", "Wt_ext", "A_cat", "sBt")):
        assert torch.equal(got, want), name + " after update"


@pytest.mark.parametrize("kind", ["bf16", "int8"])
@pytest.mark.parametrize("S,split", [(1000, 0), (1000, 4), (100, 0), (2100, 3)])
def test_attention_output_residual_and_precise_delta(ops, S, split, kind):
    """vgpa_attn_fwd_w1_res / vgpa_attn_bwd_prep_w1_res / vgpa_attn_bwd_delta_res ("precise delta" in ops.py): the forward also stores what the bf16
    rounding of its output dropped -- as a bf16 residual o_res = O_fp32 - bf16(O) (VGPA_RES_BF16) or as eight further mantissa bits per element
    (VGPA_RES_8, csrc/common.h res8; decoded here by ops.res8_decode) -- and the backward forms delta = rowsum(dO o O) from the completed output.
    Diffuse attention over values with a large mean (|O| ~ 2, so bf16(O) is off by up to 4e-3 while the kernel's fp32 O is good to ~2e-4): (i) the
    completed output is >= 4x closer to the fp64 output than o alone, through the main launch, the key-range split + merge (split > 0) and the
    online-softmax path (S < 128); (ii) both delta kernels reproduce rowsum(dO o O_completed) of the stored tensors to fp32 rounding; (iii) dQ -- whose
    rows pick up -d(delta) * sum_j P_ij K_j when delta comes from the rounded O -- is >= 3x closer to the fp64 gradient with the residual than
    without (k carries a mean, so that sum is not small)."""
    from videogpa_amd import _lib
    g = torch.Generator().manual_seed(7 * S + split)
    B, H = 1, 2
    q = (0.3 * torch.randn(B, H, S, 64, generator=g)).to(torch.bfloat16)
    k = (torch.randn(B, H, S, 64, generator=g) + 1.0).to(torch.bfloat16)
    v = (torch.randn(B, H, S, 64, generator=g) + 2.0).to(torch.bfloat16)
    do = torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16)
    qd, kd, vd, dod = dev(q), dev(k), dev(v), dev(do)
    if kind == "bf16":
        o_res = torch.full((B, S, H * 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    else:
        o_res = torch.full((B, S, H * 64), 7, dtype=torch.uint8, device="cuda")           # 7 = a residual of -121/256 ulp: never what a written byte looks like on average
    rk = ops._res_kind(o_res)
    o, lse = ops.attention_fwd_raw(qd, kd, vd, split_mode=split, o_res=o_res)
    o_ref, dq_ref, dk_ref, dv_ref = _attn_ref(q, k, v, do)
    bhsd = lambda t: t.view(B, S, H, 64).permute(0, 2, 1, 3)
    o_full = (o.double() + o_res.double()) if kind == "bf16" else ops.res8_decode(o, o_res).double()      # fp32 holds bf16 + 8 bits exactly
    res = o_full - o.double()
    assert torch.isfinite(o_full).all()
    e_plain = (bhsd(o).double().cpu() - o_ref).abs().max().item()
    e_res = (bhsd(o_full).cpu() - o_ref).abs().max().item()
    assert e_plain > 2e-3 and e_res < 0.25 * e_plain, (e_plain, e_res)
    assert (res.abs() <= 2.0 ** -8 * o.double().abs() + 1e-30).all()          # a residual never exceeds half an ulp of o
    assert res.abs().mean().item() > 2.0 ** -12 * o.double().abs().mean().item()         # and it was written (the fill pattern is gone)
    # (ii) the two delta kernels
    want = (dod.double() * bhsd(o_full)).sum(-1)
    st = lambda t: ops._bhs_strides(t)
    for name in ("prep", "delta"):
        delta = torch.empty(B, H, S, dtype=torch.float32, device="cuda")
        if name == "prep":
            stats = torch.empty(B, H, 2, S, dtype=torch.float32, device="cuda")
            _lib.call("vgpa_attn_bwd_prep_w1_res", bhsd(o), bhsd(o_res), rk, dod, lse, st(bhsd(o)), st(bhsd(o_res)), st(dod), delta, stats, B, H, S, 64, ops._stream())
            assert torch.equal(stats[:, :, 1], -delta) and torch.equal(stats[:, :, 0], -lse)
        else:
            _lib.call("vgpa_attn_bwd_delta_res", bhsd(o), bhsd(o_res), rk, dod, st(bhsd(o)), st(bhsd(o_res)), st(dod), delta, B, H, S, 64, ops._stream())
        assert (delta.double() - want).abs().max().item() < 1e-4 * want.abs().max().item() + 1e-5, name
    # (iii) dQ with and without the residual
    errs = {}
    for tag, r in (("plain", None), ("res", bhsd(o_res))):
        dq, dk, dv = (torch.empty(B, H, S, 64, dtype=torch.bfloat16, device="cuda") for _ in range(3))
        ops.attention_bwd_raw(qd, kd, vd, bhsd(o), dod, lse, dq, dk, dv, o_res=r)
        errs[tag] = (dq.double().cpu() - dq_ref).norm().item() / dq_ref.norm().item()
        for nm, a, ref in (("dk", dk, dk_ref), ("dv", dv, dv_ref)):
            assert (a.double().cpu() - ref).abs().max().item() < 0.03 * ref.abs().max().item() + 2e-3, (tag, nm)
    assert errs["res"] < 0.05 and errs["res"] < errs["plain"] / 3, errs
