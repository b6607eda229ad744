"""What gives the per-element attention tolerances (tests/attn_tol.py, over the sums of tests/attn_ref64.py) their teeth -- on the CPU, no kernel involved.

A rounding EMULATION of the kernels (fp32 scores and accumulation, weights rounded to bf16 where they multiply V and dO, the row sum of the rounded weights, lse2 in
fp32, the output as bf16 + its int8 residual, P~ = exp2(s2 - lse2~), dS rounded to bf16, results rounded to bf16) must stay inside every bound and inside the rms
ratio; the same emulation with ONE defect of the kind a long-sequence kernel makes must be rejected by both; and the absolute tolerances the suite had for short
sequences ("err < 0.02", "0.03 max + 2e-3") accept those defects -- the reason this file exists.

Shapes: 240 query rows (rows 0..127 and the 112 rows of the last, partial strip) against all 17 776 keys (head_dim 64) / 18 480 keys (head_dim 128), N(0,1) operands;
full S = 333 and 1000 (and 700 x 1000 at head_dim 128) with k and v carrying a mean, where delta's precision shows in dQ.

Measured with the faithful emulation (max err/tol | rms(err)/rms(sigma) over the head), every term of attn_tol.PER_ELEMENT included:
    17 776 keys, d 64, 240 rows :  O 0.60 | 0.84   lse2 0.13   dQ 0.50 | 0.84   dK 0.51 | 0.84   dV 0.53 | 0.84
    18 480 keys, d 128, 240 rows:  O 0.55 | 0.83   lse2 0.00   dQ 0.51 | 0.83   dK 0.56 | 0.84   dV 0.52 | 0.84
    S = 333, d 64 (k, v + mean) :  O 0.93 | 1.00   lse2 0.27   dQ 0.38 | 0.76   dK 0.33 | 0.83   dV 0.34 | 0.84
    S = 1000, d 64 (k, v + mean):  O 0.96 | 0.99   lse2 0.24   dQ 0.43 | 0.76   dK 0.36 | 0.84   dV 0.29 | 0.83
    700 x 1000, d 128 (+ mean)  :  O 0.92 | 1.00   lse2 0.00   dQ 0.37 | 0.75   dK 0.31 | 0.84   dV 0.34 | 0.85
(printed again by the tests.  0.84 = the variance of a bf16 rounding over the mantissas that occur against unit^2 / 3 at mantissa 1.0; with a mean in v the output's own
rounding, ulp^2 / 12 exactly, dominates O: 1.00.  There an exactly rounded O reaches 0.96 of half an ulp; "2^-9 |o|" in its place rejects the emulation, asserted below.)
One defect each, worst tensor (max err/tol | worst 256-row rms ratio) at 17 776 keys: last 48 keys dropped O 32.9 | 20.1; one key dropped O 8.2 | 3.2; one 64-key tile
twice O 30.0 | 22.2; lse2 of a strip + 2^-6: lse2 19.9, dQ 1.8 | 3.8; last strip's rows from the previous strip: > 270 | > 350 everywhere; at S = 1000 delta from the bf16 O
alone: dQ 12.0 | 26.0.
e4m3 weights (vgpa_attn128_fwd_f8's rounding, N(0,1)): faithful at 18 480 keys O 0.53 | 0.73, dQ 0.47 | 0.77, dK 0.53 | 0.83, dV 0.54 | 0.84; 700 x 1500: O 0.56 | 0.69, dQ 0.52 | 0.74,
dK 0.50 | 0.80, dV 0.45 | 0.84.  Defects at 18 480 keys (worst tensor, lse2 aside): last 48 keys dropped O 1.36 | 1.62 (lse2 7.2); a tile twice O 1.93 | 1.75 (lse2 8.2); lse2 of a
strip + 2^-6 dV 1.9 | 3.6; strip copy > 20 | > 30.  A 4-bit weight is 16 x coarser than a bf16 one: ONE key of 18 480 (O 0.54 | 0.74, lse2 0.69) is below what this bound
can show and is not asserted; of 1500 it is seen per element (O 2.9, lse2 10.2) and not by the rms ratio.
Known limit, measured here and NOT covered by a term: the e4m3 rounding of a row's weights is not zero-mean -- sum_j (P8_ij - p_ij) / sum_j p_ij = -7e-4 for every row at
18 480 keys (bf16: -3e-6), against 3e-4 of independent part.  With a fp32 row sum that is a common factor on O (below half a bf16 ulp) and on the precise delta; where
|delta| is large (v carrying a mean of 2, 18 480 keys) the emulation's dQ stays inside the per-element bound (0.66) and misses the rms ratio (2.4).  The device case and
this file's e4m3 cases use N(0,1) operands, where delta is small and the effect is not seen (dQ 0.77)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_tol as T  # noqa: E402
from attn_ref64 import attn_ref64  # noqa: E402

C64, C128 = 64 ** -0.5 * T.LOG2E, 128 ** -0.5 * T.LOG2E
bf = lambda x: x.to(torch.bfloat16).float()


def res8_complete(o32):
    """bf16(o) + the int8 residual of csrc/common.h: steps of 2^-15 of the binade of bf16(o)"""
    ob = bf(o32)
    step = torch.exp2(torch.floor(torch.log2(ob.abs().clamp_min(1e-30))) - 15.0)
    return ob + torch.clamp(torch.round((o32 - ob) / step), -128, 127) * step


def e4m3_weights(p, tile=64):
    """the weights as vgpa_attn128_fwd_f8 hands them to its second product (csrc/attention_hd128.hip, tools/gen_w1_asm.py Fwd128F8Loop): per row and 64-key tile
    x = (frexp exponent of the tile's sum) - 8, P8 = e4m3(p / 2^x) 2^x"""
    Skv = p.shape[-1]
    pt = torch.nn.functional.pad(p, (0, (-Skv) % tile)).unflatten(-1, (-1, tile))
    x = (torch.frexp(pt.sum(-1, keepdim=True))[1] - 8).clamp_min(-126).float()
    return ((pt / torch.exp2(x)).to(torch.float8_e4m3fn).float() * torch.exp2(x)).flatten(-2)[..., :Skv]


def emulate(qs, k, v, do, rows, smul=1.0, dq_mul=0.125, dk_mul=T.LN2, mut=None, precise=True, rounded_rowsum=True, weights="bf16"):
    """the kernels' arithmetic in fp32 with their roundings; mut: None or (name, argument) -- one defect.  weights: what the forward rounds its weights to where they
    multiply V ("bf16", or "e4m3": e4m3_weights; the backward rounds to bf16 either way)"""
    name, arg = mut if mut else (None, None)
    Skv = k.shape[0]
    src = rows.clone()
    if name == "strip_copy":                  # the rows of the last partial strip computed from the previous strip's queries
        last = (qs.shape[0] - 1) // 256 * 256
        src = torch.where(rows >= last, rows - 256, rows)
    qf, kf, vf, dof = qs.float()[src], k.float(), v.float(), do.float()[src]
    s2 = (qf @ kf.t()) * smul
    mult = torch.ones(Skv)
    if name == "drop_tail":
        mult[Skv - arg:] = 0
    if name == "drop_key":
        mult[arg] = 0
    if name == "tile_twice":
        mult[64 * arg:64 * arg + 64] = 2
    m = s2.max(-1, keepdim=True).values
    p = torch.exp2(s2 - m)
    pb = (bf(p) if weights == "bf16" else e4m3_weights(p)) * mult
    l = (pb if rounded_rowsum else p * mult).sum(-1, keepdim=True)
    o32 = (pb @ vf) / l
    lse = (m + torch.log2(l)).squeeze(-1)
    if name == "lse_strip":
        lse = torch.where(rows // 256 == arg, lse + 2.0 ** -6, lse)
    o_b = bf(o32)
    o_delta = res8_complete(o32) if precise and name != "delta_bf16" else o_b
    P = torch.exp2(s2 - lse.unsqueeze(-1))
    delta = (dof * o_delta).sum(-1, keepdim=True)
    dv = bf(bf(P).t() @ dof)
    dS = bf(P * (dof @ vf.t() - delta))
    dq = bf(dq_mul * (dS @ kf))
    dk = bf(dk_mul * (dS.t() @ qf))
    return {"o": o_b, "lse2": lse, "dq": dq, "dk": dk, "dv": dv}


judge = T.judge          # (emulation, reference[, delta]) -> (problems, figures per tensor)


def old_tolerances_accept(E, R):
    """the assertions of test_gpu_kernels.py::test_attention_fwd_bwd_raw as they stood alone: |o - ref| < 0.02, gradients 0.03 max|ref| + 2e-3, lse2 1.5e-2"""
    ok = float((E["o"].double() - R["o"]).abs().max()) < 0.02 and float((E["lse2"].double() - R["lse2"]).abs().max()) < 1.5e-2
    for n in ("dq", "dk", "dv"):
        ok = ok and float((E[n].double() - R[n]).abs().max()) < 0.03 * float(R[n].abs().max()) + 2e-3
    return ok


def rejected(problems):
    per_element = any("over the bound" in p or "over lse2_tol" in p for p in problems)
    rms = any("rms(err)" in p for p in problems)
    return per_element, rms


def make(Sq, Skv, D, seed, mean=False):
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(S_, D, generator=g) for S_ in (Sq, Skv, Skv, Sq))
    if mean:       # diffuse rows over keys and values with a common component: sum_j P_ij K_j and O are not small, so delta's precision shows in dQ
        q, k, v = 0.3 * q, k + 1.0, v + 2.0
    return tuple(t.to(torch.bfloat16) for t in (q, k, v, do))


def contract(q, D):
    """-> (qs, kwargs shared by attn_ref64 and emulate) for the head_dim's kernels"""
    if D == 64:
        return (q.float() * C64).to(torch.bfloat16), dict(smul=1.0, dq_mul=64 ** -0.5, dk_mul=T.LN2)
    return q, dict(smul=C128, dq_mul=128 ** -0.5, dk_mul=128 ** -0.5)


FULL = [(17776, 64, True), (18480, 128, False)]


@pytest.mark.parametrize("S,D,rounded", FULL)
def test_emulation_at_the_real_key_lengths_and_its_mutations(S, D, rounded):
    q, k, v, do = make(S, S, D, seed=S)
    qs, kw = contract(q, D)
    last = (S - 1) // 256 * 256
    rows = torch.cat([torch.arange(0, 128), torch.arange(last, S)])
    R = attn_ref64(qs, k, v, do, rows=rows, rounded_rowsum=rounded, **kw)
    E = emulate(qs, k, v, do, rows, rounded_rowsum=rounded, **kw)
    problems, figs = judge(E, R)
    print(S, D, "faithful", figs)
    assert not problems, problems
    accepted_by_old = []
    for mut in (("drop_tail", 48), ("drop_key", 9001), ("tile_twice", 100), ("lse_strip", 0), ("strip_copy", None)):
        M = emulate(qs, k, v, do, rows, rounded_rowsum=rounded, mut=mut, **kw)
        problems, figs = judge(M, R)
        pe, rms = rejected(problems)
        print(S, D, mut, {n: (round(f["max_err_over_tol"], 2), round(f.get("worst_block_rms_ratio", 0), 2)) for n, f in figs.items()})
        assert pe and rms, (mut, problems)
        if mut[0] in ("drop_tail", "drop_key", "tile_twice", "lse_strip"):
            assert any(("o " in p or "lse2 " in p or "dq " in p) for p in problems)
        if old_tolerances_accept(M, R):
            accepted_by_old.append(mut[0])
    # the documented reason for this file: what the suite asserted before lets a kernel lose keys or count a tile twice (the strip's lse2, 2^-6 = 0.0156 off, its
    # "< 1.5e-2" just catches -- where an lse2 reference exists at all, which at this length it did not)
    assert {"drop_tail", "drop_key", "tile_twice"} <= set(accepted_by_old), accepted_by_old


@pytest.mark.parametrize("Sq,Skv,D", [(333, 333, 64), (1000, 1000, 64), (700, 1000, 128)])
def test_emulation_of_the_gradients_on_small_full_cases_and_its_mutations(Sq, Skv, D):
    q, k, v, do = make(Sq, Skv, D, seed=Sq + D, mean=True)
    qs, kw = contract(q, D)
    rounded = D == 64
    rows = torch.arange(Sq)
    R = attn_ref64(qs, k, v, do, rounded_rowsum=rounded, **kw)
    E = emulate(qs, k, v, do, rows, rounded_rowsum=rounded, **kw)
    problems, figs = judge(E, R)
    print(Sq, Skv, D, "faithful", figs)
    assert not problems, problems
    # 2^-9 |o| in place of half an ulp would reject this exactly rounded output (|o| ~ 2: mantissas near 1.0)
    tol_o, _ = T.o_tol(R)
    rest = tol_o - T.half_ulp_bf16(R["o"].abs() + (tol_o - T.half_ulp_bf16(R["o"])))
    assert float(((E["o"].double() - R["o"]).abs() / (2.0 ** -9 * R["o"].abs() + rest.clamp_min(0))).max()) > 1.0
    # the textbook delta (bf16 O alone) is a legitimate mode with its own, 256 x wider delta term -- and a defect when the test claims the precise one
    Et = emulate(qs, k, v, do, rows, rounded_rowsum=rounded, precise=False, **kw)
    problems, _ = judge(Et, R, delta=None)
    assert not problems, problems
    muts = [("delta_bf16", None), ("drop_key", Skv // 2), ("drop_tail", Skv % 64 or 48), ("tile_twice", 2), ("lse_strip", 1), ("strip_copy", None)]
    accepted_by_old = []
    for mut in muts:
        M = emulate(qs, k, v, do, rows, rounded_rowsum=rounded, mut=mut, **kw)
        problems, figs = judge(M, R)
        pe, rms = rejected(problems)
        print(Sq, Skv, D, mut, {n: (round(f["max_err_over_tol"], 2), round(f.get("worst_block_rms_ratio", 0), 2)) for n, f in figs.items()})
        assert pe and rms, (mut, problems)
        if old_tolerances_accept(M, R):
            accepted_by_old.append(mut[0])
    if Skv == 1000:         # one key of a thousand lost: 2-8 x the derived bound in O and dQ, inside "err < 0.02" and "0.03 max + 2e-3"
        assert "drop_key" in accepted_by_old, accepted_by_old


@pytest.mark.parametrize("Sq,Skv", [(18480, 18480), (700, 1500)])
def test_e4m3_weight_emulation_and_its_mutations(Sq, Skv):
    """the e4m3 forward's weight model (attn_tol.PER_ELEMENT: 2^-4 relative, 2^-18 of the tile's sum) against an emulation that rounds the weights the way
    vgpa_attn128_fwd_f8 does, fp32 row sum of the unrounded weights, the backward on the same pre-scaled operands (N(0,1), the device test's)"""
    q, k, v, do = make(Sq, Skv, 128, seed=Skv + 1)
    qs = (q.float() * C128).to(torch.bfloat16)
    kw = dict(smul=1.0, dq_mul=128 ** -0.5, dk_mul=T.LN2)
    last = (Sq - 1) // 256 * 256
    rows = torch.cat([torch.arange(0, 128), torch.arange(last, Sq)])
    R = attn_ref64(qs, k, v, do, rows=rows, rounded_rowsum=False, p_unit=2.0 ** -4, p_sub=2.0 ** -18, **kw)
    E = emulate(qs, k, v, do, rows, rounded_rowsum=False, weights="e4m3", **kw)
    problems, figs = judge(E, R)
    print(Sq, Skv, "e4m3 faithful", figs)
    assert not problems, problems
    for mut in (("drop_tail", 48), ("tile_twice", 3), ("lse_strip", 0), ("strip_copy", None)):
        M = emulate(qs, k, v, do, rows, rounded_rowsum=False, weights="e4m3", mut=mut, **kw)
        problems, figs = judge(M, R)
        pe, rms = rejected(problems)
        print(Sq, Skv, "e4m3", mut, {n: (round(f["max_err_over_tol"], 2), round(f.get("worst_block_rms_ratio", 0), 2)) for n, f in figs.items()})
        assert pe and rms, (mut, problems)


def test_half_ulp_and_the_smallest_it_can_be():
    """2^-9 |x| is the least half an ulp can be, 2^-8 |x| the most: an exactly rounded value just above a power of two is 2^-8 |x| from it"""
    x = torch.tensor([1.00390625, 1.99609375, 0.75, 3.0], dtype=torch.float64)
    h = T.half_ulp_bf16(x)
    assert torch.equal(h, torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -9, 2.0 ** -7], dtype=torch.float64))
    assert bool(((x - x.to(torch.bfloat16).double()).abs() <= h).all()) and float((x[0] - x[:1].to(torch.bfloat16).double()).abs()) == 2.0 ** -8
    assert bool((h >= 2.0 ** -9 * x).all()) and bool((h <= 2.0 ** -8 * x).all())


def test_lse2_tol_is_what_it_was():
    g = torch.Generator().manual_seed(0)
    w = torch.softmax(2 * torch.randn(5, 300, generator=g, dtype=torch.float64), -1)
    lse = torch.randn(5, generator=g, dtype=torch.float64) * 10
    want = T.LOG2E * torch.minimum(6.0 * T.RND / math.sqrt(3.0) * (w * w).sum(-1).sqrt(), torch.full((5,), 1.02 * T.RND, dtype=torch.float64)) + 3e-4 + 2e-5 * lse.abs()
    assert torch.equal(T.lse2_tol(w, lse), want)
