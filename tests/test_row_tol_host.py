"""tests/row_tol.py on the CPU: on every input family of tests/test_gpu_step_kernels.py and tests/test_gpu_row_kernels.py, at its shapes, the float32 restatement of each kernel stays inside
the bound around the fp64 reference -- and `judge` REJECTS deliberately wrong restatements, which is how a reader checks that the device tests can fail.
No mutated kernel is ever built.  `-s` prints, per kernel and family, the largest error of the restatement over its bound."""
import numpy as np
import pytest
import torch

import row_tol as R
from row_tol import bhs

ROPES = [None, "contract", "arbitrary"]
EPS = [1e-6, 1e-5]


def _fwd(c, text_len, eps, mode, wrong=None):
    q, k = bhs(c["qkv"], 0), bhs(c["qkv"], 1)
    args = (q, k, c["wq"], c["bq"], c["wk"], c["bk"], c["cos"], c["sin"], text_len, eps, R.QK_SCALE, mode)
    ref = R.qknorm_rope_ref64(*args)
    got = R.qknorm_rope_fwd_f32(*args, wrong=wrong)
    tols = (R.qknorm_fwd_tol(q, c["wq"], c["bq"], ref[0], c["cos"], c["sin"], eps, R.QK_SCALE),
            R.qknorm_fwd_tol(k, c["wk"], c["bk"], ref[1], c["cos"], c["sin"], eps, 1.0))
    return got, ref, tols


def _bwd(c, text_len, eps, mode, wrong=None):
    q, k = bhs(c["qkv"], 0), bhs(c["qkv"], 1)
    args = (c["dq"], c["dk"], q, k, c["wq"], c["wk"], c["cos"], c["sin"], text_len, eps, mode)
    ref = R.qknorm_rope_grad64(*args)
    got = R.qknorm_rope_bwd_f32(*args, wrong=wrong)
    tols = (R.qknorm_bwd_tol(c["dq"], q, c["wq"], ref[0], c["cos"], c["sin"], text_len, eps, mode),
            R.qknorm_bwd_tol(c["dk"], k, c["wk"], ref[1], c["cos"], c["sin"], text_len, eps, mode))
    return got, ref, tols


def _problems(name, got, ref, tols):
    return [m for i, n in enumerate("qk") for m in R.judge(f"{name} {n}", got[i], ref[i], tols[i])]


@pytest.mark.parametrize("shape", R.QK_SHAPES)
@pytest.mark.parametrize("rope", ROPES)
@pytest.mark.parametrize("mode", [0, 1])
def test_qknorm_restatement_inside_bounds(mode, rope, shape):
    B, S, H, Lt = shape
    c = R.qknorm_inputs(B, S, H, Lt, rope, mode)
    for eps in EPS:
        for name, (got, ref, tols) in (("fwd", _fwd(c, Lt, eps, mode)), ("bwd", _bwd(c, Lt, eps, mode))):
            print(f"qknorm {name} mode {mode} rope {rope} {shape} eps {eps}: restatement / bound q {R.worst(got[0], ref[0], tols[0])[0]:.3f} "
                  f"k {R.worst(got[1], ref[1], tols[1])[0]:.3f}")
            assert not _problems(name, got, ref, tols)


def test_qknorm_planted_vectors_behave_as_described():
    """zero variance: output = bias (q: times q_scale) whatever eps is; the near-constant vector is where the two eps values differ by a factor"""
    B, S, H, Lt = 1, 7, 3, 3
    c = R.qknorm_inputs(B, S, H, Lt, None, 0)
    (q6, k6), (q5, k5) = (R.qknorm_rope_ref64(bhs(c["qkv"], 0), bhs(c["qkv"], 1), c["wq"], c["bq"], c["wk"], c["bk"], None, None, Lt, e, 1.0, 0) for e in EPS)
    assert torch.allclose(q6[0, 0, 0], c["bq"].double(), atol=1e-12) and torch.allclose(k5[0, H - 1, S - 1], c["bk"].double(), atol=1e-12)
    near6, near5 = q6[B - 1, H - 1, S - 1, 9] - c["bq"][9], q5[B - 1, H - 1, S - 1, 9] - c["bq"][9]
    assert 2.0 < float(near6 / near5) < 2.6          # rstd 718 against 302


WRONG_FWD = [  # (variant, rope_mode, table kind, shape)
    ("eps", 0, None, (1, 7, 3, 3)),
    ("row_s", 0, "contract", (1, 7, 3, 3)),
    ("row_s", 1, "contract", (3, 5, 5, 2)),
    ("skip_first", 0, "contract", (1, 64, 2, 1)),
    ("skip_first", 1, "contract", (1, 7, 3, 3)),
    ("sign1", 1, "contract", (2, 33, 2, 0)),
    ("round_q", 0, None, (2, 33, 2, 0)),
]


@pytest.mark.parametrize("wrong,mode,rope,shape", WRONG_FWD)
def test_judge_rejects_wrong_qknorm_forward(wrong, mode, rope, shape):
    """eps 1e-5 where 1e-6 was asked; the table row taken at s instead of s - text_len; the token at s == text_len left unrotated; mode 1 without the sign flip
    of the upper half; q rounded to bf16 before the q_scale multiply"""
    B, S, H, Lt = shape
    c = R.qknorm_inputs(B, S, H, Lt, rope, mode)
    assert not _problems("fwd", *_fwd(c, Lt, 1e-6, mode))
    bad = _problems("fwd", *_fwd(c, Lt, 1e-6, mode, wrong=wrong))
    print(*bad[:3], sep="\n")
    assert bad
    if wrong == "round_q":
        assert all(m.startswith("fwd q") for m in bad)             # k is not scaled


@pytest.mark.parametrize("wrong,mode", [("sp_j", 0), ("own_sin", 1)])
def test_judge_rejects_wrong_qknorm_backward(wrong, mode):
    """mode 0 with sp[j] in place of sp[j+1]; mode 1 with the sin read at the own lane instead of the partner's.  Both are invisible with the models' tables
    (pair-repeated, resp. equal across the pair): the arbitrary tables are what catches them."""
    B, S, H, Lt = 3, 5, 5, 2
    c = R.qknorm_inputs(B, S, H, Lt, "arbitrary", mode)
    assert not _problems("bwd", *_bwd(c, Lt, 1e-6, mode))
    bad = _problems("bwd", *_bwd(c, Lt, 1e-6, mode, wrong=wrong))
    print(*bad[:3], sep="\n")
    assert bad
    c = R.qknorm_inputs(B, S, H, Lt, "contract", mode)
    assert not _problems("bwd", *_bwd(c, Lt, 1e-6, mode, wrong=wrong))          # ... which is why the device test also runs arbitrary tables


# ------------------------------------------------------------------------------------------ gelu
@pytest.mark.parametrize("n", [8, 8 * 4200])
def test_gelu_restatement_inside_bounds_and_missing_cubic_term_rejected(n):
    u, dy = R.gelu_inputs(n)
    val, der = R.gelu_ref64(u, dy)
    tv, td = R.gelu_fwd_tol(u, val), R.gelu_bwd_tol(u, dy, der)
    got_v, got_d = R.gelu_fwd_f32(u), R.gelu_bwd_f32(u, dy)
    print(f"gelu n {n}: restatement / bound value {R.worst(got_v, val, tv)[0]:.3f} derivative {R.worst(got_d, der, td)[0]:.3f}")
    assert not R.judge("gelu", got_v, val, tv) and not R.judge("dgelu", got_d, der, td)
    bad = R.judge("dgelu", R.gelu_bwd_f32(u, dy, wrong="no_cubic"), der, td)          # without the 0.2140644488 x^2 term
    assert bad or n == 8
    ref_t = torch.nn.functional.gelu(u.double(), approximate="tanh")                    # the reference is torch's function, without its cancellation
    assert float((val - ref_t).abs().max()) < 1e-14


def test_gelu_bound_is_not_the_old_absolute_one():
    """0.04 absolute let every small output through; per element the bound is the bf16 half ulp of the result: a result replaced by its neighbour in bf16 fails"""
    u, dy = R.gelu_inputs(8 * 4200)
    val, _ = R.gelu_ref64(u)
    got = torch.as_tensor(R.gelu_fwd_f32(u)).to(torch.bfloat16)
    nxt = (got.view(torch.int16) + 1).view(torch.bfloat16)
    assert len(R.judge("gelu", nxt, val, R.gelu_fwd_tol(u, val))) > 1
    small = val.abs() < 4
    assert float((nxt.double() - val)[small].abs().max()) < 0.04


# ------------------------------------------------------------------------------------------ DPO error means
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,vec_ok", [(524288 + 2400, True), (524288 + 2405, False), (524288 + 2405, True), (1248, False)])
def test_dpo_errs_restatement_inside_bound_and_dropped_tail_rejected(N, vec_ok, dtype):
    ins = R.dpo_inputs(2, N, dtype)
    ref = R.dpo_errs_ref64(*ins)
    rel = R.dpo_errs_rel(N, vec_ok)
    got = R.dpo_errs_f32(*ins, vec_ok=vec_ok)
    print(f"dpo errs N {N} vec_ok {vec_ok} {dtype}: adds per thread {R.dpo_adds_per_thread(N, vec_ok)}, bound {rel:.2e} rel, restatement / bound "
          f"{R.worst(got, ref, rel * ref)[0]:.3f}")
    assert not R.judge("errs", got, ref, rel * ref)
    bad = R.judge("errs", R.dpo_errs_f32(*ins, vec_ok=vec_ok, wrong="drop5"), ref, rel * ref)      # a reduction that drops the last 5 elements
    assert bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dpo_cases_share_a_prefix_and_the_last_five_elements_outweigh_the_bound(dtype):
    """what the device test's comparison of its cases with one another rests on"""
    a, b = R.dpo_inputs(2, 524288 + 2400, dtype), R.dpo_inputs(2, 524288 + 2405, dtype)
    assert all(torch.equal(x, y[:, :524288 + 2400]) for x, y in zip(a, b))
    sa, sb = R.dpo_errs_ref64(*a) * (524288 + 2400), R.dpo_errs_ref64(*b) * (524288 + 2405)
    bound = max(R.dpo_errs_rel(524288 + 2400), R.dpo_errs_rel(524288 + 2405), R.dpo_errs_rel(524288 + 2405, False)) * float(sb.max())
    print(f"last five elements: {float((sb - sa).min()):.1f} .. {float((sb - sa).max()):.1f}, bound on a sum {bound:.2f}")
    assert float((sb - sa).min()) > 10 * bound


def test_adamw_cases_have_the_norms_they_are_meant_to_have():
    for n in (2097152 + 203, 5):
        g = R.adamw_state(n)[1]
        assert R.grad_norm_ref64(3.0 * g, 0.5) > 2.0 and R.grad_norm_ref64(1e-4 * g, 1.0) < 0.5


def test_dpo_adds_per_thread_counts_the_kernel_loops():
    assert R.dpo_adds_per_thread(1248) == 8 and R.dpo_adds_per_thread(44928) == 8           # the suite's earlier shapes: one chunk per thread
    assert R.dpo_adds_per_thread(524288 + 2400) == 16                                        # the vector loop strides
    assert R.dpo_adds_per_thread(524288 + 2405) == 17                                        # ... plus one element of the scalar tail
    assert R.dpo_adds_per_thread(524288 + 2405, vec_ok=False) == 9                           # the scalar loop strides: 8.04 elements per thread
    assert R.dpo_adds_per_thread(1248, vec_ok=False) == 5


# ------------------------------------------------------------------------------------------ AdamW, gradient norm
HYP = R.ADAMW_HYPER


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("gscale,grad_scale,max_norm", R.ADAMW_COMBOS)
@pytest.mark.parametrize("n", [2097152 + 203, 5])
def test_adamw_restatement_inside_bounds(n, gscale, grad_scale, max_norm, wd):
    p, g, m, v, z = R.adamw_state(n)
    g = g * gscale
    tn = None if max_norm == 0 else R.grad_norm_f32(g, grad_scale)
    if tn is not None:
        ref_n = R.grad_norm_ref64(g, grad_scale)
        print(f"grad_norm n {n}: bound {R.grad_norm_rel(n):.2e} rel, restatement {abs(float(tn) - ref_n) / ref_n:.2e}")
        assert abs(float(tn) - ref_n) <= R.grad_norm_rel(n) * ref_n
        assert (ref_n > 1.0) == (gscale == 3.0) or n == 5
    for step in (1, 2, 1000):
        kw = dict(HYP, weight_decay=wd, step=step, grad_scale=grad_scale, max_norm=max_norm, total_norm=tn)
        ref = R.adamw_ref64(p, g, m, v, **kw)
        tols = R.adamw_tols(g, m, v, ref[1], ref[2], ref[0], HYP["beta1"], HYP["beta2"], grad_scale, max_norm, tn)
        got = R.adamw_f32(p, g, m, v, **kw)
        for name, a, r, t in zip(("param", "exp_avg", "exp_avg_sq"), got, ref, tols):
            print(f"adamw n {n} std {gscale} wd {wd} step {step} {name}: restatement / bound {R.worst(a, r, t)[0]:.3f}")
            assert not R.judge(f"{name} step {step}", a, r, t)
        assert torch.equal(torch.as_tensor(got[0][z]), torch.as_tensor(R.f32(p)[z] * (np.float32(1) - np.float32(0.1) * np.float32(wd))))   # zero gradient: only the decay
        p, m, v = (torch.as_tensor(a) for a in got)


@pytest.mark.parametrize("wrong,wd", [("decay_after", 0.01), ("no_bc2", 0.0), ("no_bc2", 0.01)])
def test_judge_rejects_wrong_adamw(wrong, wd):
    """weight decay applied after the moment update; bc2_sqrt not applied"""
    p, g, m, v, _ = R.adamw_state(4099)
    for step in (1, 2, 1000):
        kw = dict(HYP, weight_decay=wd, step=step)
        ref = R.adamw_ref64(p, g, m, v, **kw)
        tol_p = R.adamw_tols(g, m, v, ref[1], ref[2], ref[0], HYP["beta1"], HYP["beta2"])[0]
        assert not R.judge("param", R.adamw_f32(p, g, m, v, **kw)[0], ref[0], tol_p)
        assert R.judge("param", R.adamw_f32(p, g, m, v, wrong=wrong, **kw)[0], ref[0], tol_p), step


def test_judge_reports_where_and_treats_nan_as_outside():
    ref = torch.zeros(2, 3, dtype=torch.float64)
    got = ref.clone()
    got[1, 2] = float("nan")
    got[0, 1] = 1.0
    msgs = R.judge("x", got, ref, torch.full_like(ref, 0.5))
    assert msgs[0].startswith("x: 2 of 6") and any("x[1, 2]" in m for m in msgs) and any("x[0, 1]: got 1, want 0, bound 0.5" in m for m in msgs)
    assert R.judge("x", ref, ref, 0.0) == []


# ------------------------------------------------------------------------------------------ one-wave-per-row norm kernels
def _ratio(got, ref, tol):
    return R.worst(got, ref, tol)[0]


def _cog_tabs(c, B, S, Lt, mod, wrong=None):
    if not mod:
        return None, None
    m = c["mod"]
    return R.cog_rows(m[:, 1], m[:, 3], B, S, Lt, wrong), R.cog_rows(m[:, 0], m[:, 2], B, S, Lt, wrong)


def _cog_fwd(c, B, S, Lt, mod, with_y, eps=1e-5, wrong=None):
    """-> problems, worst ratios (n, mean, rstd), xn, restatement's mean / rstd"""
    xn = R.cog_x_new(c, B, S, Lt) if with_y else c["x"]
    s1p, shift = _cog_tabs(c, B, S, Lt, mod)
    ref = R.cog_ln_fwd_ref64(xn, c["w"], c["b"], s1p, shift, eps)
    tols = R.cog_ln_fwd_tol(xn, c["w"], c["b"], s1p, shift, eps, ref[0])
    got = R.cog_ln_fwd_f32(xn, c["w"], c["b"], *_cog_tabs(c, B, S, Lt, mod, wrong), eps, wrong)
    bad = [m for i, n in enumerate(("n", "mean", "rstd")) for m in R.judge(f"cog fwd {n}", got[i], ref[i], tols[i])]
    return bad, [_ratio(got[i], ref[i], tols[i]) for i in range(3)], xn, got[1], got[2]


def _cog_bwd(c, B, S, Lt, mod, xn, mean, rstd, dres, wrong=None):
    s1p, _ = _cog_tabs(c, B, S, Lt, mod)
    alpha = c["w"].double() if s1p is None else c["w"].double() * s1p.double()
    g = c["dn"].double() * alpha
    ref = R.ln_bwd_ref64(g, xn, mean, rstd, dres)
    tol = R.bf16_tol(ref, R.ln_bwd_rest(g, xn, mean, rstd, 2.0 if mod else 0.0, dres))
    got = R.cog_ln_bwd_f32(c["dn"], xn, mean, rstd, c["w"], s1p, dres, wrong)
    return R.judge("cog bwd dx", got, ref, tol), _ratio(got, ref, tol)


@pytest.mark.parametrize("D", R.ROW_WIDTHS)
def test_cog_ln_restatements_inside_bounds(D):
    worst = np.zeros(4)
    for B, S, Lt in R.cog_layouts(D):
        c = R.cog_case(B, S, Lt, D)
        for mod in (True, False):
            for with_y in (True, False):
                bad, r, xn, mean, rstd = _cog_fwd(c, B, S, Lt, mod, with_y)
                assert not bad, bad
                worst[:3] = np.maximum(worst[:3], r)
            for dres in (c["dres"], None):
                bad, r = _cog_bwd(c, B, S, Lt, mod, xn, mean, rstd, dres)
                assert not bad, bad
                worst[3] = max(worst[3], r)
    print(f"cog LN D {D}: restatement / bound n {worst[0]:.3f} mean {worst[1]:.3f} rstd {worst[2]:.3f} dx {worst[3]:.3f}")


def _wan_forms():
    """(x dtype, affine, modulation, round_xhat, bf16 result): every combination the forward entry accepts without y"""
    for xdt in (torch.float32, torch.bfloat16):
        for affine in (False, True):
            for mod in (False, True):
                for rnd in (0, 1):
                    yield xdt, affine, mod, rnd, True
    yield torch.float32, False, True, 0, False
    yield torch.float32, False, False, 0, False


def _wan_fwd(c, affine, mod, rnd, out_bf16, x=None, eps=1e-6, wrong=None):
    x = c["x"] if x is None else x
    a = (x, c["gid"] if mod else None, c["w"] if affine else None, c["b"] if affine else None, c["tab"][:, 3] if mod else None, c["tab"][:, 4] if mod else None, eps)
    ref = R.wan_ln_fwd_ref64(*a)
    tols = R.wan_ln_fwd_tol(*a, rnd, ref[0], out_bf16)
    got = R.wan_ln_fwd_f32(*a, rnd, out_bf16, wrong)
    bad = [m for i, n in enumerate(("out", "mean", "rstd")) for m in R.judge(f"wan fwd {n}", got[i], ref[i], tols[i])]
    return bad, max(_ratio(got[i], ref[i], tols[i]) for i in range(3)), got[1], got[2]


def _wan_bwd(c, affine, mod, mean, rstd, dy, dres, wrong=None):
    gid, w, scale = c["gid"] if mod else None, c["w"] if affine else None, c["tab"][:, 4] if mod else None
    g, cg = R.wan_ln_bwd_g64(dy, gid, w, scale)
    ref = R.ln_bwd_ref64(g, c["x"], mean, rstd, dres)
    tol = R.ln_bwd_rest(g, c["x"], mean, rstd, cg, dres)
    got = R.wan_ln_bwd_f32(dy, c["x"], mean, rstd, gid, w, scale, dres, wrong)
    return R.judge("wan bwd dx", got, ref, tol), _ratio(got, ref, tol)


@pytest.mark.parametrize("D", R.WAN_LN_WIDTHS)
def test_wan_ln_restatements_inside_bounds(D):
    wf = wb = 0.0
    for rows in R.WAN_LN_ROWS:
        for xdt, affine, mod, rnd, out_bf16 in _wan_forms():
            c = R.wan_ln_case(rows, D, xdt)
            bad, r, mean, rstd = _wan_fwd(c, affine, mod, rnd, out_bf16)
            assert not bad, (rows, xdt, affine, mod, rnd, out_bf16, bad)
            wf = max(wf, r)
            if rnd:
                continue
            fp32_dy = not out_bf16
            for dres in ((None,) if fp32_dy else (c["dres"], None)):
                bad, r = _wan_bwd(c, affine, mod, mean, rstd, c["dy32"] if fp32_dy else c["dy"], dres)
                assert not bad, (rows, xdt, affine, mod, bad)
                wb = max(wb, r)
    print(f"wan LN D {D}: restatement / bound forward {wf:.3f} backward {wb:.3f}")


def _rms(c, D, hd, tables, eps=1e-6, wrong_f=None, wrong_b=None):
    cos, sin = (c["cos"], c["sin"]) if tables else (None, None)
    ref, rs_ref = R.rms_rope_ref64(c["u"], c["w"], cos, sin, R.RMS_L, hd, eps)
    tol, tol_rs = R.rms_rope_fwd_tol(c["u"], c["w"], cos, sin, R.RMS_L, hd, eps, ref)
    got, rs = R.rms_rope_fwd_f32(c["u"], c["w"], cos, sin, R.RMS_L, hd, eps, wrong_f)
    rs_ok, _ = R.rms_rope_fwd_f32(c["u"], c["w"], cos, sin, R.RMS_L, hd, eps)[1], None
    bad_f = R.judge("rms fwd out", got, ref, tol) + R.judge("rms fwd rs", rs, rs_ref, tol_rs)
    gref = R.rms_rope_bwd_ref64(c["dout"], c["u"], rs_ok, c["w"], cos, sin, R.RMS_L, hd)
    gtol = R.rms_rope_bwd_tol(c["dout"], c["u"], rs_ok, c["w"], cos, sin, R.RMS_L, hd, gref)
    ggot = R.rms_rope_bwd_f32(c["dout"], c["u"], rs_ok, c["w"], cos, sin, R.RMS_L, hd, wrong_b)
    return bad_f, R.judge("rms bwd du", ggot, gref, gtol), (_ratio(got, ref, tol), _ratio(rs, rs_ref, tol_rs), _ratio(ggot, gref, gtol))


@pytest.mark.parametrize("D,hd", R.RMS_SHAPES)
@pytest.mark.parametrize("tables", [True, False])
def test_rms_rope_restatements_inside_bounds(tables, D, hd):
    bad_f, bad_b, r = _rms(R.rms_case(D, hd), D, hd, tables)
    print(f"rms_rope D {D} head_dim {hd} tables {tables}: restatement / bound out {r[0]:.3f} rstd {r[1]:.3f} du {r[2]:.3f}")
    assert not bad_f and not bad_b, (bad_f, bad_b)


@pytest.mark.parametrize("rows,D", [(5, 264), (9, 4096)])
def test_wan_gate_restatement_inside_bound_and_neighbour_gid_rejected(rows, D):
    c = R.wan_ln_case(rows, D)
    ref, tol = R.wan_gate_ref64(c["x"], c["y"], c["gid"], c["tab"][:, 2])
    assert not R.judge("gate", R.wan_gate_f32(c["x"], c["y"], c["gid"], c["tab"][:, 2]), ref, tol)
    assert R.judge("gate", R.wan_gate_f32(c["x"], c["y"], c["gid"], c["tab"][:, 2], wrong="gid_neighbour"), ref, tol)


# the widths at which the variant differs from the kernel: "div_nv" only where the last chunk is partly filled
@pytest.mark.parametrize("wrong,D", [("mask8", 8), ("mask8", 520), ("mask8", 3080), ("mask8", 4096), ("div_nv", 8), ("div_nv", 520), ("div_nv", 1288),
                                     ("div_nv", 3080), ("div_nv", 4088), ("text_first_video", 512), ("text_first_video", 4088)])
def test_judge_rejects_wrong_cog_ln_forward(wrong, D):
    """the last valid group of eight columns outside the sums; division by 512 NV; the text range's modulation on the first video row"""
    B, S, Lt = R.COG_LAYOUTS[0]
    c = R.cog_case(B, S, Lt, D)
    assert not _cog_fwd(c, B, S, Lt, True, True)[0]
    bad = _cog_fwd(c, B, S, Lt, True, True, wrong=wrong)[0]
    print(*bad[:3], sep="\n")
    assert bad


@pytest.mark.parametrize("wrong,D", [("no_c1", 8), ("no_c1", 520), ("no_c1", 4096), ("mask8", 520), ("mask8", 4096), ("div_nv", 520), ("div_nv", 4088)])
def test_judge_rejects_wrong_cog_ln_backward(wrong, D):
    """c1 dropped; the last group of eight outside c1 and c2; division by 512 NV"""
    B, S, Lt = R.COG_LAYOUTS[0]
    c = R.cog_case(B, S, Lt, D)
    _, _, xn, mean, rstd = _cog_fwd(c, B, S, Lt, True, True)
    for dres in (c["dres"], None):
        assert not _cog_bwd(c, B, S, Lt, True, xn, mean, rstd, dres)[0]
        bad = _cog_bwd(c, B, S, Lt, True, xn, mean, rstd, dres, wrong=wrong)[0]
        print(*bad[:2], sep="\n")
        assert bad


@pytest.mark.parametrize("wrong,D", [("mask8", 264), ("mask8", 4096), ("div_nv", 264), ("div_nv", 4088), ("gid_neighbour", 8), ("gid_neighbour", 3072)])
def test_judge_rejects_wrong_wan_ln_forward(wrong, D):
    for xdt in (torch.float32, torch.bfloat16):
        c = R.wan_ln_case(9, D, xdt)
        assert not _wan_fwd(c, True, True, 0, True)[0]
        bad = _wan_fwd(c, True, True, 0, True, wrong=wrong)[0]
        print(*bad[:2], sep="\n")
        assert bad


@pytest.mark.parametrize("wrong,D", [("scale_no1p", 8), ("scale_no1p", 4088), ("no_c1", 264), ("no_c1", 4096), ("mask8", 520), ("gid_neighbour", 264)])
def test_judge_rejects_wrong_wan_ln_backward(wrong, D):
    """scale where 1 + scale belongs; c1 dropped; the last group outside the sums; a neighbour's group"""
    c = R.wan_ln_case(9, D)
    _, _, mean, rstd = _wan_fwd(c, True, True, 0, True)
    for dres in (c["dres"], None):
        assert not _wan_bwd(c, True, True, mean, rstd, c["dy"], dres)[0]
        assert _wan_bwd(c, True, True, mean, rstd, c["dy"], dres, wrong=wrong)[0]


def test_bf16_output_bound_cannot_see_a_missing_xhat_rounding():
    """why the device test also compares round_xhat bit for bit with bf16((x - mean) rstd) from the device's own mean and rstd: without the intermediate rounding the
    output stays inside the bound (the reference is the unrounded expression and the rounding's half ulp is part of the tolerance)"""
    c = R.wan_ln_case(9, 520)
    assert not _wan_fwd(c, True, True, 1, True, wrong="no_round")[0]
    a = (c["x"], None, None, None, None, None, 1e-6)
    with_r, without = R.wan_ln_fwd_f32(*a, 1)[0], R.wan_ln_fwd_f32(*a, 1, wrong="no_round")[0]
    assert np.array_equal(with_r, without)                 # and with nothing behind it the second rounding changes nothing: the bit-exact case has no affine ...
    mean, rstd = R.wan_ln_fwd_f32(*a, 0)[1:]
    assert np.array_equal(with_r, R.bf16_round((R.f32(c["x"]) - mean[:, None]) * rstd[:, None]))       # ... and is the two-operation fp32 expression


@pytest.mark.parametrize("wrong,D,hd", [("mask8", 264, 24), ("mask8", 4096, 128), ("div_nv", 264, 8), ("div_nv", 520, 40), ("per_head", 264, 24),
                                        ("per_head", 3072, 128), ("row_no_mod", 264, 8), ("row_no_mod", 4096, 128)])
def test_judge_rejects_wrong_rms_rope_forward(wrong, D, hd):
    """the last group outside the sum of squares; division by 512 NV; the mean of squares per head; table row `row` where `row % L` belongs"""
    c = R.rms_case(D, hd)
    assert not _rms(c, D, hd, True)[0]
    bad = _rms(c, D, hd, True, wrong_f=wrong)[0]
    print(*bad[:2], sep="\n")
    assert bad


@pytest.mark.parametrize("wrong,D,hd", [("no_transpose", 264, 24), ("no_transpose", 4096, 128), ("row_no_mod", 520, 40), ("mask8", 264, 8), ("div_nv", 520, 40)])
def test_judge_rejects_wrong_rms_rope_backward(wrong, D, hd):
    """the forward's rotation applied to the gradient; `row` for `row % L`; the last group outside mean(dn n); division by 512 NV"""
    c = R.rms_case(D, hd)
    assert not _rms(c, D, hd, True)[1]
    assert _rms(c, D, hd, True, wrong_b=wrong)[1]


def test_ln_bounds_are_not_the_old_absolute_ones():
    """tests/test_gpu_kernels.py::test_ln_modulate_fwd_bwd allowed 0.03 absolute on the output and 2 % of the largest gradient + 1e-3: on that test's own inputs
    (D = 3072, B = 2, S = 37, text_len = 5, randn) a LayerNorm whose sums leave out the last eight columns passes the first, and a backward without c1 passes the second.
    Per element both are rejected."""
    D, B, S, Lt = 3072, 2, 37, 5
    g = torch.Generator().manual_seed(D)
    x = torch.randn(B, S, D, generator=g).to(torch.bfloat16)
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    mod = 0.3 * torch.randn(B, 4, D, generator=g)
    mod[:, 1] += 1
    mod[:, 3] += 1
    dy = torch.randn(B, S, D, generator=g).to(torch.bfloat16)
    s1p, shift = R.cog_rows(mod[:, 1], mod[:, 3], B, S, Lt), R.cog_rows(mod[:, 0], mod[:, 2], B, S, Lt)
    ref = R.cog_ln_fwd_ref64(x, w, b, s1p, shift, 1e-5)
    tols = R.cog_ln_fwd_tol(x, w, b, s1p, shift, 1e-5, ref[0])
    ok, bad = R.cog_ln_fwd_f32(x, w, b, s1p, shift, 1e-5), R.cog_ln_fwd_f32(x, w, b, s1p, shift, 1e-5, wrong="mask8")
    assert float((torch.as_tensor(bad[0]).double() - ref[0]).abs().max()) < 0.03                   # the old assertion accepts it
    assert not R.judge("n", ok[0], ref[0], tols[0]) and R.judge("n", bad[0], ref[0], tols[0]) and R.judge("mean", bad[1], ref[1], tols[1])
    gg = dy.double() * w.double() * s1p.double()
    gref = R.ln_bwd_ref64(gg, x, ok[1], ok[2])
    gtol = R.bf16_tol(gref, R.ln_bwd_rest(gg, x, ok[1], ok[2], 2.0))
    gok, gbad = R.cog_ln_bwd_f32(dy, x, ok[1], ok[2], w, s1p), R.cog_ln_bwd_f32(dy, x, ok[1], ok[2], w, s1p, wrong="no_c1")
    assert float((torch.as_tensor(gbad).double() - gref).abs().max()) < 0.02 * float(gref.abs().max()) + 1e-3       # the old assertion accepts it
    assert not R.judge("dx", gok, gref, gtol) and len(R.judge("dx", gbad, gref, gtol)) > 1


def test_row_sum_constants_count_the_kernel_loops():
    assert [R.nv_of(D) for D in R.ROW_WIDTHS] == [1, 1, 2, 2, 3, 4, 5, 6, 7, 8, 8]
    assert R.c_sum(64 * 8) == 7 + 6 and R.c_mean(4096) == 70 and R.c_rstd(512) == 11 and R.c_rms(4096) == 38
