"""tests/row_tol.py on the CPU: on every input family of tests/test_gpu_step_kernels.py, at its shapes, the float32 restatement of each kernel stays inside
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
