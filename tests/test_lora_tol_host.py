"""tests/lora_tol.py on the CPU: on every case of tests/test_gpu_lora_kernels.py the float32 restatement of each LoRA kernel stays inside its per-element bound
around the fp64 reference (and equals the int64 result on integer data) -- and deliberately wrong restatements are REJECTED, by the bound on random data or by
equality on integer data, which is how a reader checks that the device tests can fail.  Two tests show wrong variants PASSING the former assertions of
test_gpu_kernels.py::test_lora_kernels_raw (2 % / 0.2 % of the largest element): the gap the per-element bounds close.  No mutated kernel is ever built.
`-s` prints, per family, the largest error of the restatement over its bound."""
import numpy as np
import pytest
import torch

import lora_tol as L


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def _equal(got, ref):
    """bit-for-bit on integer data: NaN (not written) is unequal"""
    return bool(torch.equal(_t(got), ref.double()))


# ------------------------------------------------------------------------------------------ down
def _down(M, K, R, kind, wrong=None):
    x, a = L.down_inputs(M, K, R, kind)
    ref, S = L.down_ref64(x, a)
    return L.down_f32(x, a, wrong), ref, L.down_tol(ref, S, K)


def _down_live(wrong, M, K, R, kind):
    """does the variant change anything the checks of this kind of data can see?  acc_bf16: integers <= 256 are bf16 values, and with one chunk (K = 64) the extra rounding
    IS the store; on random data its double rounding passes the bound on most elements, so a case counts from 1000 elements on.  no_tail_cols: R % 4"""
    if wrong == "acc_bf16":
        return kind != "exact" and K > 64 and M * R >= 1000
    if wrong == "no_tail_cols":
        return R % 4 != 0
    return True


@pytest.mark.parametrize("group", L.DOWN_GROUPS)
def test_down_restatement_inside_bounds_and_wrong_variants_rejected(group):
    worst, rejected = 0.0, {w: 0 for w in L.DOWN_WRONG}
    for M, K, R, _, kinds in L.down_cases(group):
        for kind in kinds:
            got, ref, tol = _down(M, K, R, kind)
            if kind == "exact":
                assert _equal(got, ref), (M, K, R)
            else:
                worst = max(worst, L.worst(got, ref, tol)[0])
            assert not L.judge(f"down {(M, K, R, kind)}", got, ref, tol)
            for w in L.DOWN_WRONG:
                if not _down_live(w, M, K, R, kind):
                    continue
                bad, _, _ = _down(M, K, R, kind, w)
                assert (not _equal(bad, ref)) if kind == "exact" else L.judge("down", bad, ref, tol), f"{w} passes at {(M, K, R, kind)}"
                rejected[w] += 1
    print(f"down {group}: restatement / bound {worst:.3f}; rejected {rejected}")
    assert all(rejected[w] for w in L.DOWN_WRONG if w != "no_tail_cols" or group == "tail")


def test_old_assertion_passes_drop_one_term_at_K3072_which_the_bound_rejects():
    """the gap: one k-term of one row of X lost at K = 3072 (64 elements of T off by |x a|, x nearest 1) stays inside `0.02 max|ref| + 1e-3`"""
    M, K, R = 200, 3072, 64
    bad, ref, tol = _down(M, K, R, "randn", "drop_one_term")
    err, old = float((_t(bad) - ref).abs().max()), 0.02 * float(ref.abs().max()) + 1e-3
    print(f"down K 3072 drop_one_term: max err {err:.4f}, old tolerance {old:.4f}, over the new bound by {L.worst(bad, ref, tol)[0]:.1f}x")
    assert err < old
    assert L.judge("down", bad, ref, tol)
    bad, ref, tol = _down(M, K, R, "randn", "acc_bf16")                    # 48 roundings of the accumulator to bf16: the old assertion passes that too
    assert float((_t(bad) - ref).abs().max()) < old and L.judge("down", bad, ref, tol)


# ------------------------------------------------------------------------------------------ up_add
def _up(M, N, rp, s, acc, kind, wrong=None):
    t, b, y = L.up_inputs(M, N, rp, kind)
    s = L.up_scale(s, kind)
    y = y if acc else None
    ref, dot, S = L.up_ref64(y, t, b, s)
    return L.up_f32(y, t, b, s, wrong), ref, L.up_tol(ref, dot, S, s, rp, acc)


def _up_live(wrong, M, N, rp, acc, kind):
    """the three variants of the add need accumulate; the two double roundings are exact on integers and pass the bound on most random elements (1000 elements on);
    acc_bf16 without accumulate, or at rp <= 64 (one chunk) with s a power of two, is the store itself"""
    if wrong in ("up_double_round", "up_scale_after", "no_accumulate") and not acc:
        return False
    if wrong in ("up_double_round", "acc_bf16"):
        return kind != "exact" and M * N >= 1000 and (wrong == "up_double_round" or acc)
    return True


def test_up_add_restatement_inside_bounds_and_wrong_variants_rejected():
    worst, rejected = 0.0, {w: 0 for w in L.UP_WRONG}
    for M, N, rp, s, acc in L.up_cases():
        for kind in ("exact", "randn", "mean"):
            got, ref, tol = _up(M, N, rp, s, acc, kind)
            if kind == "exact":
                assert _equal(got, ref), (M, N, rp, s, acc)
            else:
                worst = max(worst, L.worst(got, ref, tol)[0])
            assert not L.judge(f"up_add {(M, N, rp, s, acc, kind)}", got, ref, tol)
            for w in L.UP_WRONG:
                if not _up_live(w, M, N, rp, acc, kind):
                    continue
                bad, _, _ = _up(M, N, rp, s, acc, kind, w)
                assert (not _equal(bad, ref)) if kind == "exact" else L.judge("up", bad, ref, tol), f"{w} passes at {(M, N, rp, s, acc, kind)}"
                rejected[w] += 1
    print(f"up_add: restatement / bound {worst:.3f}; rejected {rejected}")
    assert all(rejected.values())


# ------------------------------------------------------------------------------------------ grad
def _grad_live(wrong, M, P, Q, kind):
    p = L.grad_plan(M, P, Q)
    if wrong == "acc_bf16":                      # integers up to 256 are bf16 values: random data only, and more than one chunk of 64 rows
        return kind != "exact" and M > 64
    if wrong == "grad_split_overlap":            # the unrounded split must end inside a 64-row tile that the next split's rows fill
        return p["sp"] > 1 and L._cdiv(M, p["sp"]) % 64 != 0
    return True


@pytest.mark.parametrize("P,Q", L.GRAD_PQ)
def test_grad_restatement_inside_bounds_and_wrong_variants_rejected(P, Q):
    worst, rejected = 0.0, {w: 0 for w in L.GRAD_WRONG}
    for M in [c[0] for c in L.grad_cases() if c[1:] == (P, Q)]:
        for kind in ("exact", "randn") + (("mean",) if (P, Q) == (192, 320) else ()):
            u, v = L.grad_inputs(M, P, Q, kind)
            ref, S = L.grad_ref64(u, v, L.GRAD_S)
            got, tol = L.grad_f32(u, v, L.GRAD_S), L.grad_tol(ref, S, L.GRAD_S, M)
            if kind == "exact":
                assert _equal(got, ref), (M, P, Q)
            else:
                worst = max(worst, L.worst(got, ref, tol)[0])
            assert not L.judge(f"grad {(M, P, Q, kind)}", got, ref, tol)
            if L.grad_plan(M, P, Q)["splits"] > 1 and kind == "randn":  # with one split its end IS M; the row ranges do not depend on the data
                assert np.array_equal(got, L.grad_f32(u, v, L.GRAD_S, "grad_zfill_M")), "the zero-fill bound is live after all"
            if max(P, Q) > 320 and (M, kind) not in ((257, "exact"), (257, "randn"), (4810, "randn")):     # the wide shapes: where a second split and a short last split exist
                continue
            for w in L.GRAD_WRONG:
                if not _grad_live(w, M, P, Q, kind):
                    continue
                bad = L.grad_f32(u, v, L.GRAD_S, w)
                assert (not _equal(bad, ref)) if kind == "exact" else L.judge("grad", bad, ref, tol), f"{w} passes at {(M, P, Q, kind)}"
                rejected[w] += 1
    print(f"grad {(P, Q)}: restatement / bound {worst:.3f}; rejected {rejected}")
    assert all(rejected.values())


def test_grad_plan_reaches_its_three_regimes_with_short_last_splits():
    plans = {c: L.grad_plan(*c) for c in L.grad_cases()}
    assert {p["regime"] for p in plans.values()} == {"one", "rows", "target"}
    assert plans[(1300, 8, 8)] == dict(n_pt=1, n_qt=1, sp=6, rows=256, splits=6, regime="rows", last=20)
    assert plans[(5000, 3072, 64)]["splits"] == 16 == L.GRAD_WGS // 48 and plans[(5000, 3072, 64)]["regime"] == "target"
    assert plans[(4810, 3072, 64)]["splits"] == 16 and plans[(4810, 3072, 64)]["last"] == 10
    assert all(p["rows"] % 64 == 0 for p in plans.values())


def test_old_grad_assertion_passes_a_lost_product_and_grad_split_overlap_is_not_live_under_the_plan():
    """Passing M for the split's end to the zero fill (the `grad_split_overlap` mutation of the kernel) changes no bit under lora_grad_plan, whose rows_per_split is a
    multiple of the 64-row tile: no test can reject it.  Its live form (rows_per_split not rounded) IS rejected.  What `2e-3 max|ref| + 1e-4` lets through is smaller:
    one lost product of one element.  At M = 1000, P x Q = 64 x 3072 that tolerance is 0.15 and 46 % of the products of a row are below it; the bound (median 4e-3)
    rejects 97.7 % of them, all but the products that are nearly zero."""
    M, P, Q = 1000, 64, 3072                                               # the largest shape of test_lora_kernels_raw
    u, v = L.grad_inputs(M, P, Q, "randn")
    ref, S = L.grad_ref64(u, v, L.GRAD_S)
    tol = L.grad_tol(ref, S, L.GRAD_S, M)
    good = L.grad_f32(u, v, L.GRAD_S)
    assert np.array_equal(good, L.grad_f32(u, v, L.GRAD_S, "grad_zfill_M")) and not L.judge("grad", good, ref, tol)
    old = 2e-3 * float(ref.abs().max()) + 1e-4
    over = L.grad_f32(u, v, L.GRAD_S, "grad_split_overlap")
    assert L.judge("grad", over, ref, tol)
    lost = L.GRAD_S * torch.outer(u[M // 2].double(), v[M // 2].double())          # element (p, q) of this is what G[p, q] loses with the product of row M / 2
    err = (_t(good) - lost - ref).abs()
    old_passes, new_rejects = float((err < old).double().mean()), float((err > tol).double().mean())
    print(f"grad M 1000: one lost product of row {M // 2}: {100 * old_passes:.0f} % of the P Q choices pass the old tolerance {old:.3f}, the bound (median {float(tol.median()):.2e}) "
          f"rejects {100 * new_rejects:.1f} %; live overlap: err {float((_t(over) - ref).abs().max()):.2f}")
    assert old_passes > 0.25 and new_rejects > 0.95


# ------------------------------------------------------------------------------------------ refresh
@pytest.mark.parametrize("r,K,Dn,s", L.REFRESH_CASES)
def test_refresh_inputs_hold_values_on_which_the_two_roundings_differ(r, K, Dn, s):
    A, B, n = L.refresh_inputs(r, K, Dn, s)
    assert n >= min(Dn * r, 32)
    once = (B * s).to(torch.bfloat16)
    _, twice = L.refresh_ref(A, B, s)
    assert int((once != twice).sum()) >= n and bool((once.view(-1)[:n] != twice.view(-1)[:n]).all())
