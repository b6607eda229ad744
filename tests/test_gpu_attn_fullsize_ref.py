"""The attention kernels at the FULL sequence lengths, element by element against fp64 (tests/attn_ref64.py) inside the derived per-element bounds and rms ratio of
tests/attn_tol.py -- launched at the real launch shapes (task scheduling, tail-round split, LDS-ring wrap, 112- / 48-row last strips, 48-key tile remainder are
bench.py's), with the reference held to a few heads:
    head_dim 64   B 2, H 48, S 17 776 (cfg2)   token-major views of one fused QKV buffer, int8 residual, forward + backward; N(0,1) and trained-like (gain 3) operands
    head_dim 64   H 6, S 41 026 (cfg4)         forward + backward
    head_dim 64   online-softmax entry at S 17 776 (fp32 row sums)
    head_dim 128  B 2, H 24, 18 480 x 18 480 (cfg5) bf16 forward + backward; e4m3 forward + straight-through backward on the operands it hands back; 18 480 x 512 cross
A failure names tensor, head, row, column, err/tol and the 256-row strip / 64-key tile.  tests/test_attn_tol_host.py shows (without a GPU) that these bounds reject a
kernel that loses ONE key of 17 776 and that the absolute tolerances written for short sequences do not.  -m gpu only.  Wall time of the file on one MI355X: 10 s of tests (12 s with start-up);
the measured err/tol maxima are in DESIGN 5."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_tol as T  # noqa: E402
from attn_ref64 import attn_ref64  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops as o
    return o


def _judge(tag, head, R, got, delta="int8", report=None):
    """got: {"o", "lse2"[, "dq", "dk", "dv"]} slices of one head -> list of problems; prints and records the figures"""
    where = f"[{tag} b{head[0]} h{head[1]}]"
    problems, f = T.judge(got, R, delta, where)
    figs = {n: (round(x["max_err_over_tol"], 3), round(x["rms_ratio"], 3), round(x["worst_block_rms_ratio"], 3)) for n, x in f.items() if n != "lse2"}
    figs["lse2"] = round(f["lse2"]["max_err_over_tol"], 3)
    print(f"ATTN_FULLSIZE {where} (max err/tol, rms ratio, worst 256-row rms ratio) {figs}", flush=True)
    if report is not None:
        report[where] = figs
    return problems


def _fused_qkv(B, H, S, D, g):
    """q, k, v as the model passes them: token-major [B, H, S, D] views of one fused [B, S, 3 H D] buffer (the views keep it alive); gradients likewise"""
    buf = torch.randn(B, S, 3 * H * D, generator=g, device="cuda").to(torch.bfloat16)
    view = lambda t: tuple(t.view(B, S, 3, H, D)[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    return view(buf), view(torch.empty_like(buf))


def _run64(ops, q, k, v, do, dqkv, policy=None, split_mode=None):
    B, H, S, D = q.shape
    o_res = torch.empty(B, S, H * D, dtype=torch.uint8, device="cuda")
    o, lse = ops.attention_fwd_raw(q, k, v, o_res=o_res, policy=policy, split_mode=split_mode)
    ov = o.view(B, S, H, D).permute(0, 2, 1, 3)
    if do is None:
        return ov, lse
    ops.attention_bwd_raw(q, k, v, ov, do, lse, *dqkv, o_res=o_res.view(B, S, H, D).permute(0, 2, 1, 3), split_mode=split_mode)
    return ov, lse


def _head64(tag, head, q, k, v, do, ov, lse, dqkv, rounded=True, chunk=2048, report=None):
    b, h = head
    qs = (q[b, h].float() * (64 ** -0.5 * T.LOG2E)).to(torch.bfloat16)          # one bf16 rounding of q * scale * log2 e: the kernels' contract
    R = attn_ref64(qs, k[b, h], v[b, h], None if do is None else do[b, h], smul=1.0, dq_mul=64 ** -0.5, dk_mul=T.LN2, rounded_rowsum=rounded, chunk=chunk)
    got = {"o": ov[b, h], "lse2": lse[b, h]}
    if do is not None:
        got.update(dq=dqkv[0][b, h], dk=dqkv[1][b, h], dv=dqkv[2][b, h])
    return _judge(tag, head, R, got, report=report)


@pytest.mark.parametrize("data", ["randn", "trained_like_gain3"])
def test_head_dim_64_at_the_headline_launch_shape(ops, data):
    """B = 2, H = 48, S = 17 776: forward with the int8 residual, backward with it; O, lse2, dQ, dK, dV of (b0, h0), a middle head and (b1, h47).  (b1, h47) holds the
    leftover tasks the automatic tail-round split cuts (the LAST 64 forward / dQ and 32 dK/dV tasks of the launch: attn_common.h split_plan): asserted by comparing
    O, dQ, dK and dV of that head against a split_mode = 0 run, so the case cannot go vacuous."""
    B, H, S, D = 2, 48, 17776, 64
    g = torch.Generator(device="cuda").manual_seed(17776)
    (q, k, v), dqkv = _fused_qkv(B, H, S, D, g)
    pol = None
    if data != "randn":
        from attn_data import trained_like_qkv
        tq, tk, tv, _ = trained_like_qkv(B, H, S, gain=3.0)
        for dst, src in ((q, tq), (k, tk), (v, tv)):
            dst.copy_(src)
        del tq, tk, tv
        pol = ops.AttnFwdPolicy()
    do = torch.randn(B, S, H * D, generator=g, device="cuda").to(torch.bfloat16).view(B, S, H, D).permute(0, 2, 1, 3)
    ov, lse = _run64(ops, q, k, v, do, dqkv, policy=pol, split_mode=-1)
    if pol is not None:
        print("ATTN_FULLSIZE trained-like redo fraction", pol.redo_fraction, flush=True)
        # sharp rows, no strip redone (a redone strip runs the online kernel, whose fp32 row sum the rounded-sum variance below does not describe)
        assert pol.redo_fraction == 0.0 and pol.mode == "bound", pol.redo_fraction
    problems = []
    if data == "randn":
        g0 = tuple(torch.empty(B, S, H, D, dtype=torch.bfloat16, device="cuda").permute(0, 2, 1, 3) for _ in range(3))
        o0, _ = _run64(ops, q, k, v, do, g0, split_mode=0)
        for name, a, b in (("O", o0, ov), ("dQ", g0[0], dqkv[0]), ("dK", g0[1], dqkv[1]), ("dV", g0[2], dqkv[2])):
            assert bool((a[1, 47].float() != b[1, 47].float()).any()), f"the automatic tail split no longer cuts {name} tasks of (b1, h47): pick the head that holds the leftover tasks"
        del o0, g0
    for head in ((0, 0), (0, 23), (1, 47)):
        problems += _head64(data, head, q, k, v, do, ov, lse, dqkv)
        torch.cuda.empty_cache()
    assert not problems, "\n".join(problems)


def test_head_dim_64_at_41026_tokens(ops):
    """cfg4's sequence length (H = 6 as tests/test_gpu_fullsize.py runs it), forward and backward, first and last head"""
    B, H, S, D = 1, 6, 41026, 64
    g = torch.Generator(device="cuda").manual_seed(41026)
    (q, k, v), dqkv = _fused_qkv(B, H, S, D, g)
    do = torch.randn(B, S, H * D, generator=g, device="cuda").to(torch.bfloat16).view(B, S, H, D).permute(0, 2, 1, 3)
    ov, lse = _run64(ops, q, k, v, do, dqkv)
    problems = []
    for head in ((0, 0), (0, 5)):
        problems += _head64("cfg4", head, q, k, v, do, ov, lse, dqkv, chunk=1024)
        torch.cuda.empty_cache()
    assert not problems, "\n".join(problems)


def test_online_softmax_entry_at_17776_tokens(ops):
    """vgpa_attn_fwd_online_res (what a layer with mostly flagged strips runs, and the redo pass): fp32 row sums of the unrounded weights -- lse2 inside the SAME
    lse2_tol, O inside the bound of a forward normalised by the unrounded sum"""
    B, H, S, D = 2, 48, 17776, 64
    g = torch.Generator(device="cuda").manual_seed(7)
    (q, k, v), _ = _fused_qkv(B, H, S, D, g)
    ov, lse = _run64(ops, q, k, v, None, None, policy=ops.AttnFwdPolicy(mode="online", fixed=True))
    problems = []
    for head in ((0, 1), (1, 47)):
        problems += _head64("online", head, q, k, v, None, ov, lse, None, rounded=False)
        torch.cuda.empty_cache()
    assert not problems, "\n".join(problems)


def _tm(B, S, H, D, g, mul=1.0):
    return (mul * torch.randn(B, S, H, D, generator=g, device="cuda")).to(torch.bfloat16).permute(0, 2, 1, 3)


@pytest.mark.parametrize("Skv", [18480, 512])
def test_head_dim_128_bf16_at_the_cfg5_launch_shape(ops, Skv):
    """B = 2, H = 24, Sq = 18 480 against 18 480 keys (self-attention) and 512 (cross-attention over the text), bf16 forward with the int8 residual and backward"""
    B, H, Sq, D = 2, 24, 18480, 128
    scale = D ** -0.5
    g = torch.Generator(device="cuda").manual_seed(Skv)
    q, do = _tm(B, Sq, H, D, g), _tm(B, Sq, H, D, g)
    k, v = _tm(B, Skv, H, D, g), _tm(B, Skv, H, D, g)
    o_res8 = torch.empty(B, Sq, H * D, dtype=torch.uint8, device="cuda")
    o, lse = ops.attention128_fwd_raw(q, k, v, scale, o_res8=o_res8)
    dq, dk, dv = (torch.empty(B, S_, H, D, dtype=torch.bfloat16, device="cuda").permute(0, 2, 1, 3) for S_ in (Sq, Skv, Skv))
    ops.attention128_bwd_raw(q, k, v, o, do, lse, dq, dk, dv, scale, o_res8=o_res8)
    problems = []
    for b, h in ((0, 0), (1, 23)):
        R = attn_ref64(q[b, h], k[b, h], v[b, h], do[b, h], smul=scale * T.LOG2E, dq_mul=scale, dk_mul=scale, rounded_rowsum=False)
        problems += _judge(f"hd128 bf16 Skv {Skv}", (b, h), R, {"o": o[b, h], "lse2": lse[b, h], "dq": dq[b, h], "dk": dk[b, h], "dv": dv[b, h]})
        del R
        torch.cuda.empty_cache()
    assert not problems, "\n".join(problems)


def test_head_dim_128_e4m3_forward_and_straight_through_backward(ops):
    """vgpa_attn128_fwd_f8 at the cfg5 shape: the reference runs on the operands the kernel hands back (q_deq pre-scaled, k_deq, v_deq), so what is left is the e4m3
    rounding of the weights (attn_tol.PER_ELEMENT: 2^-4 relative, 2^-18 of the tile's sum below e4m3's normal range) and fp32 accumulation; the backward is
    vgpa_attn128_bwd_prescaled on those operands with this forward's lse2, output and residual"""
    B, H, S, D = 2, 24, 18480, 128
    scale = D ** -0.5
    g = torch.Generator(device="cuda").manual_seed(8)
    q, k, v, do = (_tm(B, S, H, D, g) for _ in range(4))
    deq = [torch.empty(B, S, H * D, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    o_res8 = torch.empty(B, S, H * D, dtype=torch.uint8, device="cuda")
    rep = {}
    o, lse = ops.attention128_fwd_raw(q, k, v, scale, f8=True, o_res8=o_res8, deq=deq, report=rep)
    print("ATTN_FULLSIZE e4m3 redo fraction", rep["redo_fraction"], flush=True)
    assert rep["redo_fraction"] == 0.0          # N(0,1): no strip handed to the bf16 redo pass, the figures below are the e4m3 kernel's
    qd, kd, vd = (t.view(B, S, H, D).permute(0, 2, 1, 3) for t in deq)
    dq, dk, dv = (torch.empty(B, S, H, D, dtype=torch.bfloat16, device="cuda").permute(0, 2, 1, 3) for _ in range(3))
    ops.attention128_bwd_raw(qd, kd, vd, o, do, lse, dq, dk, dv, scale, o_res8=o_res8, q_prescaled=True)
    problems = []
    for b, h in ((0, 0), (1, 23)):
        R = attn_ref64(qd[b, h], kd[b, h], vd[b, h], do[b, h], smul=1.0, dq_mul=scale, dk_mul=T.LN2, rounded_rowsum=False, p_unit=2.0 ** -4, p_sub=2.0 ** -18)
        problems += _judge("hd128 e4m3", (b, h), R, {"o": o[b, h], "lse2": lse[b, h], "dq": dq[b, h], "dk": dk[b, h], "dv": dv[b, h]})
        del R
        torch.cuda.empty_cache()
    assert not problems, "\n".join(problems)
