"""The small kernels of the CogVideoX training step, each called on its own and judged per element against fp64 with the bounds derived in
tests/row_tol.py (tests/test_row_tol_host.py shows on the CPU that those bounds reject wrong kernels).  Every case names the code path it is the smallest
shape for.  `-s` prints the largest device error over its bound per case.  -m gpu only."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import row_tol as R
from oracle import dpo as odpo
from oracle import scheduler as osch
from row_tol import bhs

SENT = -776.0          # exact in bf16: what every output buffer holds before a launch


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from videogpa_amd import _lib
    return _lib


def dev(t):
    return None if t is None else t.cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _untouched(t):
    return bool((t.view(torch.int16) == torch.tensor(SENT, dtype=torch.bfloat16).view(torch.int16).item()).all())


# ------------------------------------------------------------------------------------------ QK-norm + RoPE
def _views(layout, B, H, S):
    """two sentinel-filled bf16 buffers and their [B,H,S,64] views -> (q view, k view, check() that everything outside the views still holds the sentinel)"""
    n = B * H * S * 64
    if layout == "bhsd":             # contiguous [B,H,S,64] inside a longer buffer: 64 guard elements on either side
        bufs = [torch.full((n + 128,), SENT, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
        views = [b[64:64 + n].view(B, H, S, 64) for b in bufs]
        return (*views, lambda: all(_untouched(b[:64]) and _untouched(b[64 + n:]) for b in bufs))
    if layout == "padded":           # token-major [B,S,H,64+8]: strides (S H 72, 72, H 72), all multiples of 8; the 8 columns of padding are not the kernel's
        bufs = [torch.full((B, S, H, 72), SENT, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
        views = [b[..., :64].permute(0, 2, 1, 3) for b in bufs]
        return (*views, lambda: all(_untouched(b[..., 64:].contiguous()) for b in bufs))
    if layout == "fused":            # the q and k slices of a [B,S,3,H,64] gradient buffer (where the backward writes in the model): the v slice is not the kernel's
        buf = torch.full((B, S, 3, H, 64), SENT, dtype=torch.bfloat16, device="cuda")
        return bhs(buf, 0), bhs(buf, 1), lambda: _untouched(buf[:, :, 2].contiguous())
    raise ValueError(layout)


def _qk_fwd(ops, lib, c, q_in, k_in, q_out, k_out, Lt, B, H, S, eps, mode, head_dim=64):
    s3 = ops._bhs_strides
    lib.call("vgpa_qknorm_rope_fwd", q_in, k_in, q_out, k_out, s3(q_in), s3(k_in), s3(q_out), s3(k_out), c["wq"], c["bq"], c["wk"], c["bk"], c["cos"], c["sin"],
             Lt, B, H, S, head_dim, float(eps), float(R.QK_SCALE), int(mode), _stream())


def _qk_bwd(ops, lib, c, q_in, k_in, dq_in, dk_in, Lt, B, H, S, eps, mode):
    s3 = ops._bhs_strides
    lib.call("vgpa_qknorm_rope_bwd", c["dq"], c["dk"], q_in, k_in, dq_in, dk_in, s3(c["dq"]), s3(c["dk"]), s3(q_in), s3(k_in), s3(dq_in), s3(dk_in),
             c["wq"], c["wk"], c["cos"], c["sin"], Lt, B, H, S, 64, float(eps), int(mode), _stream())


# (B, S, H, text_len) = R.QK_SHAPES.  256 threads = 32 vectors per workgroup; the kernel's `which = vid >= nvec` switches from q to k at vector B S H:
#   (1, 7, 3, 3)    21 vectors: the switch is at thread 168, inside the third wavefront of the only workgroup (test_qknorm_attention_fused has 184: thread 1472, a wavefront boundary)
#   (2, 33, 2, 0)   no text token: table row = s
#   (2, 33, 2, 33)  tables given and no token rotated; the table has the single row that rope_mode 1 reads for tokens that are off
#   (1, 64, 2, 1)   128 vectors: the switch falls exactly on the boundary between workgroups 3 and 4; the first rotated token is s = 1
#   (3, 5, 5, 2)    75 vectors, every extent odd: b, s, h of the 32-bit index split all change inside a wavefront
@pytest.mark.parametrize("shape", R.QK_SHAPES)
@pytest.mark.parametrize("rope", [None, "contract", "arbitrary"])
@pytest.mark.parametrize("mode", [0, 1])
def test_qknorm_rope_alone(ops, lib, mode, rope, shape):
    B, S, H, Lt = shape
    host = R.qknorm_inputs(B, S, H, Lt, rope, mode)
    c = {k: dev(v) for k, v in host.items()}
    q_host, k_host = bhs(host["qkv"], 0), bhs(host["qkv"], 1)
    q_in, k_in = bhs(c["qkv"], 0), bhs(c["qkv"], 1)                     # the q and k slices of one fused [B,S,3,H,64] buffer
    for eps in (1e-6, 1e-5):
        ref = R.qknorm_rope_ref64(q_host, k_host, host["wq"], host["bq"], host["wk"], host["bk"], host["cos"], host["sin"], Lt, eps, R.QK_SCALE, mode)
        tols = (R.qknorm_fwd_tol(q_host, host["wq"], host["bq"], ref[0], host["cos"], host["sin"], eps, R.QK_SCALE),
                R.qknorm_fwd_tol(k_host, host["wk"], host["bk"], ref[1], host["cos"], host["sin"], eps, 1.0))
        gref = R.qknorm_rope_grad64(host["dq"], host["dk"], q_host, k_host, host["wq"], host["wk"], host["cos"], host["sin"], Lt, eps, mode)
        gtols = (R.qknorm_bwd_tol(host["dq"], q_host, host["wq"], gref[0], host["cos"], host["sin"], Lt, eps, mode),
                 R.qknorm_bwd_tol(host["dk"], k_host, host["wk"], gref[1], host["cos"], host["sin"], Lt, eps, mode))
        for layout in ("bhsd", "padded"):
            q_out, k_out, clean = _views(layout, B, H, S)
            _qk_fwd(ops, lib, c, q_in, k_in, q_out, k_out, Lt, B, H, S, eps, mode)
            torch.cuda.synchronize()
            got = (q_out.cpu(), k_out.cpu())
            print(f"qknorm fwd mode {mode} rope {rope} {shape} eps {eps} {layout}: device / bound q {R.worst(got[0], ref[0], tols[0])[0]:.3f} k {R.worst(got[1], ref[1], tols[1])[0]:.3f}")
            assert not [m for i, n in enumerate("qk") for m in R.judge(f"fwd {layout} {n}", got[i], ref[i], tols[i])]
            assert clean(), f"forward wrote outside its {layout} view"
        for layout in ("fused", "padded"):
            dq_in, dk_in, clean = _views(layout, B, H, S)
            _qk_bwd(ops, lib, c, q_in, k_in, dq_in, dk_in, Lt, B, H, S, eps, mode)
            torch.cuda.synchronize()
            got = (dq_in.cpu(), dk_in.cpu())
            print(f"qknorm bwd mode {mode} rope {rope} {shape} eps {eps} {layout}: device / bound q {R.worst(got[0], gref[0], gtols[0])[0]:.3f} k {R.worst(got[1], gref[1], gtols[1])[0]:.3f}")
            assert not [m for i, n in enumerate("qk") for m in R.judge(f"bwd {layout} {n}", got[i], gref[i], gtols[i])]
            assert clean(), f"backward wrote outside its {layout} view"


def test_qknorm_rope_entries_refuse_what_no_kernel_handles(ops, lib):
    """head_dim != 64, a stride that is no multiple of 8, cos without sin, text_len > S, rope_mode 2: VGPA_ERR_INVALID before any launch.  Every buffer has
    its valid size ([B,H,S,128] for the head_dim 128 call), so a call accepted by mistake would still be a valid launch."""
    L = lib.load()
    B, H, S = 1, 2, 9
    buf = lambda: torch.zeros(B, H, S, 128, dtype=torch.bfloat16, device="cuda")
    q, k, qo, ko, dq, dk, dqi, dki = (buf() for _ in range(8))
    w = torch.ones(128, device="cuda")
    cos, sin = torch.ones(S, 128, device="cuda"), torch.zeros(S, 128, device="cuda")
    good = (ctypes.c_int64 * 3)(H * S * 128, S * 128, 128)
    bad = (ctypes.c_int64 * 3)(H * S * 128, S * 128, 124)
    p = lambda t: None if t is None else t.data_ptr()

    def fwd(si=good, so=good, cos=cos, sin=sin, Lt=2, head_dim=64, mode=0):
        return L.vgpa_qknorm_rope_fwd(p(q), p(k), p(qo), p(ko), si, good, so, good, p(w), p(w), p(w), p(w), p(cos), p(sin), Lt, B, H, S, head_dim, 1e-6, 1.0, mode, _stream())

    def bwd(sg=good, sd=good, cos=cos, sin=sin, Lt=2, head_dim=64, mode=0):
        return L.vgpa_qknorm_rope_bwd(p(dq), p(dk), p(q), p(k), p(dqi), p(dki), sg, good, good, good, sd, good, p(w), p(w), p(cos), p(sin), Lt, B, H, S, head_dim, 1e-6,
                                      mode, _stream())

    assert fwd() == 0 and bwd() == 0 and fwd(mode=1) == 0 and bwd(mode=1) == 0 and fwd(cos=None, sin=None) == 0 and fwd(Lt=S) == 0
    refused = {
        "fwd head_dim": fwd(head_dim=128), "bwd head_dim": bwd(head_dim=128),
        "fwd in stride": fwd(si=bad), "fwd out stride": fwd(so=bad), "bwd grad stride": bwd(sg=bad), "bwd out stride": bwd(sd=bad),
        "fwd cos without sin": fwd(sin=None), "fwd sin without cos": fwd(cos=None), "bwd cos without sin": bwd(sin=None),
        "fwd text_len > S": fwd(Lt=S + 1), "bwd text_len > S": bwd(Lt=S + 1),
        "fwd rope_mode 2": fwd(mode=2), "bwd rope_mode 2": bwd(mode=2),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ gelu_tanh
# gelu_tanh_*_kernel: grid = min(4096, ceil(total8 / 256)) blocks of 256, stride = grid * 256 chunks of 8; a thread handles chunk c and chunk c + stride, then c += 2 stride.
#   8                            one chunk, one thread (the smallest call)
#   8 (4096 256 + 37)            the grid reaches its cap of 4096 blocks and `two` is true for threads 0..36 only: the first shape with a live second chunk
#   8 (2 4096 256 + 300)         every thread has both chunks, and threads 0..299 enter a second loop iteration whose second chunk is absent
# (the suite's earlier shape, 8 448 elements = 1 056 chunks, has stride 1 280 > total8: `two` false everywhere, one iteration)
@pytest.mark.parametrize("n", [8, 8 * (4096 * 256 + 37), 8 * (2 * 4096 * 256 + 300)])
def test_gelu_tanh_second_chunk_and_second_iteration(ops, n):
    u, dy = R.gelu_inputs(n)
    ud = dev(u).requires_grad_(True)
    out = ops.gelu_tanh(ud)
    out.backward(dev(dy))
    torch.cuda.synchronize()
    val, der = R.gelu_ref64(ud.detach(), dev(dy))                      # fp64 on the device: 17 M elements
    tv, td = R.gelu_fwd_tol(ud.detach(), val), R.gelu_bwd_tol(ud.detach(), dev(dy), der)
    print(f"gelu n {n}: device / bound value {R.worst(out, val, tv)[0]:.3f} derivative {R.worst(ud.grad, der, td)[0]:.3f}")
    assert not R.judge("gelu", out.detach(), val, tv)
    assert not R.judge("dgelu", ud.grad, der, td)
    assert torch.equal(out.detach()[-2:].cpu().view(torch.int16), torch.tensor([0.0, -0.0]).to(torch.bfloat16).view(torch.int16))     # +-0 keep their sign


# ------------------------------------------------------------------------------------------ gate_residual
# gate_residual_kernel: grid = min(rows, 16384) blocks, `row += gridDim.x`; inside a row `c += 256` over D / 8 chunks.
#   (3, 5500, 8, 7)     16 500 rows: blocks 0..115 take a second row (the row loop strides), and one chunk per row leaves 255 threads idle
#   (2, 9, 3072, 4)     384 chunks per row: threads 0..127 take a second chunk (the column loop repeats)
#   (1, 5, 264, 5)      every token is text: only gate_t is read; 33 chunks
# (the suite's earlier shape is 38 rows of 32 chunks)
@pytest.mark.parametrize("B,S,D,Lt", [(3, 5500, 8, 7), (2, 9, 3072, 4), (1, 5, 264, 5)])
def test_gate_residual_row_and_column_loops(ops, lib, B, S, D, Lt):
    g = torch.Generator().manual_seed(B * S + D)
    x, y, dout = (torch.randn(B, S, D, generator=g).to(torch.bfloat16) for _ in range(3))
    gates = torch.randn(B, 2, D, generator=g).to(torch.bfloat16).float()
    gfull = torch.cat([gates[:, 1:2].expand(B, Lt, D), gates[:, 0:1].expand(B, S - Lt, D)], 1).to(torch.bfloat16)
    xd, yd, gd = dev(x).requires_grad_(True), dev(y).requires_grad_(True), dev(gates)
    out = ops.gate_residual(xd, yd, gd, Lt)
    out.backward(dev(dout))
    assert torch.equal(out.cpu(), x + gfull * y)                       # torch bf16 semantics: round(g y), then round(x + .)
    assert torch.equal(xd.grad.cpu(), dout)
    assert torch.equal(yd.grad.cpu(), gfull * dout)
    # the x == NULL form (out = gate * y, what the backward launches), through the C entry, into a guarded buffer
    buf = torch.full((B * S * D + 128,), SENT, dtype=torch.bfloat16, device="cuda")
    o = buf[64:64 + B * S * D].view(B, S, D)
    lib.call("vgpa_gate_residual", None, yd.detach(), gd[:, 0], gd[:, 1], gd.stride(0), B, S, D, Lt, o, _stream())
    torch.cuda.synchronize()
    assert torch.equal(o.cpu(), gfull * y)
    assert _untouched(buf[:64]) and _untouched(buf[64 + B * S * D:])


# ------------------------------------------------------------------------------------------ DPO loss
N_VEC, N_ODD = 524288 + 2400, 524288 + 2405
LOSSES = [("sigmoid", 0.0), ("sigmoid", 0.1), ("hinge", 0.0)]
_DT = {torch.float32: 0, torch.bfloat16: 1}


def _dpo_check(name, got, ins64, beta, loss_type, ls, dtype, N, vec_ok, grads=None):
    """got = (loss, margin, winner reward, loser reward, accuracy, errs) of the device; ins64 the six inputs in fp64 on the device"""
    req = [t.clone().requires_grad_(i < 2) for i, t in enumerate(ins64)]
    ref = odpo.dpo_loss(*req, beta=beta, label_smoothing=ls, loss_type=loss_type)
    tol = R.DPO_LOSS_REL * max(1.0, beta)
    loss, margin, wr, lr, acc, errs = got
    eref = R.dpo_errs_ref64(*ins64)
    rel = R.dpo_errs_rel(N, vec_ok)
    print(f"dpo {name} {dtype} beta {beta} {loss_type} ls {ls}: loss err {abs(loss.item() - ref['loss'].item()):.2e} (bound {tol * max(1.0, abs(ref['loss'].item())):.2e}), "
          f"errs device / bound {R.worst(errs, eref, rel * eref)[0]:.3f} (bound {rel:.2e} rel)")
    assert abs(loss.item() - ref["loss"].item()) <= tol * max(1.0, abs(ref["loss"].item()))
    assert abs(margin.item() - ref["reward_margin"].item()) < R.DPO_MARGIN_ABS
    assert abs(wr.item() - ref["winner_reward"].item()) < R.DPO_REWARD_REL * abs(ref["winner_reward"].item())
    assert abs(lr.item() - ref["loser_reward"].item()) < R.DPO_REWARD_REL * abs(ref["loser_reward"].item())
    assert acc.item() == ref["accuracy"].item()
    assert not R.judge(f"{name} errs", errs, eref, rel * eref)
    if grads is not None:
        ref["loss"].backward()
        for n, g, r in (("grad_win", grads[0], req[0].grad), ("grad_lose", grads[1], req[1].grad)):
            bound = torch.full_like(r, R.dpo_grad_rel(beta) * (r.abs().max().item() + 1e-30))
            if dtype == torch.bfloat16:
                bound = bound + R.half_ulp_bf16(r)                     # the store of a bf16 gradient (row_tol, "DPO error means")
            assert g.dtype == dtype and not R.judge(f"{name} {n}", g, r, bound)
    return errs.double(), eref


def _dpo_padded(lib, ins, beta, loss_type, ls, dtype):
    """the C entries with per-sample strides of 8 ceil(N / 8): every row starts 16-byte aligned, so the vector body runs and the scalar tail takes N mod 8
    elements.  The padding holds 1000: read by mistake it would show in every sum.  Gradients go into sentinel-free buffers of the same padded shape."""
    B, N = ins[0].shape
    st = 8 * -(-N // 8)
    pad = []
    for t in ins:
        b = torch.full((B, st), 1000.0, dtype=dtype, device="cuda")
        b[:, :N] = t
        pad.append(b)
    out5, dlogit, errs = torch.empty(5, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, 4, device="cuda")
    wsb = lib.query("vgpa_dpo_loss_workspace_bytes", B)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    lt = {"sigmoid": 0, "hinge": 1}[loss_type]
    lib.call("vgpa_dpo_loss_fwd", *pad, B, N, st, st, st, _DT[dtype], float(beta), float(ls), lt, 0, out5, dlogit, errs, ws, wsb, _stream())
    gw, gl = (torch.full((B, st), 7.0, dtype=dtype, device="cuda") for _ in range(2))
    lib.call("vgpa_dpo_loss_bwd", pad[0], pad[1], pad[4], pad[5], B, N, st, st, st, _DT[dtype], float(beta), 0, dlogit, None, gw, gl, _stream())
    torch.cuda.synchronize()
    assert bool((gw[:, N:] == 7.0).all()) and bool((gl[:, N:] == 7.0).all()), "the backward wrote into the padding"
    return (*out5.unbind(0), errs), (gw[:, :N], gl[:, :N])


# dpo_err_partial_kernel / dpo_bwd_kernel: grid = min(256, ceil(N / 2048)) x B blocks of 256; vector loop over N / 8 chunks with stride grid * 256 when every
# base is aligned and every per-sample stride is a multiple of 8 (vec_ok), then a scalar loop from 8 (N / 8) -- from 0 without vec_ok -- with the same stride.
#   N = 524 288 + 2 400 (ops.dpo_loss)            65 836 chunks over 65 536 threads: threads 0..299 take a second chunk (the vector loop strides)
#   N = 524 288 + 2 405 (ops.dpo_loss)            the per-sample stride N is odd: vec_ok = 0, the scalar loop takes all of it, 8.04 elements per thread (it strides)
#   N = 524 288 + 2 405, strides 524 288 + 2 408  vec_ok = 1: the vector body as above plus a scalar tail of 5 elements
# The three share their values on the common prefix (R.dpo_inputs cuts one draw), the last two wholly: their errs must agree.
# (the suite's earlier shapes: N <= 44 928, a multiple of 8, at most 22 blocks, one chunk per thread)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dpo_loss_grid_stride_scalar_tail_and_scalar_fallback(ops, lib, dtype):
    B = 2
    sums = {}
    for name, N, vec_ok in (("vector", N_VEC, True), ("scalar", N_ODD, False), ("padded", N_ODD, True)):
        ins = [dev(t) for t in R.dpo_inputs(B, N, dtype)]
        ins64 = [t.double() for t in ins]
        for beta in (1.0, 500.0):
            for loss_type, ls in LOSSES:
                if name == "padded":
                    got, grads = _dpo_padded(lib, ins, beta, loss_type, ls, dtype)
                else:
                    req = [t.clone().requires_grad_(i < 2) for i, t in enumerate(ins)]
                    got = ops.dpo_loss(*req, beta=beta, label_smoothing=ls, loss_type=loss_type)
                    got[0].backward()
                    grads = (req[0].grad, req[1].grad)
                errs, eref = _dpo_check(name, got, ins64, beta, loss_type, ls, dtype, N, vec_ok, grads)
        sums[name] = (errs * N, eref * N, R.dpo_errs_rel(N, vec_ok))
    # one another: the same values -> the same means; five elements more -> the sums differ by exactly those five (fp64), to the bound of the larger count of additions
    (sv, rv, bv), (ss, rs, bs), (sp, rp, bp) = sums["vector"], sums["scalar"], sums["padded"]
    assert not R.judge("scalar against padded", ss, sp, max(bs, bp) * rs)
    assert float((rs - rv).min()) > 10 * max(bv, bs) * float(rs.max()),"the five elements must weigh more than the bound, or a dropped tail would pass"
    assert not R.judge("scalar - vector = the last five", ss - sv, rs - rv, max(bs, bv) * rs)
    assert not R.judge("padded - vector = the last five", sp - sv, rp - rv, max(bp, bv) * rp)


# N = 1 248, v_win one element past an aligned base: aligned_ok fails for that one pointer, vec_ok = 0 although N and the strides are multiples of 8; one block,
# 4.9 elements per thread in the scalar loop.  The same values from an aligned copy take the vector path: both are held to the fp64 means.
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dpo_loss_one_unaligned_base_takes_the_scalar_path(ops, dtype):
    B, N = 2, 1248
    ins = [dev(t) for t in R.dpo_inputs(B, N, dtype)]
    raw = torch.zeros(B * N + 1, dtype=dtype, device="cuda")
    raw[1:] = ins[0].flatten()
    shifted = raw[1:].view(B, N)
    assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    ins64 = [t.double() for t in ins]
    for first, vec_ok in ((shifted, False), (ins[0], True)):
        req = [t.clone().requires_grad_(i < 2) if i else first.requires_grad_(True) for i, t in enumerate(ins)]
        assert req[0].data_ptr() == first.data_ptr()
        got = ops.dpo_loss(*req, beta=500.0)
        got[0].backward()
        _dpo_check(f"unaligned={not vec_ok}", got, ins64, 500.0, "sigmoid", 0.0, dtype, N, vec_ok, (req[0].grad, req[1].grad))
        first.grad = None
        first.requires_grad_(False)


# dpo_loss_paired: win and lose are the halves of one [B,2,N] buffer, per-sample stride 2 N (a multiple of 8); N = 524 288 + 2 400 as above: the vector loop strides
def test_dpo_loss_paired_grid_stride(ops):
    B, N, dtype = 2, N_VEC, torch.bfloat16
    ins = [dev(t) for t in R.dpo_inputs(B, N, dtype)]
    v, vref, tgt = (torch.stack([ins[i], ins[i + 1]], 1).contiguous() for i in (0, 2, 4))
    for beta, (loss_type, ls) in ((1.0, LOSSES[1]), (500.0, LOSSES[2])):
        vr = v.clone().requires_grad_(True)
        got = ops.dpo_loss_paired(vr, vref, tgt, beta=beta, label_smoothing=ls, loss_type=loss_type)
        got[0].backward()
        _dpo_check("paired", got, [t.double() for t in ins], beta, loss_type, ls, dtype, N, True, (vr.grad[:, 0], vr.grad[:, 1]))


# ------------------------------------------------------------------------------------------ noise / velocity
# noise_velocity_kernel / flow_noise_velocity_kernel: grid = min(2048, ceil(N / 8 / 256)) x B; N = 8 (2048 256 + 77): the cap is reached and threads 0..76 take a
# second chunk (the suite's earlier shapes stop at N = 4 800: 3 blocks)
N_NOISE = 8 * (2048 * 256 + 77)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_noise_velocity_at_the_grid_cap_bit_exact(ops, dtype):
    g = torch.Generator().manual_seed(31)
    B = 2
    x = (torch.randn(B, 2, N_NOISE, generator=g) * 0.7).to(dtype)
    eps = torch.randn(B, N_NOISE, generator=g).to(dtype)
    t = torch.tensor([0, 999])
    ad = osch.alphas_cumprod().to(dtype)           # diffusers casts the table to the sample dtype first
    sa, sb = (ad ** 0.5)[t].view(B, 1), ((1 - ad) ** 0.5)[t].view(B, 1)
    xt, v = ops.noise_velocity_paired(dev(x), dev(eps), dev(t), dev((ad ** 0.5).float()), dev(((1 - ad) ** 0.5).float()))
    for p in range(2):
        assert torch.equal(xt[:, p].cpu(), sa * x[:, p] + sb * eps)
        assert torch.equal(v[:, p].cpu(), sa * eps - sb * x[:, p])


@pytest.mark.parametrize("dtype,xt_fp32", [(torch.float32, True), (torch.bfloat16, True), (torch.bfloat16, False)])
def test_flow_noise_velocity_at_the_grid_cap_bit_exact(ops, dtype, xt_fp32):
    g = torch.Generator().manual_seed(32)
    B = 2
    x = torch.randn(B, 2, N_NOISE, generator=g).to(dtype)
    eps = torch.randn(B, N_NOISE, generator=g).to(dtype)
    sigma = ops.flow_sigma(torch.tensor([0, 999]), 1000, 5.0)
    xt, v = ops.flow_noise_velocity_paired(dev(x), dev(eps), dev(sigma), xt_fp32=xt_fp32)
    sg = sigma.view(B, 1)
    for p in range(2):
        ref_xt = (1.0 - sg) * x[:, p] + sg * eps                       # fp32 by torch's promotion of the fp32 sigma
        assert ref_xt.dtype == torch.float32
        if not xt_fp32:
            ref_xt = ref_xt.to(dtype)
        assert xt.dtype == ref_xt.dtype and torch.equal(xt[:, p].cpu(), ref_xt)
        assert torch.equal(v[:, p].cpu(), eps - x[:, p])


# ------------------------------------------------------------------------------------------ AdamW, gradient norm
# adamw_kernel / sumsq_partial_kernel: grid = min(1024, ceil(n / 4 / 256)) blocks of 256 over n / 4 float4, then a scalar loop over n mod 4.
#   n = 2 097 152 + 203   524 338 float4 over 262 144 threads: the grid is capped and threads 0..49 take a third float4 (the loop strides), a tail of 3
#   n = 5                 one float4 and a tail of one
# (the suite's earlier shape is n = 5 133 through FlatAdamW: 6 blocks, one float4 per thread)
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("gstd,grad_scale,max_norm", R.ADAMW_COMBOS)
@pytest.mark.parametrize("n", [2097152 + 203, 5])
def test_adamw_step_and_grad_norm_alone(ops, n, gstd, grad_scale, max_norm, wd):
    p, g, m, v, z = (dev(t) if torch.is_tensor(t) else t for t in R.adamw_state(n))
    g = g * gstd
    tn = None
    if max_norm > 0:
        tn = ops.grad_norm(g, grad_scale)
        ref_n = R.grad_norm_ref64(g, grad_scale)
        print(f"grad_norm n {n} std {gstd}: device err {abs(tn.item() - ref_n) / ref_n:.2e} rel, bound {R.grad_norm_rel(n):.2e}")
        assert abs(tn.item() - ref_n) <= R.grad_norm_rel(n) * ref_n
        assert (ref_n > 2.0) if gstd == 3.0 else (ref_n < 0.5)
    H = R.ADAMW_HYPER
    for step in (1, 2, 1000):
        before = (p.clone(), m.clone(), v.clone())
        ops.adamw_step(p, g, m, v, H["lr"], H["beta1"], H["beta2"], H["eps"], wd, step, grad_scale=grad_scale, max_norm=max_norm, total_norm=tn)
        kw = dict(H, weight_decay=wd, step=step, grad_scale=grad_scale, max_norm=max_norm, total_norm=None if tn is None else tn.item())
        ref = R.adamw_ref64(before[0], g, before[1], before[2], **kw)             # fp64 from the same fp32 buffers
        tols = R.adamw_tols(g, before[1], before[2], ref[1], ref[2], ref[0], H["beta1"], H["beta2"], grad_scale, max_norm, kw["total_norm"])
        for name, a, r, t in zip(("param", "exp_avg", "exp_avg_sq"), (p, m, v), ref, tols):
            print(f"adamw n {n} std {gstd} wd {wd} step {step} {name}: device / bound {R.worst(a, r, t)[0]:.3f}")
            assert not R.judge(f"{name} step {step}", a, r, t)
        # zero gradient, zero moments: the moments stay exactly zero and the parameter moves by the decay alone
        assert not bool(m[z].any()) and not bool(v[z].any())
        assert torch.allclose(p[z].double(), before[0][z].double() * (1.0 - float(torch.tensor(H["lr"]).float()) * float(torch.tensor(wd).float())), rtol=3 * R.U, atol=0)


def test_adamw_refusals(ops):
    n = 64
    p, g, m, v = (torch.zeros(n + 4, device="cuda") for _ in range(4))
    tn = torch.ones(1, device="cuda")
    H = R.ADAMW_HYPER
    args = (H["lr"], H["beta1"], H["beta2"], H["eps"], 0.01)
    ops.adamw_step(p[:n], g[:n], m[:n], v[:n], *args, 1, max_norm=1.0, total_norm=tn)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.adamw_step(p[:n], g[:n], m[:n], v[:n], *args, 0)                                   # step = 0
    for i in range(4):                                                                          # one pointer 4 bytes past a 16-byte boundary
        ts = [t[1:n + 1] if j == i else t[:n] for j, t in enumerate((p, g, m, v))]
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.adamw_step(*ts, *args, 1)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.adamw_step(p[:n], g[:n], m[:n], v[:n], *args, 1, max_norm=1.0, total_norm=None)    # clipping asked for, no norm given
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.grad_norm(g[1:n + 1])
    torch.cuda.synchronize()
