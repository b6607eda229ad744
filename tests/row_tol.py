"""fp64 references, per-element bounds and float32 restatements of the small kernels of the CogVideoX training step: QK-norm + RoPE
(csrc/qknorm.hip), gelu_tanh (csrc/norm.hip), the DPO error reduction (csrc/dpo_loss.hip), AdamW and the gradient norm (csrc/adamw.hip).
tests/test_row_tol_host.py shows on the CPU that the restatements stay inside the bounds and that wrong variants do not;
tests/test_gpu_step_kernels.py holds the device to the same bounds.  No number below was fitted to a device result.

Units.  u = 2^-24 is the unit roundoff of fp32 (half an ulp, relative): one correctly rounded fp32 operation is off by at most u |result|.  The hardware
exp2 / rcp / rsq are 1 ulp = 2u (CDNA ISA: V_EXP_F32, V_RCP_F32, V_RSQ_F32).  hipcc contracts a*b+c into one FMA where it likes: that only removes
roundings, so every count below takes the uncontracted form.

bf16 store (`half_ulp_bf16`, the statement of tests/attn_tol.py).  bf16 keeps 8 significant bits: round-to-nearest is off by at most half an ulp,
2^(floor(log2 |x|) - 8), which is 2^-9 |x| when the mantissa is just under 2 and 2^-8 |x| at mantissa 1.0.  2^-9 |ref| is therefore the smallest
figure a correct rounding can stay under, not a bound on it (1.00390625 rounds to 1.0 or 1.0078125, either way 2^-8 away); every tolerance of a bf16
result here is
    tol = half_ulp_bf16(|ref| + rest) + rest
with `rest` the fp32 error before the store; the ulp is taken at |ref| + rest because the unrounded value may sit in the next binade.

QK-norm forward, one vector of 64 (eight lanes of eight):  y_d = (x_d - mean) rstd w_d + b_d, rotation, q_scale, store.
    mean    seven serial adds per lane, three shuffle adds, an exact * 1/64: |d mean| <= 10u mean|x|                                    (C_MEAN = 10)
    x-mean  1u.   var: the squares carry 2u + 1u, their sum 10u -> 13u relative (the mean's own error enters at second order: sum d = 0); + eps 1u;
            rsq 2u:  rstd is off by 13/2 + 1/2 + 2 = 9u relative                                                                           (C_RSTD = 9)
    affine  (x - mean) [1u] * rstd [9u + 1u] * w [1u] + b [1u]:  12u |xhat_d w_d| + 1u |y_d|
    rope    two products and a sum: 2u (|y_d cos_d| + |y_p sin_d|), and it carries the errors of y_d and y_p with weights |cos_d|, |sin_d|
    scale   1u
    With A = max_d (|xhat_d w_d| + |b_d|), the vector's largest pre-rotation magnitude without credit for cancellation, and T = max(1, max_d |cos_d| +
    |sin_d|) over the table (1 without a table):
        rest = u q_scale T (16 A + 10 K),      16 = 12 + 1 + 2 + 1 = C_FWD,      K = mean|x| rstd max|w|  (what the mean's error is multiplied by)
    K is the conditioning of LayerNorm itself (a vector of large mean and tiny spread), not a property of the kernel; on N(0.3, 1.7) inputs K < A.
QK-norm backward:  g'_d = g_d cos_d + S_p g_p sin_p (the transposed rotation), gw_d = g'_d w_d, c1 = mean gw, c2 = mean gw xhat,
    dx_d = rstd (gw_d - c1 - xhat_d c2).  With G = max_d (|g_d cos_d| + |g_p sin_p|) |w_d| >= |gw_d|, hence |c1| <= G and |c2| <= G (Cauchy-Schwarz, mean xhat^2 <= 1):
    gw      2u rotation + 1u product = 3u G
    xhat    1u + 9u + 1u = 11u relative, plus the shift d mean rstd <= 10u K',  K' = mean|x| rstd
    c1      3u G + 10u G (the sum) = 13u G.   c2: terms (3 + 11 + 1)u, sum 10u:  25u G mean|xhat| <= 25u G
    dx      rstd [3u G + 13u G + |xhat_d| (11u G + 25u G) + 3u (|gw_d| + |c1| + |xhat_d c2|)] + (9 + 1)u |dx_d|,   |dx_d| <= rstd G (2 + |xhat_d|)
            = u rstd G (42 + 49 |xhat_d|);   the shift of xhat moves c2 by <= 10u K' G and xhat_d c2 by <= 10u K' G (1 + |xhat_d|)
        rest = u rstd G (1 + X) (49 + 10 K'),      X = max_d |xhat_d|                                                                      (C_BWD = 49)
    It scales with rstd max|g w| as it must: dx = rstd (g - c1 - xhat c2) cancels, so nothing smaller than its terms bounds the error.

gelu_tanh (common.h gelu_sig): s = rcp(1 + exp2(t)), t = x (K1 + K2 x^2); value x s; derivative dy (s + x (s - s^2) dz2), dz2 = 2c + 6c 0.044715 x^2.
    t       x^2 1u, K2 x^2 + K1 2u (same signs, no cancellation), * x 1u, the literals 1u: 5u |t|, i.e. exp2(t) is off by ln2 5u |t| + 2u relative
    s       R u relative,  R = 3 + (1 - s) (2 + 3.5 |t|)      (1 + e: 1u, rcp: 2u, and e / (1 + e) = 1 - s of the error of e)
    SUB     = 2^-126, the smallest normal fp32.  Below x = -10 the true s is under SUB: exp2 overflows to inf from t = 128 and rcp returns 0 for it, and a
            subnormal result of rcp, of a product or of the bf16 pack may be flushed to zero.  So s carries an ABSOLUTE error of up to SUB next to R u s,
            and so does every later result
    value   rest = (R + 1) u |ref| + (|x| + 1) SUB
    deriv   b = s - s^2 is off by (R + 1) u s + u b (the same computed s on both sides: d b = s R u (1 - 2s) - s^2 u);  x b dz2: dz2 2u, two products 2u
            rest = u |dy| [R s + |x| dz2 ((R + 1) s + b) + 4 |x b dz2| + 2 |s + x b dz2|] + (|dy| (1 + |x| dz2) + 1) SUB
            (the SUB of s is multiplied by x dz2, up to 389 at x = -12: at x = -10 the device returns 0 where the derivative is 230 s = 2e-36, a normal fp32)
    At x = 12 this is 1.6e3 u = 1e-4 of the result: far below the bf16 half ulp, so the store decides almost everywhere; the fp32 term decides near
    the zeros of the result.

DPO error means (dpo_err_partial_kernel): per thread fp32 partial sums of (a - t)^2, then fp64.  d = a - t 1u, so d^2 2u + 1u; k non-negative terms added in
    fp32 add k u; the fp64 block / grid sums add nothing visible; the final (float) cast 1u:
        |errs - ref| <= (k + 4) u ref,      k = fp32 additions per thread and accumulator at that N  (`dpo_adds_per_thread`: 8 per chunk of the vector
        loop, 1 per element of the scalar loop, over a grid of min(256, ceil(N / 2048)) blocks of 256)
    Loss, margin, rewards and gradients take the bounds tests/test_gpu_kernels.py::test_dpo_loss_golden uses (DPO_LOSS_REL, DPO_MARGIN_ABS, DPO_REWARD_REL,
    dpo_grad_rel).  A bf16 gradient cannot meet 2.5e-4 of the maximum per element at beta = 1 (its store alone is 2^-9 .. 2^-8 of the element): for bf16
    gradients half_ulp_bf16 of the element is added, nothing else.

AdamW (adamw_kernel; header comment of csrc/adamw.hip: clip_grad_norm_ then torch.optim.AdamW).  The C entry takes lr, beta1, beta2, eps, weight_decay,
    grad_scale and max_norm as floats: the reference evaluates the same formulas in fp64 FROM THOSE fp32 VALUES and from the fp32 buffers (1.f - beta is exact
    in fp32 for beta >= 0.5, Sterbenz).  [1 - float(0.999) is 1.3e-5 below 0.001, which torch rounds from the double: that is the interface, and it is far below ADAMW_P_RTOL.]
    coef    norm + 1e-6 1u, the division 1u, * grad_scale 1u: 3u;  gj = g coef 1u -> 4u
    m'      beta1 m [1u] + (1 - beta1) gj [4u + 1u], the sum 1u over both: |dm'| <= 7u (|beta1 m| + |(1 - beta1) gj|)            (C_M = 7; m and g may cancel, so
            the bound is relative to the sum of magnitudes)
    v'      beta2 v [1u] + (1 - beta2) gj gj [8u + 2u], the sum 1u: |dv'| <= 11u v'  (non-negative terms)                           (C_V = 11)
    param   rtol 1e-5, atol 1e-6: tests/test_gpu_model.py::test_optimizer_step_matches_torch_adamw
grad_norm (sumsq_partial_kernel): per iteration four squares and three adds (4u), one add into the accumulator per iteration (k u, k = iterations per thread incl.
    the scalar tail), fp64 from there; the square root halves it, the (float) cast adds 1u:   |norm - ref| <= ((4 + k) / 2 + 1) u ref

gate_residual and the noise kernels are bit-exact with a torch expression; they need no bound."""
import math

import numpy as np
import torch

U = 2.0 ** -24
C_MEAN, C_RSTD, C_FWD, C_BWD = 10.0, 9.0, 16.0, 49.0
GELU_SUB = 2.0 ** -126
C_M, C_V = 7.0, 11.0
ADAMW_P_RTOL, ADAMW_P_ATOL = 1e-5, 1e-6
DPO_LOSS_REL, DPO_MARGIN_ABS, DPO_REWARD_REL = 5e-6, 2e-6, 5e-6


def dpo_grad_rel(beta):
    return max(1e-5, 50 * DPO_LOSS_REL * max(1.0, beta))


def half_ulp_bf16(x):
    """half an ulp of bf16 at magnitude |x| (0 at 0)"""
    x = x.abs()
    return torch.where(x > 0, torch.exp2(torch.floor(torch.log2(x.clamp_min(1e-300))) - 8.0), torch.zeros_like(x))


def bf16_tol(ref, rest):
    return half_ulp_bf16(ref.abs() + rest) + rest


def judge(where, got, ref, tol, limit=5):
    """-> list of messages, one per element outside its bound (the `limit` worst): where, index, got, want, bound.  Empty = everywhere inside.  NaN is outside."""
    ref = _t64(ref)
    got, tol = _t64(got).to(ref.device), _t64(tol).to(ref.device)
    if got.shape != ref.shape:
        return [f"{where}: shape {tuple(got.shape)} where {tuple(ref.shape)} was expected"]
    tol = tol.expand_as(ref)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if not bool(bad.any()):
        return []
    over = torch.where(bad, torch.nan_to_num(err / tol.clamp_min(1e-300), nan=float("inf")), torch.zeros_like(err)).flatten()
    out = [f"{where}: {int(bad.sum())} of {bad.numel()} elements outside their bound"]
    for i in torch.topk(over, min(limit, int(bad.sum()))).indices.tolist():
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape))) if ref.dim() else ()
        out.append(f"{where}{list(idx)}: got {got.flatten()[i].item():.9g}, want {ref.flatten()[i].item():.9g}, bound {tol.flatten()[i].item():.3g}")
    return out


def worst(got, ref, tol):
    """(largest |err| / bound, the largest |err|, the bound at that element): the figures a test prints before it asserts"""
    ref = _t64(ref)
    got, tol = _t64(got).to(ref.device), _t64(tol).to(ref.device).expand_as(ref)
    err = (got - ref).abs()
    i = int(torch.nan_to_num(err / tol.clamp_min(1e-300), nan=float("inf")).flatten().argmax())
    return float(err.flatten()[i] / tol.flatten()[i].clamp_min(1e-300)), float(err.max()), float(tol.flatten()[i])


def _t64(a):
    if not torch.is_tensor(a):
        a = torch.as_tensor(np.asarray(a, dtype=np.float64))
    if a.requires_grad and a.dtype == torch.float64:            # the leaves of qknorm_rope_grad64 / gelu_ref64 pass through
        return a
    return a.detach().double()          # on the tensor's own device: the large cases are judged where they were computed


# ------------------------------------------------------------------------------------------ QK-norm + RoPE
def rope_map(rope_mode):
    """out[d] = y[d] cos[d] + sign[d] y[partner[d]] sin[d]:  mode 0 pairs (2j, 2j+1), mode 1 pairs (i, i+16) inside each 32-feature half"""
    d = np.arange(64)
    if rope_mode == 0:
        return d ^ 1, np.where(d % 2 == 0, -1.0, 1.0)
    if rope_mode == 1:
        return d ^ 16, np.where(d & 16, 1.0, -1.0)
    raise ValueError(rope_mode)


def _rope64(y, cos, sin, text_len, rope_mode):
    """y [B,H,S,64] fp64; cos / sin [>= S - text_len, 64] or None: tokens s >= text_len take table row s - text_len"""
    if cos is None or text_len >= y.shape[2]:
        return y
    partner, sign = rope_map(rope_mode)
    n = y.shape[2] - text_len
    c, s = _t64(cos)[:n], _t64(sin)[:n]
    v = y[:, :, text_len:]
    v = v * c + torch.as_tensor(sign) * v[..., torch.as_tensor(partner)] * s
    return torch.cat([y[:, :, :text_len], v], 2)


def _ln64(x, w, b, eps):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = (d.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xhat = d * rstd
    return xhat * w + (0 if b is None else b), xhat, rstd


def qknorm_rope_ref64(q, k, wq, bq, wk, bk, cos, sin, text_len, eps, q_scale, rope_mode):
    """q, k [B,H,S,64] (any strides, bf16-valued) -> (q_out, k_out) fp64 [B,H,S,64].  eps is used as the float the C entry receives."""
    eps = float(np.float32(eps))
    yq, _, _ = _ln64(_t64(q), _t64(wq), _t64(bq), eps)
    yk, _, _ = _ln64(_t64(k), _t64(wk), _t64(bk), eps)
    return _rope64(yq, cos, sin, text_len, rope_mode) * float(np.float32(q_scale)), _rope64(yk, cos, sin, text_len, rope_mode)


def qknorm_rope_grad64(dq_out, dk_out, q, k, wq, wk, cos, sin, text_len, eps, rope_mode):
    """d(q_in), d(k_in) fp64 of qknorm_rope_ref64 at q_scale = 1 (what vgpa_qknorm_rope_bwd computes), through torch.autograd"""
    qq, kk = _t64(q).clone().requires_grad_(True), _t64(k).clone().requires_grad_(True)
    z = torch.zeros(64, dtype=torch.float64)
    oq, ok = qknorm_rope_ref64(qq, kk, wq, z, wk, z, cos, sin, text_len, eps, 1.0, rope_mode)
    torch.autograd.backward([oq, ok], [_t64(dq_out), _t64(dk_out)])
    return qq.grad, kk.grad


def _table_gain(cos, sin):
    return 1.0 if cos is None else max(1.0, float((_t64(cos).abs() + _t64(sin).abs()).max()))


def qknorm_fwd_tol(x, w, b, ref, cos, sin, eps, scale):
    """per-element bound of one output tensor (x [B,H,S,64] its input, ref its fp64 result; scale = q_scale for q, 1 for k)"""
    x, w = _t64(x), _t64(w)
    _, xhat, rstd = _ln64(x, w, None, float(np.float32(eps)))
    A = ((xhat * w).abs() + _t64(b).abs()).amax(-1, keepdim=True)
    K = x.abs().mean(-1, keepdim=True) * rstd * float(w.abs().max())
    rest = U * abs(float(np.float32(scale))) * _table_gain(cos, sin) * (C_FWD * A + C_MEAN * K)
    return bf16_tol(ref, rest.expand_as(ref))


def qknorm_bwd_tol(g, x, w, ref, cos, sin, text_len, eps, rope_mode):
    """per-element bound of one input gradient (g the incoming gradient, x the forward input, ref the fp64 gradient)"""
    g, x, w = _t64(g), _t64(x), _t64(w)
    _, xhat, rstd = _ln64(x, w, None, float(np.float32(eps)))
    gmag = g.abs()
    if cos is not None and text_len < x.shape[2]:
        partner, _ = rope_map(rope_mode)
        p = torch.as_tensor(partner)
        n = x.shape[2] - text_len
        c, s = _t64(cos)[:n].abs(), _t64(sin)[:n].abs()
        v = gmag[:, :, text_len:]
        gmag = torch.cat([gmag[:, :, :text_len], v * c + v[..., p] * s[..., p]], 2)
    G = (gmag * w.abs()).amax(-1, keepdim=True)
    X = xhat.abs().amax(-1, keepdim=True)
    Kp = x.abs().mean(-1, keepdim=True) * rstd
    rest = U * rstd * G * (1 + X) * (C_BWD + C_MEAN * Kp)
    return bf16_tol(ref, rest.expand_as(ref))


# ---- float32 restatements (numpy, the order of operations of the .hip source); `wrong` names a deliberately wrong variant for tests/test_row_tol_host.py
def f32(a):
    if torch.is_tensor(a):
        a = a.detach().float().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def bf16_round(a):
    """float32 array -> nearest bf16 value (ties to even), as float32"""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    b = (b + (((b >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


_ONE, _R64 = np.float32(1.0), np.float32(1.0 / 64.0)


def _group8_sum(v):
    """v [..., 8 lanes]: v += shfl_xor(v, 1), 2, 4"""
    lane = np.arange(8)
    for m in (1, 2, 4):
        v = v + v[..., lane ^ m]
    return v


def _lane_sum(t):
    acc = np.zeros(t.shape[:-1], np.float32)
    for j in range(8):
        acc = acc + t[..., j]
    return acc


def _stats_f32(x, eps):
    """x [..., 8 lanes, 8] -> x - mean, rstd [..., 8, 1]"""
    mean = _group8_sum(_lane_sum(x)) * _R64
    d = x - mean[..., None]
    var = _group8_sum(_lane_sum(d * d)) * _R64
    return d, (_ONE / np.sqrt(var + np.float32(eps)))[..., None]


def _tables_f32(cos, sin, S, text_len, row_of_s=False):
    """rows of the tables for every token s (row 0 for the tokens that are not rotated), as [S, 8, 8]"""
    s = np.arange(S)
    row = np.where(s >= text_len, s if row_of_s else s - text_len, 0)
    row = np.minimum(row, len(cos) - 1)
    return f32(cos)[row].reshape(S, 8, 8), f32(sin)[row].reshape(S, 8, 8)


def _qknorm_fwd_one(x, w, b, cos, sin, text_len, eps, scale, rope_mode, wrong):
    B, H, S, _ = x.shape
    x = f32(x).reshape(B, H, S, 8, 8)
    w, b = f32(w).reshape(8, 8), f32(b).reshape(8, 8)
    d, rstd = _stats_f32(x, 1e-5 if wrong == "eps" else eps)
    y = d * rstd * w + b
    if cos is not None:
        c, s = _tables_f32(cos, sin, S, text_len, row_of_s=wrong == "row_s")
        on = (np.arange(S) >= text_len + (1 if wrong == "skip_first" else 0))[:, None, None]
        if rope_mode == 1:
            sgn = np.where(np.arange(8) & 2, 1.0, -1.0).astype(np.float32)[:, None]
            if wrong == "sign1":
                sgn = -np.ones_like(sgn)
            r = y * c + sgn * y[..., np.arange(8) ^ 2, :] * s
        else:
            yp = y[..., np.arange(8) ^ 1]
            r = np.where(np.arange(8) % 2 == 0, y * c - yp * s, y * c + yp * s)
        y = np.where(on, r, y)
    if scale is not None:
        if wrong == "round_q":
            y = bf16_round(y)
        y = y * np.float32(scale)
    return bf16_round(y).reshape(B, H, S, 64)


def qknorm_rope_fwd_f32(q, k, wq, bq, wk, bk, cos, sin, text_len, eps, q_scale, rope_mode, wrong=None):
    return (_qknorm_fwd_one(q, wq, bq, cos, sin, text_len, eps, q_scale, rope_mode, wrong),
            _qknorm_fwd_one(k, wk, bk, cos, sin, text_len, eps, None, rope_mode, wrong))


def _qknorm_bwd_one(g, x, w, cos, sin, text_len, eps, rope_mode, wrong):
    B, H, S, _ = x.shape
    g, x, w = f32(g).reshape(B, H, S, 8, 8), f32(x).reshape(B, H, S, 8, 8), f32(w).reshape(8, 8)
    if cos is not None:
        c, s = _tables_f32(cos, sin, S, text_len)
        on = (np.arange(S) >= text_len)[:, None, None]
        if rope_mode == 1:
            sgn = np.where(np.arange(8) & 2, -1.0, 1.0).astype(np.float32)[:, None]
            sp = s if wrong == "own_sin" else s[:, np.arange(8) ^ 2, :]
            r = g * c + sgn * g[..., np.arange(8) ^ 2, :] * sp
        else:
            gp = g[..., np.arange(8) ^ 1]
            sp = s[..., np.arange(8) ^ 1]                                    # even j reads sp[j + 1], odd j reads sp[j - 1]
            if wrong == "sp_j":
                sp = np.where(np.arange(8) % 2 == 0, s, sp)
            r = np.where(np.arange(8) % 2 == 0, g * c + gp * sp, g * c - gp * sp)
        g = np.where(on, r, g)
    d, rstd = _stats_f32(x, eps)
    xh = d * rstd
    gw = g * w
    c1 = (_group8_sum(_lane_sum(gw)) * _R64)[..., None]
    c2 = (_group8_sum(_lane_sum(gw * xh)) * _R64)[..., None]
    return bf16_round(rstd * (gw - c1 - xh * c2)).reshape(B, H, S, 64)


def qknorm_rope_bwd_f32(dq_out, dk_out, q, k, wq, wk, cos, sin, text_len, eps, rope_mode, wrong=None):
    return (_qknorm_bwd_one(dq_out, q, wq, cos, sin, text_len, eps, rope_mode, wrong),
            _qknorm_bwd_one(dk_out, k, wk, cos, sin, text_len, eps, rope_mode, wrong))


# ------------------------------------------------------------------------------------------ gelu_tanh
GELU_C = 0.7978845608028654
_K1, _K2 = np.float32(-2.302208198), np.float32(-0.1029432396)


def gelu_ref64(x, dy=None):
    """-> (value, dy * derivative) fp64 of gelu(approximate="tanh"), written as x sigmoid(2z), z = c (x + 0.044715 x^3): the same function as
    0.5 x (1 + tanh z), which in fp64 cancels to 0 below x = -8.3 where the value is still 1e-16 and a bf16 result has 8 good bits of it"""
    xx = _t64(x).clone().requires_grad_(True)
    y = xx * torch.sigmoid(2.0 * GELU_C * (xx + 0.044715 * xx ** 3))
    if dy is None:
        return y.detach(), None
    y.backward(_t64(dy))
    return y.detach(), xx.grad


def _gelu_parts64(x):
    x = _t64(x)
    t = -2.0 * GELU_C * math.log2(math.e) * x * (1.0 + 0.044715 * x * x)
    s = torch.sigmoid(-t * math.log(2.0))
    R = 3.0 + (1.0 - s) * (2.0 + 3.5 * t.abs())
    return x, s, R


def gelu_fwd_tol(x, ref):
    _, _, R = _gelu_parts64(x)
    return bf16_tol(ref, (R + 1.0) * U * ref.abs() + (_t64(x).abs() + 1.0) * GELU_SUB)


def gelu_bwd_tol(x, dy, ref):
    x, s, R = _gelu_parts64(x)
    dz2 = 2.0 * GELU_C * (1.0 + 3.0 * 0.044715 * x * x)
    b = s * (1.0 - s)
    c = x * b * dz2
    rest = U * _t64(dy).abs() * (R * s + x.abs() * dz2 * ((R + 1.0) * s + b) + 4.0 * c.abs() + 2.0 * (s + c).abs()) + (_t64(dy).abs() * (1.0 + x.abs() * dz2) + 1.0) * GELU_SUB
    return bf16_tol(ref, rest)


def _gelu_sig_f32(x, x2):
    with np.errstate(over="ignore"):
        return _ONE / (_ONE + np.exp2(x * (_K1 + _K2 * x2)))


def gelu_fwd_f32(x):
    x = f32(x)
    return bf16_round(x * _gelu_sig_f32(x, x * x))


def gelu_bwd_f32(x, dy, wrong=None):
    x, dy = f32(x), f32(dy)
    x2 = x * x
    sg = _gelu_sig_f32(x, x2)
    dz2 = np.float32(1.5957691216057308) + (np.float32(0.0) if wrong == "no_cubic" else np.float32(0.2140644488) * x2)
    return bf16_round(dy * (sg + x * (sg - sg * sg) * dz2))


# ------------------------------------------------------------------------------------------ DPO error means
def _loss_threads(N):
    return min(256, max(1, -(-N // 2048))) * 256


def dpo_adds_per_thread(N, vec_ok=True):
    T = _loss_threads(N)
    n8 = N // 8 if vec_ok else 0
    return 8 * -(-n8 // T) + -(-(N - 8 * n8) // T)


def dpo_errs_rel(N, vec_ok=True):
    return (dpo_adds_per_thread(N, vec_ok) + 4) * U


def dpo_errs_ref64(v_win, v_lose, v_win_ref, v_lose_ref, tgt_win, tgt_lose):
    """[B, 4] fp64 means of squared differences in the kernel's order (win, lose, win_ref, lose_ref)"""
    tw, tl = _t64(tgt_win).flatten(1), _t64(tgt_lose).flatten(1)
    return torch.stack([(_t64(v).flatten(1) - t).pow(2).mean(1) for v, t in ((v_win, tw), (v_lose, tl), (v_win_ref, tw), (v_lose_ref, tl))], 1)


def _thread_sums_f32(sq, T, vec_ok):
    """sq [N] float32 squares -> per-thread fp32 accumulators [T] in the kernel's order: chunks of 8 strided by T, then single elements strided by T"""
    N = sq.shape[0]
    n8 = N // 8 if vec_ok else 0
    acc = np.zeros(T, np.float32)
    if n8:
        it = -(-n8 // T)
        body = np.zeros((it * T, 8), np.float32)             # adding the +0 padding is exact
        body[:n8] = sq[:n8 * 8].reshape(n8, 8)
        body = body.reshape(it, T, 8)
        for i in range(it):
            for j in range(8):
                acc = acc + body[i, :, j]
    tail = sq[n8 * 8:]
    it = -(-tail.shape[0] // T)
    pad = np.zeros(it * T, np.float32)
    pad[:tail.shape[0]] = tail
    for row in pad.reshape(it, T):
        acc = acc + row
    return acc


def dpo_errs_f32(v_win, v_lose, v_win_ref, v_lose_ref, tgt_win, tgt_lose, vec_ok=True, wrong=None):
    """[B, 4] float32, the arithmetic of dpo_err_partial_kernel + the head of dpo_finish_kernel"""
    vs = [f32(t).reshape(t.shape[0], -1) for t in (v_win, v_lose, v_win_ref, v_lose_ref, tgt_win, tgt_lose)]
    B, N = vs[0].shape
    n_sum = N - 5 if wrong == "drop5" else N
    T = _loss_threads(N)
    out = np.zeros((B, 4), np.float32)
    for b in range(B):
        for kk, (v, t) in enumerate(((vs[0], vs[4]), (vs[1], vs[5]), (vs[2], vs[4]), (vs[3], vs[5]))):
            d = v[b, :n_sum] - t[b, :n_sum]
            out[b, kk] = np.float32(_thread_sums_f32(d * d, T, vec_ok).astype(np.float64).sum() / N)
    return out


# ------------------------------------------------------------------------------------------ AdamW, gradient norm
def _opt_threads(n):
    return min(1024, max(1, -(-(n // 4) // 256))) * 256


def grad_norm_rel(n):
    T = _opt_threads(n)
    k = -(-(n // 4) // T) + -(-(n % 4) // T)
    return ((4 + k) / 2.0 + 1.0) * U


def grad_norm_ref64(g, grad_scale):
    return float(_t64(g).pow(2).sum().sqrt()) * float(np.float32(grad_scale))


def grad_norm_f32(g, grad_scale):
    g = f32(g).ravel()
    n, T = g.shape[0], _opt_threads(g.shape[0])
    n4 = n // 4
    it = -(-n4 // T)
    body = np.zeros((it * T, 4), np.float32)
    body[:n4] = g[:n4 * 4].reshape(n4, 4)
    body = body.reshape(it, T, 4)
    acc = np.zeros(T, np.float32)
    for i in range(it):
        v = body[i]
        acc = acc + (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2] + v[:, 3] * v[:, 3])
    tail = np.zeros(T, np.float32)
    tail[:n - n4 * 4] = g[n4 * 4:]
    acc = acc + tail * tail
    return np.float32(math.sqrt(acc.astype(np.float64).sum()) * float(np.float32(grad_scale)))


def _hyper32(*v):
    return [float(np.float32(a)) for a in v]


def adamw_ref64(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_norm=0.0, total_norm=None):
    """-> (p', m', v') fp64: clip_grad_norm_ (coef = max_norm / (norm + 1e-6), clamped to 1) on grad_scale * g, then torch.optim.AdamW (decoupled decay,
    bias-corrected moments), from the fp32 buffers and the float hyper-parameters; total_norm is the fp32 value the kernel reads"""
    lr, beta1, beta2, eps, weight_decay, grad_scale, max_norm = _hyper32(lr, beta1, beta2, eps, weight_decay, grad_scale, max_norm)
    p, g, m, v = _t64(p), _t64(g), _t64(m), _t64(v)
    coef = grad_scale
    if max_norm > 0 and total_norm is not None:
        coef *= min(1.0, max_norm / (float(total_norm) + float(np.float32(1e-6))))
    gj = g * coef
    p = p * (1.0 - lr * weight_decay)
    m = beta1 * m + (1.0 - beta1) * gj
    v = beta2 * v + (1.0 - beta2) * gj * gj
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def adamw_tols(g, m, v, ref_m, ref_v, ref_p, beta1, beta2, grad_scale=1.0, max_norm=0.0, total_norm=None):
    """bounds of (p', m', v') around adamw_ref64's results; g, m, v are the buffers BEFORE the step"""
    beta1, beta2, grad_scale, max_norm = _hyper32(beta1, beta2, grad_scale, max_norm)
    coef = grad_scale
    if max_norm > 0 and total_norm is not None:
        coef *= min(1.0, max_norm / (float(total_norm) + 1e-6))
    tol_m = C_M * U * (beta1 * _t64(m).abs() + (1.0 - beta1) * (_t64(g) * coef).abs())
    return ADAMW_P_ATOL + ADAMW_P_RTOL * ref_p.abs(), tol_m, C_V * U * ref_v.abs()


def adamw_f32(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_norm=0.0, total_norm=None, wrong=None):
    """(p', m', v') float32, the arithmetic of adamw_kernel and of vgpa_adamw_step's bias corrections"""
    F = np.float32
    p, g, m, v = f32(p), f32(g), f32(m), f32(v)
    lr, beta1, beta2, eps, wd, gs, mn = (F(a) for a in (lr, beta1, beta2, eps, weight_decay, grad_scale, max_norm))
    bc1 = F(1.0 - float(beta1) ** step)
    bc2_sqrt = F(1.0) if wrong == "no_bc2" else F(math.sqrt(1.0 - float(beta2) ** step))
    coef = gs
    if mn > 0 and total_norm is not None:
        coef = coef * min(mn / (F(total_norm) + F(1e-6)), F(1.0))
    step_size = lr / bc1
    gj = g * coef
    decay = _ONE - lr * wd
    if wrong != "decay_after":
        p = p * decay
    m = beta1 * m + (_ONE - beta1) * gj
    v = beta2 * v + (_ONE - beta2) * gj * gj
    p = p - step_size * m / (np.sqrt(v) / bc2_sqrt + eps)
    if wrong == "decay_after":
        p = p * decay
    return p, m, v


# ------------------------------------------------------------------------------------------ input families shared by the host and the device tests
QK_SHAPES = [(1, 7, 3, 3), (2, 33, 2, 0), (2, 33, 2, 33), (1, 64, 2, 1), (3, 5, 5, 2)]        # (B, S, H, text_len)
QK_SCALE = 64 ** -0.5 * 1.4426950408889634


def rope_tables(kind, rope_mode, rows, gen):
    """kind "contract": what the models build, from random angles per row (mode 0 pair-repeated, mode 1 [y-angles x2 | x-angles x2]); "arbitrary":
    independent cos and sin per element in (-1, 1), a valid input of the linear map that tells table elements apart; None: no rotation"""
    if kind is None:
        return None, None
    if kind == "arbitrary":
        return tuple((2 * torch.rand(rows, 64, generator=gen) - 1).contiguous() for _ in range(2))
    ang = 2 * math.pi * torch.rand(rows, 32, generator=gen)
    if rope_mode == 0:
        ang = ang.repeat_interleave(2, dim=1)
    else:
        ang = torch.cat([ang[:, :16], ang[:, :16], ang[:, 16:], ang[:, 16:]], 1)
    return ang.cos().contiguous(), ang.sin().contiguous()


def qknorm_inputs(B, S, H, text_len, rope, rope_mode, seed=0):
    """qkv bf16 [B,S,3,H,64] (the fused projection's layout) of N(0, 1) * 1.7 + 0.3 with planted vectors in q and in k: 64 identical values (zero variance:
    output = bias, rstd = eps^-1/2), a single outlier of 200, and 63 ones with one value a bf16 step above (variance 9.4e-7, next to both eps values: the only
    vector on which 1e-5 and 1e-6 give visibly different results); weights 1 + 0.2 randn, biases 0.2 randn; tables [max(S - text_len, 1), 64]; gradients randn"""
    g = torch.Generator().manual_seed(1000 * seed + 97 * B + 13 * S + 5 * H + text_len + 7 * rope_mode)
    qkv = (torch.randn(B, S, 3, H, 64, generator=g) * 1.7 + 0.3).to(torch.bfloat16)
    near = torch.ones(64)
    near[9] = 1.0078125
    qkv[0, 0, 0, 0] = 0.75
    qkv[0, min(1, S - 1), 0, 0, 5] = 200.0
    qkv[B - 1, S - 1, 0, H - 1] = near.to(torch.bfloat16)
    qkv[0, S - 1, 1, H - 1] = -1.25
    qkv[B - 1, 0, 1, H - 1, 37] = 200.0
    qkv[0, 0, 1, 0] = near.to(torch.bfloat16)
    wq, wk = (1 + 0.2 * torch.randn(64, generator=g) for _ in range(2))
    bq, bk = (0.2 * torch.randn(64, generator=g) for _ in range(2))
    cos, sin = rope_tables(rope, rope_mode, max(S - text_len, 1), g)
    dq, dk = (torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16) for _ in range(2))
    return dict(qkv=qkv, wq=wq, bq=bq, wk=wk, bk=bk, cos=cos, sin=sin, dq=dq, dk=dk)


def bhs(qkv, i):
    """q (i = 0) / k (i = 1) of the fused buffer as a [B,H,S,64] view"""
    return qkv[:, :, i].permute(0, 2, 1, 3)


def gelu_inputs(n, seed=0):
    """bf16 [n]: 3 randn, with every bf16 value of [-12, 12] planted at the front (both saturations, the minimum near -0.75, the subnormals) and +-0 behind it;
    when n is too small for the ramp, only the +-0 at the end"""
    g = torch.Generator().manual_seed(seed + n)
    u = (3 * torch.randn(n, generator=g)).to(torch.bfloat16)
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    ramp = bits[bits.float().abs() <= 12.0]                       # NaN and inf drop out of the comparison
    ramp = ramp[torch.argsort(ramp.float(), stable=True)]
    if n >= ramp.numel() + 2:
        u[: ramp.numel()] = ramp
    u[-2:] = torch.tensor([0.0, -0.0]).to(torch.bfloat16)
    dy = torch.randn(n, generator=g).to(torch.bfloat16)
    return u, dy


N_MAX_DPO = 524288 + 2408


def dpo_inputs(B, N, dtype, seed=0):
    """six [B, N] tensors (v_win, v_lose, v_win_ref, v_lose_ref, tgt_win, tgt_lose): the policy within 0.05 randn of the reference.  Always drawn at
    N_MAX_DPO and cut, so that a shorter N is a truncation of a longer one with the same seed.  The targets of the last 8 columns of N_MAX_DPO are moved
    by 4: the elements that only the longer cases have (the scalar tail of 524 288 + 2 405) weigh about 18 each where the others weigh 2"""
    g = torch.Generator().manual_seed(seed)
    full = torch.randn(B, 6, N_MAX_DPO, generator=g)
    full[:, 2:4, N_MAX_DPO - 8:] += 4.0
    full = full[:, :, :N]
    ref_w, ref_l, tw, tl = full[:, 0], full[:, 1], full[:, 2], full[:, 3]
    out = [ref_w + 0.05 * full[:, 4], ref_l + 0.05 * full[:, 5], ref_w, ref_l, tw, tl]
    return [t.to(dtype).contiguous() for t in out]


ADAMW_HYPER = dict(lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8)       # lr 0.1: the order of decay and update then differs by lr^2 wd = 1e-4, ten times ADAMW_P_RTOL
ADAMW_COMBOS = [(3.0, 0.5, 1.0), (1e-4, 1.0, 1.0), (1.0, 1.0, 0.0)]   # (gradient std, grad_scale, max_norm): norm well above 1; below 1; no clipping, no norm


def adamw_state(n, seed=0):
    """-> p, grad, exp_avg, exp_avg_sq fp32 [n] and the slice of a block with exactly-zero gradient and zero moments (there the step is the decay alone)"""
    g = torch.Generator().manual_seed(seed + n)
    p, m = torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)
    v = (0.1 * torch.randn(n, generator=g)) ** 2
    gr = torch.randn(n, generator=g)
    z = slice(n // 3, n // 3 + max(1, n // 8))
    gr[z], m[z], v[z] = 0, 0, 0
    return p, gr, m, v, z
