"""fp64 references, per-element bounds and float32 restatements of the small kernels of the training steps: QK-norm + RoPE
(csrc/qknorm.hip), gelu_tanh (csrc/norm.hip), the DPO error reduction (csrc/dpo_loss.hip), AdamW and the gradient norm (csrc/adamw.hip), and the
one-wave-per-row norm kernels over csrc/row_ln.h: CogVideoX LayerNorm + modulation with and without the residual add (csrc/norm.hip, csrc/residual_ln.hip),
Wan LayerNorm + per-token modulation, RMS-norm + RoPE and the gated residual add (csrc/wan.hip).
tests/test_row_tol_host.py shows on the CPU that the restatements stay inside the bounds and that wrong variants do not;
tests/test_gpu_step_kernels.py and tests/test_gpu_row_kernels.py hold the device to the same bounds.  No number below was fitted to a device result.

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

Row kernels (one wave per row of D <= 4096 columns, NV = ceil(D / 512) chunks of 64 lanes x 8).  The summation constants of the 64-wide vector become functions of D:
    sum     a lane adds its 8 NV values serially (8 NV - 1 additions, fewer in a partly filled last chunk), wave_sum adds six times (offsets 32..1):
            C_SUM(D) = 8 NV + 5 additions behind every element
    mean    the division by (float)D 1u:  |d mean| <= C_MEAN(D) u mean|x|,   C_MEAN(D) = 8 NV + 6                      (14 at NV 1, 70 at NV 8)
    rstd    x - mean 1u, the squares 2u + 1u, their sum C_SUM u, / D 1u: (C_MEAN + 3) u relative on the variance; + eps 1u; rsq 2u:
            C_RSTD(D) = (C_MEAN + 3) / 2 + 1/2 + 2 = C_MEAN(D) / 2 + 4.   The mean's own error d enters the variance as d^2 (sum of deviations = 0): relative to
            var + eps that is (C_MEAN u K)^2, K = mean|x| rstd as above -- nothing on ordinary rows, kept because a constant row has K = |c| eps^-1/2
    xhat    (x - mean) [1u] rstd [C_RSTD u + 1u]:  e_xhat = u ((C_RSTD + 2) |xhat_d| + C_MEAN K) + (C_MEAN u K)^2 / 2 |xhat_d|.  On a constant row xhat = 0
            and the K term is the whole bound: the device's xhat there is (c - mean') rstd, the mean's rounding times eps^-1/2
  CogVideoX forward (ln_modulate_fwd_kernel, residual_ln_fwd_kernel):  alpha = w s1p [1u], beta = b s1p [1u] + shift [1u of the sum], n = xhat alpha + beta
            rest_d = e_xhat |alpha_d| + u (|xhat_d alpha_d| [alpha] + |xhat_d alpha_d| [product] + |b_d s1p_d| + |beta_d| + |n_d| [sum]);   tol = bf16_tol(n, rest)
            mean and rstd are outputs and are judged with the two bounds above.  x' = bf16(x + bf16(gate y)) is a torch expression, bit for bit
  LayerNorm backward (ln_modulate_bwd_kernel, residual_ln_bwd_kernel, wan_ln_mod_bwd_kernel):  dx = [dres +] rstd (g - c1 - xhat c2) FROM THE fp32 mean / rstd THE FORWARD
            WROTE: they are the kernel's inputs, so the reference takes them as given and no K term appears.  g arrives with cg u |g| (CogVideoX: alpha 1u, dy alpha 1u:
            cg = 2, 0 without modulation; Wan: 1 + scale 1u, the product 1u, the product with w 1u)
    xhat    (x - mean) [1u] rstd [1u]: 2u |xhat|
    c1      (cg + C_MEAN) u mean|g|.      c2: terms (cg + 2 + 1) u, sum and division C_MEAN u:  (cg + 3 + C_MEAN) u mean|g xhat|
    dx      rstd [cg u |g| + d c1 + u |g - c1| + |xhat| d c2 + 3u |xhat c2| + u |g - c1 - xhat c2|] + u |d| (the product with rstd) [+ u |dres + d|]
            stored as bf16 (CogVideoX: bf16_tol) or as fp32 (Wan: the rest itself).  dy = bf16(gate dx) resp. dy_prev = bf16(dx gate_prev[g]) is one fp32 product of the
            STORED dx and one rounding: bit for bit with torch given the device's dx
  Wan forward (wan_ln_mod_fwd_kernel):  o = xhat, [round_bf16], o w + b, o (1 + scale[g]) + shift[g].  The reference is the unrounded expression; every step maps (v, e) to
            round_xhat   e + half_ulp_bf16(|v| + e)
            affine       e |w| + u |v w| + u |v w + b|
            modulation   e |1 + s| + 2u |v (1 + s)| (1 + s and the product) + u |v (1 + s) + shift|
            and the store is bf16_tol(ref, e), or e + u |ref| for the fp32 result.  A missing round_xhat stays inside that bound (its half ulp is part of it), so the
            device test also holds bf16((x - mean') rstd'), two exactly rounded fp32 operations from the device's own mean' and rstd', bit for bit
  RMS-norm + RoPE (wan_rms_rope_*_kernel):  the squares 1u, sum and division C_MEAN u, + eps 1u, rsq 2u:  rs is off by C_RMS(D) = C_MEAN(D) / 2 + 3 (judged as rstd_out)
    forward n = bf16(u rs): e = (C_RMS + 1) u |n| + its half ulp;  y = bf16(n w): e |w| + u |n w| + its half ulp;  rotation (a, b) -> (a cos - b sin, a sin + b cos):
            e_a |cos| + e_b |sin| + 2u (|a cos| + |b sin|);  store.  Without tables y is the output (its half ulp is the store's) and must also equal
            bf16(bf16(u rs') w) formed in torch fp32 from the device's rs', bit for bit
    backward du = bf16(rs (dn - n m)), dn = w R^T dout [cg = 3: rotation 2u, w 1u, of G = (|a cos| + |b sin|) |w|; 1 without tables], n = u rs [1u], m = mean(dn n):
            d m = (cg + 2 + C_MEAN) u mean(G |n|);   rest = rs [cg u G + |n| d m + 2u |n m| + u |dn - n m|] + u |du|,  from the rs the forward wrote
  gate_residual (Wan, fp32):  x + y gate[g] is a product and an add or one FMA: 2u (|x| + |y g|).  gate_bwd is one product and one rounding: bit for bit.

The CogVideoX gate_residual, x' of the residual + LayerNorm pass, dy = bf16(gate dx), the Wan gate_bwd and the noise kernels are bit-exact with a torch expression;
they need no bound."""
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


# ------------------------------------------------------------------------------------------ one-wave-per-row norm kernels (csrc/row_ln.h and its three users)
def nv_of(D):
    return -(-D // 512)


def c_sum(D):
    """fp32 additions behind one element of a row sum: 8 NV - 1 serial per lane, six in wave_sum"""
    return 8.0 * nv_of(D) + 5.0


def c_mean(D):
    return c_sum(D) + 1.0


def c_rstd(D):
    return c_mean(D) / 2.0 + 4.0


def c_rms(D):
    return c_mean(D) / 2.0 + 3.0


def _eps32(eps):
    return float(np.float32(eps))


def row_stats64(x, eps):
    """x [..., D] -> mean, rstd [..., 1], xhat, K = mean|x| rstd   (fp64, eps as the float the C entry receives)"""
    x = _t64(x)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = (d.pow(2).mean(-1, keepdim=True) + _eps32(eps)).rsqrt()
    return mean, rstd, d * rstd, x.abs().mean(-1, keepdim=True) * rstd


def stats_tols(x, eps):
    """bounds of the mean / rstd outputs ([..., 1]) and of the computed xhat ([..., D]) of a LayerNorm forward"""
    D = x.shape[-1]
    _, rstd, xh, K = row_stats64(x, eps)
    second = 0.5 * (c_mean(D) * U * K) ** 2
    tol_mean = c_mean(D) * U * _t64(x).abs().mean(-1, keepdim=True)
    tol_rstd = rstd * (c_rstd(D) * U + second)
    e_xhat = U * ((c_rstd(D) + 2.0) * xh.abs() + c_mean(D) * K) + second * xh.abs()
    return tol_mean, tol_rstd, e_xhat


def cog_rows(tab_v, tab_t, B, S, Lt, wrong=None):
    """per-range [B, D] tables -> [B, S, D]: rows s < Lt take the text table.  wrong "text_first_video": the first video row of every sample takes the text table"""
    s = torch.arange(S, device=tab_v.device)
    text = s < (Lt + 1 if wrong == "text_first_video" and 0 < Lt < S else Lt)
    return torch.where(text[None, :, None], tab_t[:, None, :], tab_v[:, None, :])


def cog_ln_fwd_ref64(xn, w, b, s1p, shift, eps):
    """xn [B,S,D] the LayerNorm input; s1p / shift [B,S,D] (cog_rows) or None -> n, mean, rstd fp64"""
    mean, rstd, xh, _ = row_stats64(xn, eps)
    alpha = _t64(w) if s1p is None else _t64(w) * _t64(s1p)
    beta = _t64(b) if s1p is None else _t64(b) * _t64(s1p) + _t64(shift)
    return xh * alpha + beta, mean.squeeze(-1), rstd.squeeze(-1)


def cog_ln_fwd_tol(xn, w, b, s1p, shift, eps, ref_n):
    """-> bounds of n (bf16 store), mean, rstd"""
    tol_mean, tol_rstd, e_xh = stats_tols(xn, eps)
    _, _, xh, _ = row_stats64(xn, eps)
    w, b = _t64(w), _t64(b)
    if s1p is None:
        alpha, e_alpha, e_beta = w, 0.0, 0.0
    else:
        alpha = w * _t64(s1p)
        e_alpha = U * alpha.abs()
        e_beta = U * ((b * _t64(s1p)).abs() + (b * _t64(s1p) + _t64(shift)).abs())
    rest = e_xh * alpha.abs() + xh.abs() * e_alpha + U * (xh * alpha).abs() + e_beta + U * ref_n.abs()
    return bf16_tol(ref_n, rest), tol_mean.squeeze(-1), tol_rstd.squeeze(-1)


def ln_bwd_ref64(g, x, mean, rstd, dres=None):
    """g = the incoming gradient times the affine (fp64, [..., D]); mean / rstd [...] as the forward wrote them -> rstd (g - c1 - xhat c2) [+ dres]"""
    g, mean, rstd = _t64(g), _t64(mean).unsqueeze(-1), _t64(rstd).unsqueeze(-1)
    xh = (_t64(x) - mean) * rstd
    c1, c2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    d = rstd * (g - c1 - xh * c2)
    return d if dres is None else d + _t64(dres)


def ln_bwd_rest(g, x, mean, rstd, cg, dres=None):
    """fp32 error of ln_bwd_ref64's expression; cg u |g| is the error g arrives with"""
    D = x.shape[-1]
    g, mean, rstd = _t64(g), _t64(mean).unsqueeze(-1), _t64(rstd).unsqueeze(-1)
    xh = (_t64(x) - mean) * rstd
    c1, c2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    e_c1 = (cg + c_mean(D)) * g.abs().mean(-1, keepdim=True)
    e_c2 = (cg + 3.0 + c_mean(D)) * (g * xh).abs().mean(-1, keepdim=True)
    inner = g - c1 - xh * c2
    e = cg * g.abs() + e_c1 + (g - c1).abs() + xh.abs() * e_c2 + 3.0 * (xh * c2).abs() + inner.abs()
    rest = U * rstd.abs() * (e + inner.abs())
    if dres is not None:
        rest = rest + U * (rstd * inner + _t64(dres)).abs()
    return rest


def wan_ln_fwd_ref64(x, gid, w, b, shift, scale, eps):
    """x [rows, D]; shift / scale [G, D] views of the table, gid [rows] or None (row 0) -> out, mean, rstd fp64 (round_xhat is not part of the reference)"""
    mean, rstd, o, _ = row_stats64(x, eps)
    if w is not None:
        o = o * _t64(w) + _t64(b)
    if scale is not None:
        gi = torch.zeros(x.shape[0], dtype=torch.long, device=x.device) if gid is None else gid.long()
        o = o * (1.0 + _t64(scale)[gi]) + _t64(shift)[gi]
    return o, mean.squeeze(-1), rstd.squeeze(-1)


def wan_ln_fwd_tol(x, gid, w, b, shift, scale, eps, round_xhat, ref, out_bf16=True):
    tol_mean, tol_rstd, e = stats_tols(x, eps)
    _, _, v, _ = row_stats64(x, eps)
    if round_xhat:
        e = e + half_ulp_bf16(v.abs() + e)
    if w is not None:
        w, b = _t64(w), _t64(b)
        e = e * w.abs() + U * (v * w).abs() + U * (v * w + b).abs()
        v = v * w + b
    if scale is not None:
        gi = torch.zeros(x.shape[0], dtype=torch.long, device=x.device) if gid is None else gid.long()
        s1 = 1.0 + _t64(scale)[gi]
        e = e * s1.abs() + 2.0 * U * (v * s1).abs() + U * (v * s1 + _t64(shift)[gi]).abs()
    tol = bf16_tol(ref, e) if out_bf16 else e + U * ref.abs()
    return tol, tol_mean.squeeze(-1), tol_rstd.squeeze(-1)


def wan_ln_bwd_g64(dy, gid, w, scale):
    """-> g = dy (1 + scale[g]) w in fp64 and cg, the roundings it carries in the kernel (1 + scale, the product; the product with w)"""
    g, cg = _t64(dy), 0.0
    if scale is not None:
        gi = torch.zeros(dy.shape[0], dtype=torch.long, device=dy.device) if gid is None else gid.long()
        g, cg = g * (1.0 + _t64(scale)[gi]), cg + 2.0
    if w is not None:
        g, cg = g * _t64(w), cg + 1.0
    return g, cg


def _rope_rows(cos, sin, rows, L, D, head_dim, device):
    """tables [L, head_dim / 2] -> per-row, per-pair [rows, D / 2] fp64"""
    r = torch.arange(rows, device=device) % L
    rep = D // head_dim
    return _t64(cos).to(device)[r].repeat(1, rep), _t64(sin).to(device)[r].repeat(1, rep)


def _rot64(y, cs, sn, transpose=False):
    a, b = y[:, 0::2], y[:, 1::2]
    if transpose:
        return torch.stack([a * cs + b * sn, -a * sn + b * cs], -1).flatten(1)
    return torch.stack([a * cs - b * sn, a * sn + b * cs], -1).flatten(1)


def rms_rope_ref64(u, w, cos, sin, L, head_dim, eps):
    """u [rows, D] -> out, rs fp64: u rs w rotated, nothing rounded"""
    u = _t64(u)
    rs = (u.pow(2).mean(-1, keepdim=True) + _eps32(eps)).rsqrt()
    y = u * rs * _t64(w)
    if cos is not None:
        y = _rot64(y, *_rope_rows(cos, sin, u.shape[0], L, u.shape[1], head_dim, u.device))
    return y, rs.squeeze(-1)


def rms_rope_fwd_tol(u, w, cos, sin, L, head_dim, eps, ref):
    """n = bf16(u rs) and y = bf16(n w) each add their half ulp; the rotation carries both through |cos|, |sin|; then the store"""
    u, w = _t64(u), _t64(w)
    D = u.shape[1]
    rs = (u.pow(2).mean(-1, keepdim=True) + _eps32(eps)).rsqrt()
    n = u * rs
    e = (c_rms(D) + 1.0) * U * n.abs()
    e = e + half_ulp_bf16(n.abs() + e)
    e = e * w.abs() + U * (n * w).abs()
    tol_rs = (c_rms(D) * U * rs).squeeze(-1)
    if cos is None:
        return bf16_tol(ref, e), tol_rs
    y = n * w
    e = e + half_ulp_bf16(y.abs() + e)
    cs, sn = (t.abs() for t in _rope_rows(cos, sin, u.shape[0], L, D, head_dim, u.device))
    ya, yb, ea, eb = y[:, 0::2].abs(), y[:, 1::2].abs(), e[:, 0::2], e[:, 1::2]
    rest = torch.stack([ea * cs + eb * sn + 2.0 * U * (ya * cs + yb * sn), ea * sn + eb * cs + 2.0 * U * (ya * sn + yb * cs)], -1).flatten(1)
    return bf16_tol(ref, rest), tol_rs


def rms_rope_bwd_ref64(dout, u, rs, w, cos, sin, L, head_dim):
    """du = rs (dn - n mean(dn n)), dn = w R^T dout, n = u rs, from the fp32 rs the forward wrote"""
    dn, u, rs = _t64(dout), _t64(u), _t64(rs).unsqueeze(-1)
    if cos is not None:
        dn = _rot64(dn, *_rope_rows(cos, sin, u.shape[0], L, u.shape[1], head_dim, u.device), transpose=True)
    dn = dn * _t64(w)
    n = u * rs
    return rs * (dn - n * (dn * n).mean(-1, keepdim=True))


def rms_rope_bwd_tol(dout, u, rs, w, cos, sin, L, head_dim, ref):
    g, u, rs, w = _t64(dout), _t64(u), _t64(rs).unsqueeze(-1), _t64(w)
    D = u.shape[1]
    if cos is None:
        dn, G, cg = g * w, (g * w).abs(), 1.0
    else:
        cs, sn = _rope_rows(cos, sin, u.shape[0], L, D, head_dim, u.device)
        dn = _rot64(g, cs, sn, transpose=True) * w
        a, b = g[:, 0::2].abs(), g[:, 1::2].abs()
        G, cg = torch.stack([a * cs.abs() + b * sn.abs(), a * sn.abs() + b * cs.abs()], -1).flatten(1) * w.abs(), 3.0
    n = u * rs
    m = (dn * n).mean(-1, keepdim=True)
    e_m = (cg + 2.0 + c_mean(D)) * (G * n.abs()).mean(-1, keepdim=True)
    inner = dn - n * m
    rest = U * rs * (cg * G + n.abs() * e_m + 2.0 * (n * m).abs() + inner.abs()) + U * ref.abs()
    return bf16_tol(ref, rest)


def wan_gate_ref64(x, y, gid, gate):
    """x + y gate[g] fp64 and its bound 2u (|x| + |y g|): a product and an add, or one FMA"""
    p = _t64(y)
    if gate is not None:
        gi = torch.zeros(y.shape[0], dtype=torch.long, device=y.device) if gid is None else gid.long()
        p = p * _t64(gate)[gi]
    ref = p if x is None else _t64(x) + p
    return ref, 2.0 * U * (p.abs() + (0.0 if x is None else _t64(x).abs()))


# ---- float32 restatements of the row kernels
def _row_sum_f32(t, D, wrong=None):
    """t [rows, D] float32 -> the row sums [rows, 1] in a wave's order (lane l adds elements (64 c + l) 8 .. + 7 of chunk c = 0 .. NV - 1 serially, then
    v += shfl_xor(v, 32 .. 1)), divided by D.  wrong "mask8": the last valid group of eight is left out; "div_nv": divided by 512 NV"""
    rows, NV = t.shape[0], nv_of(D)
    pad = np.zeros((rows, NV * 512), np.float32)              # adding the +0 padding is exact
    pad[:, :D] = t
    if wrong == "mask8":
        pad[:, D - 8:D] = 0
    pad = pad.reshape(rows, NV, 64, 8)
    acc = np.zeros((rows, 64), np.float32)
    for c in range(NV):
        for j in range(8):
            acc = acc + pad[:, c, :, j]
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ m]
    return (acc[:, :1] / np.float32(512 * NV if wrong == "div_nv" else D)).astype(np.float32)


def _ln_stats_f32(x, eps, wrong=None):
    """x [rows, D] float32 -> mean, rstd [rows, 1]: the exact two-pass form of the kernels"""
    D = x.shape[1]
    mean = _row_sum_f32(x, D, wrong)
    d = x - mean
    var = _row_sum_f32(d * d, D, wrong)
    return mean, (_ONE / np.sqrt(var + np.float32(eps))).astype(np.float32)


def cog_ln_fwd_f32(xn, w, b, s1p, shift, eps, wrong=None):
    """xn [B,S,D]; s1p / shift [B,S,D] or None -> n (bf16 values), mean, rstd [B,S] float32"""
    shape = xn.shape
    x = f32(xn).reshape(-1, shape[-1])
    mean, rstd = _ln_stats_f32(x, eps, wrong)
    if s1p is None:
        alpha, beta = f32(w), f32(b)
    else:
        s = f32(s1p).reshape(x.shape)
        alpha, beta = f32(w) * s, f32(b) * s + f32(shift).reshape(x.shape)
    n = (x - mean) * rstd * alpha + beta
    return bf16_round(n).reshape(shape), mean.reshape(shape[:-1]), rstd.reshape(shape[:-1])


def ln_bwd_f32(g, x, mean, rstd, dres=None, wrong=None):
    """g [rows, D] float32 (already times the affine) -> rstd (g - c1 - xhat c2) [+ dres], float32, unrounded.  wrong "no_c1": without c1"""
    D = x.shape[1]
    mean, rstd = f32(mean).reshape(-1, 1), f32(rstd).reshape(-1, 1)
    xh = (x - mean) * rstd
    c1 = _row_sum_f32(g, D, wrong)
    c2 = _row_sum_f32(g * xh, D, wrong)
    if wrong == "no_c1":
        c1 = np.zeros_like(c1)
    d = rstd * (g - c1 - xh * c2)
    return d if dres is None else f32(dres).reshape(d.shape) + d


def cog_ln_bwd_f32(dn, xn, mean, rstd, w, s1p, dres=None, wrong=None):
    """-> dx (bf16 values) [B,S,D]"""
    shape = xn.shape
    alpha = f32(w) if s1p is None else f32(w) * f32(s1p).reshape(-1, shape[-1])
    g = f32(dn).reshape(-1, shape[-1]) * alpha
    return bf16_round(ln_bwd_f32(g, f32(xn).reshape(-1, shape[-1]), mean, rstd, dres, wrong)).reshape(shape)


def _gid_np(gid, rows, wrong=None):
    gi = np.zeros(rows, np.int64) if gid is None else np.asarray(gid.cpu() if torch.is_tensor(gid) else gid).astype(np.int64)
    if wrong == "gid_neighbour" and rows > 1:                    # one row reads its neighbour's group
        r = rows // 2
        gi = gi.copy()
        gi[r] = gi[r - 1]
    return gi


def wan_ln_fwd_f32(x, gid, w, b, shift, scale, eps, round_xhat, out_bf16=True, wrong=None):
    x = f32(x)
    mean, rstd = _ln_stats_f32(x, eps, wrong)
    o = (x - mean) * rstd
    if round_xhat and wrong != "no_round":
        o = bf16_round(o)
    if w is not None:
        o = o * f32(w) + f32(b)
    if scale is not None:
        gi = _gid_np(gid, x.shape[0], wrong)
        o = o * (_ONE + f32(scale)[gi]) + f32(shift)[gi]
    return (bf16_round(o) if out_bf16 else o), mean[:, 0], rstd[:, 0]


def wan_ln_bwd_f32(dy, x, mean, rstd, gid, w, scale, dres=None, wrong=None):
    """-> dx float32.  wrong "scale_no1p": scale where 1 + scale belongs"""
    g, x = f32(dy), f32(x)
    if scale is not None:
        s = f32(scale)[_gid_np(gid, x.shape[0], wrong)]
        g = g * (s if wrong == "scale_no1p" else _ONE + s)
    if w is not None:
        g = g * f32(w)
    return ln_bwd_f32(g, x, mean, rstd, dres, wrong)


def _rope_rows_f32(cos, sin, rows, L, D, head_dim, wrong=None):
    r = np.arange(rows)
    r = np.minimum(r, L - 1) if wrong == "row_no_mod" else r % L          # `row` in place of `row % L` (clamped here to the table a device would run past)
    rep = D // head_dim
    return np.tile(f32(cos)[r], (1, rep)), np.tile(f32(sin)[r], (1, rep))


def rms_rope_fwd_f32(u, w, cos, sin, L, head_dim, eps, wrong=None):
    """-> out (bf16 values), rs [rows] float32.  wrong "per_head": the mean of squares taken over each head"""
    u, w = f32(u), f32(w)
    rows, D = u.shape
    if wrong == "per_head":
        uh = u.reshape(rows * (D // head_dim), head_dim)
        ms = np.repeat(_row_sum_f32(uh * uh, head_dim).reshape(rows, D // head_dim), head_dim, axis=1)
    else:
        ms = _row_sum_f32(u * u, D, wrong)
    rs = (_ONE / np.sqrt(ms + np.float32(eps))).astype(np.float32)
    y = bf16_round(bf16_round(u * rs) * w)
    if cos is not None:
        cs, sn = _rope_rows_f32(cos, sin, rows, L, D, head_dim, wrong)
        a, b = y[:, 0::2], y[:, 1::2]
        y = np.stack([a * cs - b * sn, a * sn + b * cs], -1).reshape(rows, D)
    return bf16_round(y), rs[:, 0]


def rms_rope_bwd_f32(dout, u, rs, w, cos, sin, L, head_dim, wrong=None):
    """-> du (bf16 values).  wrong "no_transpose": the forward's rotation applied to the gradient"""
    dn, u, w, rs = f32(dout), f32(u), f32(w), f32(rs).reshape(-1, 1)
    rows, D = u.shape
    if cos is not None:
        cs, sn = _rope_rows_f32(cos, sin, rows, L, D, head_dim, wrong)
        a, b = dn[:, 0::2], dn[:, 1::2]
        if wrong == "no_transpose":
            dn = np.stack([a * cs - b * sn, a * sn + b * cs], -1).reshape(rows, D)
        else:
            dn = np.stack([a * cs + b * sn, -a * sn + b * cs], -1).reshape(rows, D)
    dn = dn * w
    n = u * rs
    m = _row_sum_f32(dn * n, D, wrong)
    return bf16_round(rs * (dn - n * m))


def wan_gate_f32(x, y, gid, gate, wrong=None):
    p = f32(y)
    if gate is not None:
        p = p * f32(gate)[_gid_np(gid, p.shape[0], wrong)]
    return p if x is None else f32(x) + p


# ---- cases shared by tests/test_row_tol_host.py and tests/test_gpu_row_kernels.py
ROW_WIDTHS = [8, 512, 520, 1024, 1288, 2048, 2560, 3072, 3080, 4088, 4096]          # NV 1, 1, 2, 2, 3, 4, 5, 6, 7, 8, 8: full and partly filled last chunks alternate
COG_LAYOUTS = [(2, 37, 6), (3, 70, 33), (2, 33, 0), (2, 33, 33), (3, 5, 2)]          # (B, S, text_len)
WAN_LN_WIDTHS, WAN_LN_ROWS = [8, 264, 520, 3072, 4088, 4096], [1, 5, 9]
RMS_SHAPES = [(264, 24), (264, 8), (520, 40), (3072, 128), (4096, 128)]               # (D, head_dim)
RMS_L, RMS_B = 7, 3
_GID_CYCLE = [2, 0, 1, 0, 2, 1, 1, 2, 0]


def cog_layouts(D):
    """the two large layouts at every width, the three small ones where a row is cheap"""
    return COG_LAYOUTS if D <= 1288 else COG_LAYOUTS[:2]


def plant_rows(x2):
    """x2 [rows, D] float, in place; -> the planted row indices.  Last row: values of 0.01 and a single 200 in the last valid group of eight columns; row 0
    (from two rows): the constant 0.3, variance 0; row 1 (from three rows): zeros"""
    rows, D = x2.shape
    x2[rows - 1] *= 0.005
    x2[rows - 1, D - 3] = 200.0
    idx = [rows - 1]
    if rows >= 2:
        x2[0] = 0.3
        idx.append(0)
    if rows >= 3:
        x2[1] = 0.0
        idx.append(1)
    return idx


def cog_case(B, S, Lt, D, seed=0):
    """x, y, dn, dres bf16 [B,S,D] (x = 2 randn + 0.3 with plant_rows, y zero in the planted rows so that they reach the LayerNorm), gates [B,2,D] = (video, text),
    mod [B,4,D] = (shift_v, 1 + scale_v, shift_t, 1 + scale_t), w, b"""
    g = torch.Generator().manual_seed(7919 * seed + 131 * B + 17 * S + 3 * Lt + D)
    x = torch.randn(B, S, D, generator=g) * 2 + 0.3
    y = torch.randn(B, S, D, generator=g)
    y.view(-1, D)[plant_rows(x.view(-1, D))] = 0
    gates = torch.randn(B, 2, D, generator=g)
    w, b = 1 + 0.2 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    mod = 0.3 * torch.randn(B, 4, D, generator=g)
    mod[:, 1] += 1
    mod[:, 3] += 1
    dn, dres = (torch.randn(B, S, D, generator=g).to(torch.bfloat16) for _ in range(2))
    return dict(x=x.to(torch.bfloat16), y=y.to(torch.bfloat16), gates=gates, w=w, b=b, mod=mod, dn=dn, dres=dres)


def cog_x_new(c, B, S, Lt):
    """bf16(x + bf16(gate y)): the torch expression the forward's residual stream must equal bit for bit"""
    gfull = cog_rows(c["gates"][:, 0], c["gates"][:, 1], B, S, Lt)
    return c["x"] + (gfull * c["y"].float()).to(torch.bfloat16)


def wan_ln_case(rows, D, xdt=torch.float32, seed=0):
    """x [rows, D] of xdt with plant_rows; gid over 3 groups, not monotone; tab [3,6,D] (0.5 randn: columns 2 gate, 3 shift, 4 scale, 5 gate_prev); w, b;
    y bf16 (zero in the planted rows); dy bf16 and fp32; dres fp32"""
    g = torch.Generator().manual_seed(104729 * seed + 31 * rows + D + (5 if xdt == torch.float32 else 0))
    x = torch.randn(rows, D, generator=g) * 2 + 0.3
    y = torch.randn(rows, D, generator=g)
    y[plant_rows(x)] = 0
    gid = torch.tensor([_GID_CYCLE[i % 9] for i in range(rows)], dtype=torch.int32)
    tab = 0.5 * torch.randn(3, 6, D, generator=g)
    w, b = torch.randn(D, generator=g), torch.randn(D, generator=g)
    dy32 = torch.randn(rows, D, generator=g)
    dres = torch.randn(rows, D, generator=g)
    return dict(x=x.to(xdt), y=y.to(torch.bfloat16), gid=gid, tab=tab, w=w, b=b, dy=dy32.to(torch.bfloat16), dy32=dy32, dres=dres)


def rms_case(D, head_dim, seed=0):
    """u, dout bf16 [RMS_B RMS_L, D] (u with plant_rows), w bf16, cos / sin [RMS_L, head_dim / 2] of random angles"""
    rows = RMS_B * RMS_L
    g = torch.Generator().manual_seed(15485863 * seed + D + head_dim)
    u = torch.randn(rows, D, generator=g) * 2 + 0.3
    plant_rows(u)
    w = (1 + 0.2 * torch.randn(D, generator=g)).to(torch.bfloat16)
    ang = 2 * math.pi * torch.rand(RMS_L, head_dim // 2, generator=g)
    dout = torch.randn(rows, D, generator=g).to(torch.bfloat16)
    return dict(u=u.to(torch.bfloat16), w=w, cos=ang.cos().contiguous(), sin=ang.sin().contiguous(), dout=dout)
