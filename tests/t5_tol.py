"""Per-element bounds and float32 restatements of the two small kernels of csrc/t5.hip, in the manner of tests/row_tol.py (its units: u = 2^-24 the unit
roundoff of fp32, hardware rsq / exp2 / rcp 1 ulp = 2u, contraction into FMAs only removes roundings; `bf16_tol(ref, rest) = half_ulp_bf16(|ref| + rest) +
rest` for a bf16 store).  No number below was fitted to a device result; tests/test_t5_host.py shows on the CPU that the restatements stay inside and
that wrong variants do not; tests/test_gpu_t5.py holds the device to the same bounds.

T5 RMS row kernel (t5_rms_kernel, one wave per row of D <= 4096, NV = ceil(D / 512) chunks of 64 lanes x 8):
    x_new   = x + y: one correctly rounded fp32 addition of an fp32 and a bf16 value: |d x_new| <= u |x_new|  (nothing cancels: the bound is relative to the
              sum itself).  The gather writes float(table[id]) exactly.  The x_new OUTPUT is held to u |ref| (exact for the gather).
    rs      the squares 1u, their sum and the division by D  C_MEAN(D) u  (row_tol: 8 NV - 1 serial additions per lane, six in wave_sum, the division), + eps 1u,
              rsq 2u:  C_RMS(D) = C_MEAN(D) / 2 + 3 relative (row_tol.c_rms).  With the add, every square carries 2u more from x_new: + 1u on rs.
    n       (x_new [1u with the add] * rs [C_RMS u, + 1u with the add]) [1u] * w [1u]:
              rest = (C_RMS(D) + 2) u |n|  without the add,   (C_RMS(D) + 4) u |n|  with it
              fp32 output: tol = rest (the store is exact);  bf16 output: tol = bf16_tol(n, rest)
    eps is the float the C entry receives.  There is no mean, so there is no conditioning term K: every term of the sum of squares is non-negative.

Gated GELU (t5_gated_gelu_kernel): g = bf16(gelu(a) * b), gelu(a) = a * gelu_sig(a) of csrc/common.h.
    gelu    row_tol's value bound: rest_g = (R + 1) u |gelu(a)| + (|a| + 1) SUB,  R = 3 + (1 - s)(2 + 3.5 |t|)
    product rest = rest_g |b| + 1u |ref|;   tol = bf16_tol(ref, rest)"""
import numpy as np
import torch

import row_tol as rt
from row_tol import U, bf16_round, bf16_tol, f32


def rms_rest_coef(D, add):
    return rt.c_rms(D) + (4.0 if add else 2.0)


def rms_tol(ref_n, D, add, out_bf16):
    rest = rms_rest_coef(D, add) * U * ref_n.double().abs()
    return bf16_tol(ref_n.double(), rest) if out_bf16 else rest


def stream_tol(ref_x):
    return U * ref_x.double().abs()


def gated_gelu_tol(u, ref):
    F = u.shape[-1] // 2
    a, b = u[..., :F].double(), u[..., F:].double()
    _, _, R = rt._gelu_parts64(a)
    g = ref / torch.where(b == 0, torch.ones_like(b), b)                      # gelu(a) where b != 0; where b == 0 the term is multiplied by 0 anyway
    rest = ((R + 1.0) * U * g.abs() + (a.abs() + 1.0) * rt.GELU_SUB) * b.abs() + U * ref.abs()
    return bf16_tol(ref, rest)


# ---- float32 restatements (numpy, the order of operations of csrc/t5.hip); `wrong` names a deliberately wrong variant
def rms_f32(x, w, eps, y=None, out_bf16=True, wrong=None):
    """x fp32 [M,D] (or the gathered rows), y bf16-valued or None -> (x_new, n) as float32 arrays"""
    x, w = f32(x), f32(w)
    M, D = x.shape
    v = x + f32(y) if y is not None else x
    if wrong == "mean_sub":
        v_n = v - v.mean(-1, keepdims=True, dtype=np.float32)
    else:
        v_n = v
    NV = -(-D // 512)
    pad = np.zeros((M, NV * 512), np.float32)
    pad[:, :D] = v_n
    pad = pad.reshape(M, NV, 64, 8)
    acc = np.zeros((M, 64), np.float32)
    for c in range(NV):
        for j in range(8):
            acc = acc + pad[:, c, :, j] * pad[:, c, :, j]
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    ms = acc[:, :1] / np.float32(D)
    if wrong == "eps_outside":
        rs = np.float32(1.0) / (np.sqrt(ms) + np.float32(eps))
    else:
        rs = np.float32(1.0) / np.sqrt(ms + np.float32(eps))
    n = (v_n * rs) * w
    return v, (bf16_round(n) if out_bf16 else n)


def gated_gelu_f32(u, wrong=None):
    u = f32(u)
    F = u.shape[-1] // 2
    a, b = u[..., :F], u[..., F:]
    if wrong == "erf":
        import math
        ga = np.asarray([0.5 * t * (1.0 + math.erf(t / math.sqrt(2.0))) for t in a.ravel().astype(np.float64)], np.float32).reshape(a.shape)
    elif wrong == "swapped":
        a, b = b, a
        ga = a * rt._gelu_sig_f32(a, a * a)
    else:
        ga = a * rt._gelu_sig_f32(a, a * a)
    return bf16_round(ga * b)


# ---- input families shared by the host and the device tests
def rms_inputs(M, D, seed=0):
    """x fp32 [M,D] = N(0.3, 1.7) with every fourth row scaled by 1e-3 (mean square next to eps = 1e-6: the only rows on which eps inside and outside the
    root differ visibly) and a row of one outlier; y bf16 N(0, 1) (the rows follow x's scale); w = 1 + 0.3 U(-1, 1); ids and a bf16 table [97, D]"""
    g = torch.Generator().manual_seed(31 * M + D + seed)
    x = torch.randn(M, D, generator=g) * 1.7 + 0.3
    scale = torch.ones(M, 1)
    scale[0::4] = 1e-3
    x = x * scale
    if M > 1:
        x[1] = 0.0
        x[1, D // 3] = 200.0
    y = (torch.randn(M, D, generator=g) * scale).to(torch.bfloat16)
    w = 1.0 + 0.3 * (2.0 * torch.rand(D, generator=g) - 1.0)
    table = (torch.randn(97, D, generator=g) * 1.3 + 0.2).to(torch.bfloat16)
    table[5] = (table[5].float() * 1e-3).to(torch.bfloat16)
    ids = torch.randint(0, 97, (M,), generator=g)
    ids[0] = 5
    return x, y, w, table, ids


def gelu_inputs(M, F, seed=0):
    """u bf16 [M, 2F]: both halves span +-12 -- half of the values uniform in [-12, 12], half 3 N(0, 1) clamped to it -- with both saturations, the
    minimum near -0.75, where the sigmoid underflows (-10 and below) and +-0 planted at the front of each half"""
    g = torch.Generator().manual_seed(seed + 13 * M + F)
    special = torch.tensor([-12.0, 12.0, 0.0, -0.0, -0.75, -10.0, 10.0, -11.5, 1e-3, -1e-3])

    def half():
        t = torch.where(torch.rand(M, F, generator=g) < 0.5, 24.0 * torch.rand(M, F, generator=g) - 12.0, (3.0 * torch.randn(M, F, generator=g)).clamp(-12, 12))
        t[0, :special.numel()] = special[torch.randperm(special.numel(), generator=g)]
        return t.to(torch.bfloat16)

    a = half()
    a[0, :special.numel()] = special.to(torch.bfloat16)
    return torch.cat([a, half()], 1).contiguous()
