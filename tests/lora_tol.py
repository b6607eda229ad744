"""fp64 references, per-element bounds, float32 restatements and the shared case lists of the LoRA kernels of csrc/lora.hip: `down` (lora_down_dma_kernel<NCB, 4>
for R <= 64, lora_down_kernel<NCB> above), `up_add`, `grad` (+ the ordered merge) and the adapter refresh.  tests/test_lora_tol_host.py shows on the CPU that the
restatements stay inside the bounds and that wrong variants do not; tests/test_gpu_lora_kernels.py holds the device to the same bounds and, on integer data, to
equality.  No number below was fitted to a device result.

Units.  u = 2^-24 (row_tol.U).  A product of two bf16 values has at most 16 significant bits: it is exact in fp32, so only additions round.  `mfma32` of
csrc/mfma_tiles.h is v_mfma_f32_32x32x16_bf16: one issue adds MFMA_K = 16 products to every accumulator element.  How the matrix pipe rounds the additions inside an
issue is not stated in the public ISA text, so the bounds take the pessimistic reading: every one of the n - 1 additions behind an element truncates, 2u of the
partial sum it produces, and every partial sum is at most S = sum |terms| (from the fp64 reference as |x| @ |a|^T, one more product):

    rest_sum(n, S) = min(2 (n - 1), 6 * 2/sqrt(3) * sqrt(n)) * u * S

The first arm holds for any order of summation.  The second is six standard deviations of n independent roundings, each uniform over a width of 2u S (standard
deviation 2u S / sqrt(12) = u S / sqrt(3); the factor 2 keeps a truncation's mean inside the band): the two-tier form of attn_tol.lse2_tol.  It decides from n = 14.

    down     T = bf16(sum_k x a), n = K:                tol = bf16_tol(ref, rest_sum(K, S))
    up_add   Y = bf16([y +] s * sum_r t b), n = rp; the product with s 1u, the add with y 1u (only when accumulate is set: without it nothing is added):
                                                        rest = rest_sum(rp, |s| S) + u |s sum t b| [+ u |ref|];  tol = bf16_tol(ref, rest)
    grad     G = s * sum_splits sum_rows u v (fp32), n = M: the MFMA chains of the splits and the merge in slab order are M - 1 additions in all (the first addition
             of a chain and of the merge is to an exact zero); the product with s 1u:
                                                        tol = rest_sum(M, |s| S) + u |ref|
    refresh  a = bf16(A), sB = bf16(float(bf16(B)) * s): the torch statements of ops.LoraExt.refresh's other branch, bit for bit; no bound.

Integer data.  With x in {-2, -1, 1, 2} and the rows of the second operand sparse in {-1, 0, 1}, every product, partial sum and result is an integer the output
type holds exactly (|.| <= 256 for bf16, <= 2^24 for grad; s a power of two), whatever the order or rounding mode: the result must EQUAL the int64 one.  Every index of
the contraction is hit by a non-zero of the sparse operand and no x is zero, so a dropped, doubled or misplaced term changes some result.

Restatements (numpy float32).  The accumulator takes one MFMA issue at a time -- the 16 products summed in fp64, added, one rounding to nearest: the most
favourable reading of the hardware, as the bound takes the least favourable -- along K (down), rp (up_add) or the token rows (grad, in chunks of 16 from the first
row of the split; rows at and past the split's end are zeros).  grad takes rows_per_split and the split count from `grad_plan`, the Python copy of lora_grad_plan,
adds the slabs in order and multiplies by s once; up_add multiplies by s in fp32, adds the unpacked y and rounds to bf16 once.

What reading the kernels says about the arguments the entries did not check (the header's rule is now: every row stride is at least the row's length):
    down   T: 8-byte stores at T + m ldt + n, n % 4 == 0, ldt % 8 == 0  -> T must be 8-byte aligned: refused otherwise.
           ldx < K: the register-staged kernel reads X + row ldx + col, col < K, and the DMA descriptor ends at (rows - 1) ldx + K, so a stride in [0, K) only makes
           rows overlap inside the caller's own extent -- but a negative stride makes the descriptor's length wrap to 4 GB and the register kernel read below X:
           refused with every ldx < K, which no caller has.
           the chunks the DMA ring requests past K: at most 3 x 128 bytes behind a row's K columns, inside the descriptor on every row but the block's last (there
           they are out of range and read as zeros): they are the caller's own bytes (the next row, or the padding / the T tail of the same row) and go to ring slots
           whose chunk index is >= nk.  The device test puts NaN there.
    up_add ldy < N: row-overlapping read-modify-writes from different workgroups race: refused.  ldt < rp, ldb < rp: in bounds for strides in [0, rp), below the base
           pointer for negative ones: refused alike.
    grad   ldg < Q: the merge kernel's rows overlap (a race); ldu < P, ldv < Q as above; G below 4-byte alignment is no float array: all refused.
    `mend` in lora_grad_kernel's tile_load_zfill: rows_per_split is a multiple of 64, so the 64-row tiles of every split but the last end exactly at its end, and the
           last split ends at M: passing M instead of mend changes no result (`grad_f32(wrong="grad_zfill_M")` is bit-identical, shown in the host file).  The bound is
           live only under a plan whose rows_per_split is no multiple of 64: that is what wrong="grad_split_overlap" restates.

Arms not reached: the register-staged kernel at NCB 1 and 2 (taken only when 64 ldx or R K pass the 32-bit descriptor range: more than 4 GB of X), the variant
builds (-DLORA_DOWN_DMA=0, -DLORA_DOWN_NS=3, the <6, 3> / <6, 4> DMA instantiations) and the atomicAdd branch of lora_grad_kernel (`part` is never NULL: the entry
refuses a NULL workspace).

Measured on the MI355X (largest |err| / bound over every case of tests/test_gpu_lora_kernels.py; restatement: the same over tests/test_lora_tol_host.py):
    down     device 0.997 (K = 3072: 0.905, mean 0.3: 0.948)    restatement 0.997 (K = 3072: 0.948)     the bf16 store decides
    up_add   device 0.999                                       restatement 0.999                       the bf16 store decides
    grad     device 0.011 .. 0.037 by (P, Q), mean 0.3: 0.028   restatement 0.022                       LOOSE, 27-fold: the bound lets every addition truncate a
             partial sum as large as S = sum |u v|, about 0.64 M, where the partial sums of N(0, 1) products are about sqrt(M) and the device (like the restatement)
             shows errors the size of a rounding to nearest.  Nothing tighter can be COUNTED without a statement of the matrix pipe's rounding, so it stays; 97.7 % of the
             single lost products at M = 1000 are still outside it (host file: the rest are products that are nearly zero), and the integer cases are exact.
    refresh  bit for bit
No kernel changed.  Mutated copies of lora.hip, run once on the device (never committed) -- new file | the LoRA tests of test_gpu_kernels.py as they were:
    nk = K / 64 - 1 in the DMA kernel            down[dma, tail, layouts, k3072] fail | raw x3, function_vs_torch, ext_padded fail
    `^ w1_swz(row)` dropped from ao[i]           down[dma, tail, layouts, k3072] fail | raw x3, function_vs_torch, ext_padded fail
    scalar else of both down epilogues removed   down[tail, layouts] fail             | all ten pass
    tile_load_zfill(.., M, ..) in the grad kernel  all pass                           | all ten pass     (changes no bit: see `mend` above)
    the accumulate read of up_add skipped        up_add fails                         | raw x4 fail
"""
import math

import numpy as np
import torch

from row_tol import U, _t64, bf16_round, bf16_tol, f32, half_ulp_bf16, judge, worst  # noqa: F401  (re-exported: the tests take them from here)

MFMA_K = 16                 # products one v_mfma_f32_32x32x16_bf16 adds to an accumulator element
GRAD_WGS = 768              # LORA_GRAD_WGS of the product build
UP_RANKS = [16, 32, 48, 64, 96, 128, 192]


def _cdiv(a, b):
    return -(-a // b)


def rest_sum(n, S):
    return min(2.0 * (n - 1), 6.0 * 2.0 / math.sqrt(3.0) * math.sqrt(n)) * U * S


# ------------------------------------------------------------------------------------------ references and bounds (torch fp64, on the operands' device)
def down_ref64(x, a):
    """-> ref = x a^T, S = |x| |a|^T"""
    x, a = _t64(x), _t64(a)
    return x @ a.t(), x.abs() @ a.abs().t()


def down_tol(ref, S, K):
    return bf16_tol(ref, rest_sum(K, S))


def up_ref64(y, t, b, s):
    """y None = accumulate off -> ref, dot = t b^T, S = |t| |b|^T"""
    t, b = _t64(t), _t64(b)
    dot = t @ b.t()
    return (s * dot if y is None else _t64(y) + s * dot), dot, t.abs() @ b.abs().t()


def up_tol(ref, dot, S, s, rp, accumulate):
    rest = rest_sum(rp, abs(s) * S) + U * (s * dot).abs()
    if accumulate:
        rest = rest + U * ref.abs()
    return bf16_tol(ref, rest)


def grad_ref64(u, v, s):
    u, v = _t64(u), _t64(v)
    return s * (u.t() @ v), u.abs().t() @ v.abs()


def grad_tol(ref, S, s, M):
    return rest_sum(M, abs(s) * S) + U * ref.abs()


def grad_plan(M, P, Q):
    """Python copy of lora_grad_plan -> dict(n_pt, n_qt, sp (the split count aimed at), rows (per split), splits, regime, last (rows of the last split)).
    regime: "one" split; "rows": capped by ceil(M / 256); "target": capped by GRAD_WGS / tiles"""
    n_pt, n_qt = _cdiv(P, 64), _cdiv(Q, 64)
    sp_t = max(1, GRAD_WGS // (n_pt * n_qt))
    mx = _cdiv(M, 256)
    sp = min(sp_t, mx)
    rows = _cdiv(_cdiv(M, sp), 64) * 64
    splits = _cdiv(M, rows)
    regime = "one" if splits == 1 else ("rows" if mx <= sp_t else "target")
    return dict(n_pt=n_pt, n_qt=n_qt, sp=sp, rows=rows, splits=splits, regime=regime, last=M - (splits - 1) * rows)


def refresh_ref(A, B, s):
    """the statements of ops.LoraExt.refresh -> a = bf16(A) [r, K], sB = bf16(float(bf16(B)) * s) [Dn, r]"""
    return A.to(torch.bfloat16), (B.to(torch.bfloat16).float() * s).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------ float32 restatements; `wrong` names a deliberately wrong variant
def _chain(L, Rt, round_every=0):
    """L [m, n], Rt [p, n] float64 -> fp32 [m, p]: one MFMA issue (16 terms) at a time; round_every: the accumulator is rounded to bf16 after that many terms"""
    m, n, p = L.shape[0], L.shape[1], Rt.shape[0]
    nch = _cdiv(n, MFMA_K)
    Lc, Rc = np.zeros((nch, m, MFMA_K)), np.zeros((nch, MFMA_K, p))                     # the chunks, contiguous; the zero padding adds exact zeros
    Lp, Rp = np.zeros((m, nch * MFMA_K)), np.zeros((p, nch * MFMA_K))
    Lp[:, :n], Rp[:, :n] = L, Rt
    Lc[:] = Lp.reshape(m, nch, MFMA_K).transpose(1, 0, 2)
    Rc[:] = Rp.reshape(p, nch, MFMA_K).transpose(1, 2, 0)
    acc = np.zeros((m, p), np.float32)
    wide = np.zeros((m, p))
    for c in range(nch):
        np.matmul(Lc[c], Rc[c], out=wide)
        wide += acc
        acc = wide.astype(np.float32)
        if round_every and ((c + 1) * MFMA_K % round_every == 0 or c + 1 == nch):
            acc = bf16_round(acc)
    return acc


def _f64(a):
    return f32(a).astype(np.float64)


def _drop_unit_term(x, k):
    """one term of ONE row lost (a lane's fragment element): column k of the row whose value there is nearest to 1 in magnitude, a term of ordinary size"""
    x = x.copy()
    x[np.argmin(np.abs(np.abs(x[:, k]) - 1.0)), k] = 0.0
    return x


def down_f32(x, a, wrong=None):
    """-> [M, R] float32 holding bf16 values; NaN = not written"""
    x, a = _f64(x), _f64(a)
    K, R = x.shape[1], a.shape[0]
    if wrong == "drop_last_chunk":
        x, a = x[:, :K - 64], a[:, :K - 64]
    if wrong == "drop_one_term":
        x = _drop_unit_term(x, K // 2 + 5)
    out = bf16_round(_chain(x, a, 64 if wrong == "acc_bf16" else 0))
    if wrong == "no_tail_cols":
        out[:, R // 4 * 4:] = np.nan
    return out


def up_f32(y, t, b, s, wrong=None):
    """y None = accumulate off"""
    t, b = _f64(t), _f64(b)
    s = np.float32(s)
    if wrong == "drop_one_term":
        t = _drop_unit_term(t, t.shape[1] // 2)
    acc = _chain(t, b, 64 if wrong == "acc_bf16" else 0)
    if y is None or wrong == "no_accumulate":
        return bf16_round(s * acc)
    y = f32(y)
    if wrong == "up_scale_after":
        return bf16_round((acc + y) * s)
    v = s * acc
    if wrong == "up_double_round":
        v = bf16_round(v)
    return bf16_round(v + y)


def grad_f32(u, v, s, wrong=None):
    u, v = _f64(u), _f64(v)
    M = u.shape[0]
    if wrong == "drop_one_term":
        u = u.copy()
        u[M // 2] = 0.0
    p = grad_plan(M, u.shape[1], v.shape[1])
    rows = _cdiv(M, p["sp"]) if wrong == "grad_split_overlap" else p["rows"]       # the unrounded plan: the only one under which the zero-fill bound is live
    parts = []
    for c in range(_cdiv(M, rows)):
        mbeg, mend = c * rows, min((c + 1) * rows, M)
        if wrong in ("grad_split_overlap", "grad_zfill_M"):
            mend = min(mbeg + _cdiv(mend - mbeg, 64) * 64, M)                     # whole 64-row tiles, zero-filled from M on
        parts.append(_chain(u[mbeg:mend].T, v[mbeg:mend].T, 64 if wrong == "acc_bf16" else 0))
    if wrong == "grad_last_split_lost":
        parts = parts[:-1]
    a = np.zeros((u.shape[1], v.shape[1]), np.float32)
    for part in parts:
        a = a + part
    s = np.float32(s)
    return s * (s * a) if wrong == "grad_scale_twice" else s * a


DOWN_WRONG = ["drop_last_chunk", "drop_one_term", "acc_bf16", "no_tail_cols"]
UP_WRONG = ["drop_one_term", "acc_bf16", "up_double_round", "up_scale_after", "no_accumulate"]
GRAD_WRONG = ["drop_one_term", "acc_bf16", "grad_split_overlap", "grad_last_split_lost", "grad_scale_twice"]


# ------------------------------------------------------------------------------------------ inputs (CPU, seeded; the device tests move them)
_KIND = {"exact": 1, "randn": 2, "mean": 3}


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _pm12(shape, g):
    """values in {-2, -1, 1, 2}"""
    return (torch.randint(1, 3, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def _sparse_pm1(rows, n, g):
    """[rows, n] in {-1, 0, 1}: column k has a non-zero in row k % rows, row r one in column r % n -- every column and every row is hit"""
    a = torch.zeros(rows, n)
    sign = lambda k: (2 * torch.randint(0, 2, (k,), generator=g) - 1).float()
    k = torch.arange(n)
    a[k % rows, k] = sign(n)
    r = torch.arange(rows)
    a[r, r % n] = sign(rows)
    return a


def down_inputs(M, K, R, kind):
    """x [M, K], a [R, K] bf16.  kind "exact": integers (module docstring); "randn": N(0, 1) and N(0, 1 / K); "mean": both moved by 0.3 of their deviation"""
    g = _gen(M, K, R, _KIND[kind])
    if kind == "exact":
        x, a = _pm12((M, K), g), _sparse_pm1(R, K, g)
        assert float(2 * a.abs().sum(1).max()) <= 256
    else:
        sh = 0.3 if kind == "mean" else 0.0
        x, a = torch.randn(M, K, generator=g) + sh, (torch.randn(R, K, generator=g) + sh) / K ** 0.5
    return x.to(torch.bfloat16), a.to(torch.bfloat16)


def up_inputs(M, N, rp, kind):
    """t [M, rp], b [N, rp], y [M, N] bf16"""
    g = _gen(M, N, rp, _KIND[kind], 3)
    if kind == "exact":
        t, b = _pm12((M, rp), g), _sparse_pm1(N, rp, g)
        y = _pm12((M, N), g) * torch.randint(1, 5, (M, N), generator=g)
        assert float(2 * 2 * b.abs().sum(1).max()) + 8 <= 128            # |s| <= 2, results on a grid of 1/2: eight bits up to 128
    else:
        sh = 0.3 if kind == "mean" else 0.0
        t, b, y = torch.randn(M, rp, generator=g) + sh, torch.randn(N, rp, generator=g) + sh, torch.randn(M, N, generator=g)
    return t.to(torch.bfloat16), b.to(torch.bfloat16), y.to(torch.bfloat16)


def up_scale(s, kind):
    """the scale of a case: integer data needs a power of two"""
    return s if kind != "exact" else (2.0 if s > 0 else -0.5)


def grad_inputs(M, P, Q, kind):
    """u [M, P], v [M, Q] bf16"""
    g = _gen(M, P, Q, _KIND[kind], 5)
    if kind == "exact":
        u, v = _pm12((M, P), g), _sparse_pm1(Q, M, g).t().contiguous()
    else:
        sh = 0.3 if kind == "mean" else 0.0
        u, v = torch.randn(M, P, generator=g) + sh, torch.randn(M, Q, generator=g) + sh
    return u.to(torch.bfloat16), v.to(torch.bfloat16)


def refresh_inputs(r, K, Dn, s):
    """A [r, K], B [Dn, r] fp32; the first values of B are ones on which rounding B to bf16 before the product with s changes the stored result -> A, B, count"""
    g = _gen(r, K, Dn, 11)
    A, B = torch.randn(r, K, generator=g) / K ** 0.5, 0.3 * torch.randn(Dn, r, generator=g)
    cand = 0.3 * torch.randn(4096, generator=g)
    differ = (cand.to(torch.bfloat16).float() * s).to(torch.bfloat16) != (cand * s).to(torch.bfloat16)
    cand = cand[differ][:min(Dn * r, 64)]
    B.view(-1)[:cand.numel()] = cand
    return A, B, cand.numel()


# ------------------------------------------------------------------------------------------ the cases of both test files
DOWN_R = {"dma": [16, 48, 64], "reg": [96, 128, 160, 192, 224, 256], "tail": [18, 33, 61, 250]}      # NCB 1, 2 | NCB 3..8 | the scalar tail store of both kernels
DOWN_KS = [64, 128, 192, 256, 320]          # nk = 1 (every prologue chunk and the refill past K), 2, 3, 4 = NS, 5 (the ring wraps)
DOWN_MS = [1, 63, 64, 65, 130]              # one partial block; a full one; a second block of one row (the shortest descriptor); of two rows


def down_cases(group):
    """(M, K, R, layout, data kinds).  layout "contig"; "fwd": X the head and T the tail of one [M, K + R + pad] buffer; ("bwd", j): X the middle slice of
    [M, 3 K + 3 R], T the j-th tail slice, A one [R, K] slice of [2, R, K]"""
    kinds = lambda K, R: ("exact", "randn", "mean") if K in (320, 3072) and R in (64, 192, 250) else ("exact", "randn")
    if group in DOWN_R:
        out = [(65, K, R, "contig", kinds(K, R)) for R in DOWN_R[group] for K in DOWN_KS]
        out += [(M, K, R, "contig", kinds(K, R)) for R in (DOWN_R[group] if group == "tail" else DOWN_R[group][::2]) for M, K in ((1, 192), (63, 128), (64, 256), (130, 192), (1, 64), (130, 320))]
        return out
    if group == "layouts":
        out = [(M, K, R, "fwd", ("exact", "randn")) for M, K, R in ((65, 64, 16), (65, 128, 48), (130, 256, 64), (63, 192, 192), (65, 320, 18), (1, 64, 61), (64, 128, 250),
                                                                    (130, 64, 96))]
        return out + [(M, 128, R, ("bwd", j), ("exact", "randn")) for M, R, j in ((65, 16, 0), (130, 64, 1), (63, 48, 2), (1, 64, 2))]
    if group == "k3072":
        return [(200, 3072, 64, "contig", ("exact", "randn", "mean")), (65, 3072, 64, ("bwd", 1), ("exact", "randn"))]
    raise ValueError(group)


DOWN_GROUPS = ["dma", "reg", "tail", "layouts", "k3072"]
UP_NS, UP_MS, UP_SCALES = [8, 96, 128, 136], [1, 64, 65], [2.0, -0.375]


def up_cases():
    """(M, N, rp, s, accumulate): every rank with both accumulate values at two column blocks (N = 136: 128 + 8); every N, M, s, accumulate at rp = 64;
    the widest rank over the narrowest N"""
    out = [(65, 136, rp, UP_SCALES[i % 2], acc) for i, rp in enumerate(UP_RANKS) for acc in (0, 1)]
    out += [(M, N, 64, s, acc) for N in UP_NS for M in UP_MS for s in UP_SCALES for acc in (0, 1)]
    return out + [(1, 8, 192, -0.375, 1), (64, 8, 16, 2.0, 0)]


GRAD_PQ = [(8, 8), (16, 72), (72, 64), (192, 320), (3072, 64), (64, 3072)]
GRAD_MS = [1, 63, 65, 256, 257, 1300]
GRAD_S = 0.5


def grad_cases():
    """(M, P, Q).  (3072, 64) once more at M = 5000 (16 splits: GRAD_WGS / 48 tiles) and at M = 4810 (the same 16 splits of 320 rows, the last of 10)"""
    return [(M, P, Q) for P, Q in GRAD_PQ for M in GRAD_MS] + [(5000, 3072, 64), (4810, 3072, 64)]


REFRESH_CASES = [(r, K, Dn, float(np.float32(s))) for r, K, Dn, s in ((1, 100, 50, 4.0 / 3.0), (12, 200, 72, 2.0 / 3.0), (64, 192, 128, 4.0 / 3.0))]     # r K + Dn r = 150 (under one block), 3264 (12.75 blocks), 20 480 (80 blocks)
