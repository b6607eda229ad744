"""Chunked fp64 reference of ONE (batch, head) slice of attention, forward and backward, with the sums the per-element tolerances of tests/attn_tol.py are made of.
Plain torch (CPU or device), nothing from the library under test.  The S x S matrix exists 2048 query rows at a time (290 MB in fp64 at 17 776 keys).

Contract of the kernels it restates (csrc/attention_w1.hip, csrc/attention_hd128.hip):
    s2_ij = smul * (qs_i . k_j)            log2 units.  head_dim 64 and the e4m3 straight-through pair: qs = bf16(q * scale * log2 e), smul = 1;
                                           head_dim 128 in bf16: qs = q as it stands, smul = scale * log2 e (folded into the fp32 scores)
    w = softmax2(s2),  o = w v,  lse2 = log2 sum_j exp2(s2_ij)
    dP = dO v^T,  delta = rowsum(dO o o),  dS = w o (dP - delta)
    dV = w^T dO,  dQ = dq_mul dS k  (w.r.t. the UNscaled query: dq_mul = scale),  dK = dk_mul dS^T qs  (ln 2 with a pre-scaled qs, scale otherwise)
`rows` (optional index tensor) restricts the QUERY rows: o / lse2 / dQ and their sums are returned for those rows, dK / dV are the partial sums over them."""
import math

import torch

from attn_tol import RND, lse2_tol_from_conc, score_err

LN2 = math.log(2.0)


def attn_ref64(qs, k, v, do=None, smul=1.0, dq_mul=None, dk_mul=None, rows=None, chunk=2048, p_unit=RND, p_sub=0.0, rounded_rowsum=True, tile=64):
    """qs [Sq, D], k / v [Skv, D], do [Sq, D] or None (forward only) -> dict of fp64 tensors.
    p_unit / p_sub: the forward's rounding of a weight is at most max(p_unit * w_ij, p_sub * (sum of w over the key's `tile`-key tile)) -- bf16: (2^-8, 0); the e4m3
    forward: (2^-4, 2^-18), see attn_tol.  rounded_rowsum: the forward normalises by the sum of the ROUNDED weights (w1 head_dim-64 kernel) or by the fp32 sum of the
    unrounded ones (online-softmax, head_dim-128 and e4m3 kernels).
    Forward sums (per query row i, column d):   conc = sum_j w^2;  e2 = sum_j e^2;  e2v = e^2 @ v;  e2v2 = e^2 @ v^2;  wabsv = w @ |v|;  snorm = |qs_i| max_j |k_j| smul
    Backward sums: see the names below; every one is a product against w, w^2, dS, |dS| or dS^2 of the chunk."""
    dev = qs.device
    qs, k, v = qs.double(), k.double(), v.double()
    Skv, D = k.shape
    idx = torch.arange(qs.shape[0], device=dev) if rows is None else rows.to(dev)
    n = idx.numel()
    bwd = do is not None
    if bwd:
        do = do.double()
    ub2 = RND * RND                       # the backward rounds P and dS to bf16 whatever the forward ran on
    k2, v2, absk, absv = k * k, v * v, k.abs(), v.abs()
    kmax = k.norm(dim=-1).max()
    R = {name: torch.empty(n, D, dtype=torch.float64, device=dev) for name in ("o", "e2v", "e2v2", "wabsv")}
    for name in ("lse2", "conc", "e2", "snorm"):
        R[name] = torch.empty(n, dtype=torch.float64, device=dev)
    if bwd:
        for name in ("dq", "var_dq", "abs_dq", "kbar", "abskbar"):
            R[name] = torch.empty(n, D, dtype=torch.float64, device=dev)
        for name in ("delta", "absdelta", "sqdelta", "var_delta", "eps", "sig_lse"):
            R[name] = torch.empty(n, dtype=torch.float64, device=dev)
        for name in ("dk", "dv", "var_dk", "var_dv", "abs_dk", "abs_dv", "lse_dk", "lse_dv", "varlse_dk", "varlse_dv", "vardelta_dk", "detdelta_dk", "sqdelta_dk"):
            R[name] = torch.zeros(Skv, D, dtype=torch.float64, device=dev)
    pad = (-Skv) % tile
    for c0 in range(0, n, chunk):
        sl = slice(c0, min(n, c0 + chunk))
        qc = qs[idx[sl]]
        s2 = (qc @ k.t()) * smul
        m = s2.max(-1, keepdim=True).values
        p = torch.exp2(s2 - m)
        del s2
        l = p.sum(-1, keepdim=True)
        w = p / l
        del p
        w2 = w * w
        if p_sub > 0.0:
            wt = torch.nn.functional.pad(w, (0, pad)).view(w.shape[0], -1, tile).sum(-1)
            e = torch.maximum(p_unit * w, p_sub * wt.repeat_interleave(tile, dim=1)[:, :Skv])
            e2 = e * e
            del e, wt
        else:
            e2 = (p_unit * p_unit) * w2
        o = w @ v
        R["o"][sl], R["lse2"][sl] = o, (m + torch.log2(l)).squeeze(-1)
        R["conc"][sl], R["e2"][sl] = w2.sum(-1), e2.sum(-1)
        R["e2v"][sl], R["e2v2"][sl], R["wabsv"][sl] = e2 @ v, e2 @ v2, w @ absv
        R["snorm"][sl] = qc.norm(dim=-1) * kmax * abs(smul)
        if not bwd:
            continue
        doc = do[idx[sl]]
        qa, q2, do2, doa = qc.abs(), qc * qc, doc * doc, doc.abs()
        lse_tol = lse2_tol_from_conc(R["conc"][sl].sqrt(), R["lse2"][sl])
        eps = torch.exp2(lse_tol + score_err(R["snorm"][sl], D)) - 1.0          # |P~ / P - 1| of every weight of the row the backward recomputes
        sig = (RND / math.sqrt(3.0)) * R["conc"][sl].sqrt() if rounded_rowsum else torch.zeros_like(eps)
        R["eps"][sl], R["sig_lse"][sl] = eps, sig
        dP = doc @ v.t()
        delta = (doc * o).sum(-1, keepdim=True)
        # what the forward's weight rounding leaves in delta = dO . O~:  sum_j w_ij d_ij (dP_ij - delta_i)  (rounded row sum) or  sum_j w_ij d_ij dP_ij  (fp32 row sum)
        g = dP - delta
        R["var_delta"][sl] = (e2 * (g * g if rounded_rowsum else dP * dP)).sum(-1) / 3.0
        del dP, e2
        dS = w * g
        del g
        R["delta"][sl], R["absdelta"][sl] = delta.squeeze(-1), (doc * o).abs().sum(-1)
        R["sqdelta"][sl] = ((doc * o) ** 2).sum(-1)
        dS2, dSa = dS * dS, dS.abs()
        R["dq"][sl] = dq_mul * (dS @ k)
        R["var_dq"][sl] = (dq_mul * dq_mul * ub2 / 3.0) * (dS2 @ k2)
        R["abs_dq"][sl] = abs(dq_mul) * (dSa @ absk)
        R["kbar"][sl], R["abskbar"][sl] = dq_mul * (w @ k), abs(dq_mul) * (w @ absk)
        R["dv"] += w.t() @ doc
        R["dk"] += dk_mul * (dS.t() @ qc)
        R["var_dv"] += (ub2 / 3.0) * (w2.t() @ do2)
        R["var_dk"] += (dk_mul * dk_mul * ub2 / 3.0) * (dS2.t() @ q2)
        R["abs_dv"] += w.t() @ doa
        R["abs_dk"] += abs(dk_mul) * (dSa.t() @ qa)
        ec, sc2 = eps.unsqueeze(-1), (sig * sig).unsqueeze(-1)
        R["lse_dv"] += w.t() @ (ec * doa)
        R["lse_dk"] += abs(dk_mul) * (dSa.t() @ (ec * qa))
        R["varlse_dv"] += w2.t() @ (sc2 * do2)
        R["varlse_dk"] += (dk_mul * dk_mul) * (dS2.t() @ (sc2 * q2))
        R["vardelta_dk"] += (dk_mul * dk_mul) * (w2.t() @ (R["var_delta"][sl].unsqueeze(-1) * q2))
        R["detdelta_dk"] += abs(dk_mul) * (w.t() @ (R["absdelta"][sl].unsqueeze(-1) * qa))
        R["sqdelta_dk"] += (dk_mul * dk_mul) * (w2.t() @ (R["sqdelta"][sl].unsqueeze(-1) * q2))
        del w, w2, dS, dS2, dSa
    R["rows"], R["bwd"], R["D"], R["rounded_rowsum"], R["Skv"] = idx, bwd, D, rounded_rowsum, Skv
    return R

