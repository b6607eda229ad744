"""Tolerance of the forward attention's lse2 (log2 of a row's softmax denominator) -- the contract since round 6.

The w1 forward accumulates the row sums on the matrix pipe from the bf16-ROUNDED weights, the same registers the PV product reads (`mfsum`):
    l~ = sum_j bf16(p_j)        p_j = exp2(s_j - M')
so that O = sum_j bf16(p_j) v_j / l~ is an exact convex combination of V rows.  Round-to-nearest-even to 8 significant bits gives bf16(p_j) = p_j (1 + d_j),
|d_j| <= 2^-8 (reached when the mantissa of p_j is just above 1.0), independent across keys, hence
    l~ / l - 1 = sum_j w_j d_j        w_j = p_j / l  (the exact softmax weights)
    worst case  |.| <= 2^-8                     (a one-hot row: 5.6e-3 in log2 units)
    typical     std <= 2^-8 / sqrt(3) * sqrt(sum_j w_j^2)   (a row spread over n keys: ~ 2.3e-3 / sqrt(n))
Rows redone by the online-softmax kernel (flagged strips) sum the unrounded weights in fp32 and sit far inside this.  The tolerance below is the smaller of the
worst case and six standard deviations, plus the fp32 floor the old fp32 row sums were held to."""
import math

import torch

LOG2E = 1.4426950408889634
RND = 2.0 ** -8


def lse2_tol_from_conc(conc, lse_ref, floor=3e-4, rel=2e-5, sigmas=6.0):
    """lse2_tol from conc = sqrt(sum_j w_j^2) per row (what a chunked reference keeps of the weights)"""
    stat = sigmas * RND / math.sqrt(3.0) * conc
    worst = torch.full_like(conc, 1.02 * RND)
    return LOG2E * torch.minimum(stat, worst) + floor + rel * lse_ref.abs()


def lse2_tol(w, lse_ref, floor=3e-4, rel=2e-5, sigmas=6.0):
    """w: exact softmax weights (fp64, [..., Sq, Skv], rows summing to one); lse_ref [..., Sq] in log2 units -> per-row tolerance on |lse2 - lse_ref|"""
    return lse2_tol_from_conc((w * w).sum(-1).sqrt(), lse_ref, floor, rel, sigmas)


# ------------------------------------------------------------------------------------------------ per-element tolerances of O, dV, dK, dQ
PER_ELEMENT = """Every tolerance below is   tol = half_ulp(|ref| + rest) + rest,   rest = 6 sqrt(var) + det + floor,   over the sums tests/attn_ref64.py returns.

half_ulp: the result is stored in bf16 (8 significant bits): its rounding is at most half an ulp = 2^(floor(log2 |x|) - 8), which lies between 2^-9 |x| (mantissa
    just under 2) and 2^-8 |x| (mantissa 1.0).  2^-9 |ref| is therefore the SMALLEST a correct rounding can stay under, not a bound on it (1.00390625 rounds to 1.0 or
    1.0078125: 2^-8 away, exactly rounded); the ulp is taken at |ref| + rest because the unrounded result may lie in the next binade.
var:  independent roundings, each uniform within +-unit: variance unit^2 / 3 (the worst mantissa, 1.0).  Six standard deviations of their sum.
det:  effects that are the same for every term of a row (a coherent factor): bounded by their worst case, summed linearly.
floor: fp32 accumulation, 2^-20 sum |terms|.

Forward  O~_id = sum_j w~_ij v_jd / sum_j w~_ij  with  w~_ij = w_ij + r_ij,  |r_ij| <= e_ij:
    e_ij = 2^-8 w_ij                                        bf16 weights (csrc/attention_w1.hip, attention.hip, the bf16 kernels of attention_hd128.hip)
    e_ij = max(2^-4 w_ij, 2^-18 W_it)                       e4m3 weights (vgpa_attn128_fwd_f8: P8 = e4m3(p / 2^x), x = exponent of the row's sum W over the key's 64-key
                                                            tile minus 8 (tools/gen_w1_asm.py Fwd128F8Loop), so p / 2^x < 2^8; e4m3 keeps 4 significant bits down to
                                                            2^-6 and steps of 2^-9 below: half a step 2^-10 2^x <= 2^-18 W_it)
    normalised by the ROUNDED sum (w1 head_dim 64):   O~ - o = sum_j r_ij (v_jd - o_id)     var_o = 1/3 sum_j e_ij^2 (v_jd - o_id)^2
    normalised by the fp32 sum of the unrounded p:    O~ - o = sum_j r_ij v_jd              var_o = 1/3 sum_j e_ij^2 v_jd^2
    (both expand into e^2 @ v^2, e^2 @ v and sum e^2: three products, the cost of the reference itself)
    det_o  = ln 2 ds_i (sum_j w_ij |v_jd| + |o_id|):  a score accumulated in fp32 is off by |ds_i| <= (D / 16) 2^-24 |qs_i| max_j |k_j| log2 units (score_err below:
             D / 16 accumulator roundings of a dot product bounded by Cauchy-Schwarz), i.e. every weight by a factor ln 2 ds_i; invisible at N(0,1), 1e-4 at scores of +-200
    floor_o = 2^-20 sum_j w_ij |v_jd|

Backward.  The kernels recompute P~_ij = exp2(s2_ij - lse2~_i) from the FORWARD's lse2, which tests/attn_tol.py::lse2_tol bounds: P~ = w (1 + eps'_i) with
    |eps'_i| <= eps_i = exp2(lse2_tol_i + ds_i) - 1  for every key of the row (det), and of standard deviation sig_i = 2^-8 / sqrt(3) sqrt(sum_j w_ij^2) where the forward
    summed rounded weights (0 where it summed in fp32).  delta~_i = dO_i . O~_i is formed from the forward's OUTPUT, completed by the res8 byte (csrc/common.h: steps of
    2^-15 of the binade, half a step <= 2^-16 |O|) or not (2^-8 |O|): it carries
        det:  (delta_unit + 2^-20) sum_d |dO_id o_id|                                              delta_unit = 2^-16 (int8 residual), 2^-8 (textbook delta)
        var:  var_delta_i = 1/3 sum_j e_ij^2 (dP_ij - delta_i)^2   (rounded row sum; dP_ij^2 with an fp32 one): the forward's weight roundings, seen through dO . (O~ - o)
    and moves every dS of the row by -w_ij d(delta_i):  dQ_i by -d(delta_i) dq_mul kbar_i  (kbar = w @ k, the coherent term of DESIGN 5),  dK_j by -dk_mul sum_i d(delta_i) w_ij qs_i.
    Independent roundings (oracle/cogvideox.py::_RoundedSDPA): P~ to bf16 where it multiplies dO, dS = P~ o (dP - delta) to bf16 where it multiplies K and Q.
    dV_jd = sum_i bf16(P~_ij) dO_id
        var = 2^-16 / 3 sum_i w_ij^2 dO_id^2          det = sum_i eps_i w_ij |dO_id|                           floor = 2^-20 sum_i w_ij |dO_id|
    dK_jd = dk_mul sum_i bf16(dS~_ij) qs_id
        var = dk_mul^2 (2^-16 / 3 sum_i dS_ij^2 qs_id^2 + sum_i var_delta_i w_ij^2 qs_id^2)
        det = dk_mul (sum_i eps_i |dS_ij| |qs_id| + sum_i (delta_unit + 2^-20) absdelta_i w_ij |qs_id|)        floor = 2^-20 dk_mul sum_i |dS_ij| |qs_id|
    dQ_id = dq_mul sum_j bf16(dS~_ij) k_jd
        var = dq_mul^2 2^-16 / 3 sum_j dS_ij^2 k_jd^2 + var_delta_i (dq_mul kbar_id)^2
        det = eps_i |dQ_id| + (delta_unit + 2^-20) absdelta_i dq_mul |kbar_id|                                   floor = 2^-20 dq_mul sum_j |dS_ij| |k_jd|

Aggregate: rms(err) / rms(sigma) <= 1.25 over the compared head AND over each block of 256 rows of it (a strip for O / dQ, four key tiles for dK / dV), with
    sigma^2 = var + (variance of the lse2 factor: sig_i^2 times the squared terms of row i) + (the rounding of the O that delta is formed from: delta_unit^2 / 3
    sum_d (dO_id o_id)^2 per row, through the same kbar / w paths as var_delta) + ulp(ref)^2 / 12  (the output rounding).  unit^2 / 3 is the variance at mantissa 1.0;
    over a log-uniform mantissa it is 0.54 of that, so a faithful kernel sits BELOW 1.  What the rounding emulation of tests/test_attn_tol_host.py measures with every term
    included (17 776 keys, N(0,1), 256 query rows; full S = 1000 with mean-carrying k and v for the gradients) is written in that file's docstring; 1.25 is a margin
    over those, not over a kernel."""
SIGMAS = 6.0
FLOOR = 2.0 ** -20
DELTA_UNIT = {"int8": 2.0 ** -16, None: RND}
LN2 = math.log(2.0)


def score_err(snorm, D):
    """fp32 accumulation of one score on the matrix pipe: D / 16 dependent accumulator roundings of a dot product no larger than |qs_i| max_j |k_j| (Cauchy-Schwarz),
    each half an fp32 ulp (2^-24 relative) -> |ds2_ij| <= (D / 16) 2^-24 snorm_i log2 units, for every key of the row"""
    return (D / 16.0) * 2.0 ** -24 * snorm


def half_ulp_bf16(x):
    """half an ulp of the bf16 number format at magnitude |x| (0 at 0)"""
    x = x.abs()
    return torch.where(x > 0, torch.exp2(torch.floor(torch.log2(x.clamp_min(1e-300))) - 8.0), torch.zeros_like(x))


def _finish(ref, var, det, floor, var_extra):
    rest = SIGMAS * var.clamp_min(0).sqrt() + det + floor
    tol = half_ulp_bf16(ref.abs() + rest) + rest
    sigma = (var.clamp_min(0) + var_extra + (2.0 * half_ulp_bf16(ref)) ** 2 / 12.0).sqrt()
    return tol, sigma


def o_tol(R):
    """R: attn_ref64's dict -> (tol, sigma) [rows, D] of the forward output"""
    o = R["o"]
    if R["rounded_rowsum"]:
        var = (R["e2v2"] - 2.0 * o * R["e2v"] + o * o * R["e2"].unsqueeze(-1)) / 3.0
    else:
        var = R["e2v2"] / 3.0
    det = LN2 * score_err(R["snorm"], R["D"]).unsqueeze(-1) * (R["wabsv"] + o.abs())
    return _finish(o, var, det, FLOOR * R["wabsv"], torch.zeros_like(o))


def dv_tol(R):
    return _finish(R["dv"], R["var_dv"], R["lse_dv"], FLOOR * R["abs_dv"], R["varlse_dv"])


def dk_tol(R, delta="int8"):
    du = DELTA_UNIT[delta] + FLOOR
    return _finish(R["dk"], R["var_dk"] + R["vardelta_dk"], R["lse_dk"] + du * R["detdelta_dk"], FLOOR * R["abs_dk"], R["varlse_dk"] + du * du / 3.0 * R["sqdelta_dk"])


def dq_tol(R, delta="int8"):
    du = DELTA_UNIT[delta] + FLOOR
    var = R["var_dq"] + R["var_delta"].unsqueeze(-1) * R["kbar"] ** 2
    det = R["eps"].unsqueeze(-1) * R["dq"].abs() + du * R["absdelta"].unsqueeze(-1) * R["kbar"].abs()
    extra = (R["sig_lse"] ** 2).unsqueeze(-1) * R["dq"] ** 2 + (du * du / 3.0 * R["sqdelta"]).unsqueeze(-1) * R["kbar"] ** 2
    return _finish(R["dq"], var, det, FLOOR * R["abs_dq"], extra)


RMS_MAX = 1.25        # see PER_ELEMENT, "Aggregate"


def compare(name, got, ref, tol, sigma, where="", row_ids=None, keys=False, block=256):
    """-> (problems, figures).  problems: list of messages (empty = inside the per-element bound everywhere and inside the rms ratio over the head and over every
    `block` rows); figures: {"max_err_over_tol", "rms_ratio", "worst_block_rms_ratio"}.  row_ids: the row numbers of dim 0 (default 0..n-1); keys: rows are KEYS
    (dK, dV: the message names the 64-key tile), otherwise query rows (the 256-row strip and the 64-row tile of the strip)."""
    got, ref = got.double(), ref.double()
    n, D = ref.shape
    ids = torch.arange(n, device=ref.device) if row_ids is None else row_ids.to(ref.device)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)          # a result that is exact where the bound is zero (one key: dS = 0) is inside it
    problems = []
    if not bool(torch.isfinite(got).all()):
        problems.append(f"{name} {where}: non-finite values")
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
    worst = int(ratio.argmax())
    r, d = worst // D, worst % D
    row = int(ids[r])
    place = f"key tile {row // 64}" if keys else f"strip {row // 256}, 64-row tile {(row % 256) // 64} of it"
    over = ratio > 1.0
    if bool(over.any()):
        bad_rows = ids[over.any(-1)]
        problems.append(f"{name} {where}: {int(over.sum())} of {over.numel()} elements over the bound; worst row {row} col {d} ({place}): got {float(got[r, d]):.6g} "
                        f"ref {float(ref[r, d]):.6g} err/tol {float(ratio[r, d]):.3f}; rows over it span {int(bad_rows.min())}..{int(bad_rows.max())} "
                        f"({'key tiles' if keys else 'strips'} {sorted(set((bad_rows // (64 if keys else 256)).tolist()))[:12]})")
    e2, s2 = (got - ref) ** 2, sigma ** 2
    rms = float((e2.sum() / s2.sum().clamp_min(1e-300)).sqrt())
    blk = ids // block
    nb = int(blk.max()) + 1
    be = torch.zeros(nb, dtype=torch.float64, device=ref.device).index_add_(0, blk, e2.sum(-1))
    bs = torch.zeros(nb, dtype=torch.float64, device=ref.device).index_add_(0, blk, s2.sum(-1))
    brms = torch.where(bs > 0, (be / bs.clamp_min(1e-300)).sqrt(), torch.zeros_like(be))
    wb = int(brms.argmax())
    if rms > RMS_MAX:
        problems.append(f"{name} {where}: rms(err) / rms(sigma) = {rms:.3f} > {RMS_MAX} over the head")
    if float(brms[wb]) > RMS_MAX:
        problems.append(f"{name} {where}: rms(err) / rms(sigma) = {float(brms[wb]):.3f} > {RMS_MAX} over rows {wb * block}..{wb * block + block - 1} "
                        f"({'key tiles ' + str(wb * block // 64) + '..' + str(wb * block // 64 + block // 64 - 1) if keys else 'strip ' + str(wb * block // 256)})")
    return problems, {"max_err_over_tol": float(ratio.max()), "rms_ratio": rms, "worst_block_rms_ratio": float(brms[wb])}


def compare_lse2(got, R, where=""):
    """the forward's lse2 against lse2_tol, rows of R"""
    tol = lse2_tol_from_conc(R["conc"].sqrt(), R["lse2"])
    ratio = (got.double() - R["lse2"]).abs() / tol
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    w = int(ratio.argmax())
    row = int(R["rows"][w])
    problems = []
    if float(ratio[w]) > 1.0:
        problems.append(f"lse2 {where}: {int((ratio > 1).sum())} rows over lse2_tol; worst row {row} (strip {row // 256}): got {float(got[w]):.6f} ref {float(R['lse2'][w]):.6f} "
                        f"err/tol {float(ratio[w]):.3f}")
    return problems, {"max_err_over_tol": float(ratio.max())}


def judge(got, R, delta="int8", where=""):
    """every tensor of `got` ({"o"[, "lse2"][, "dq", "dk", "dv"]}: one head, the query rows of R) against attn_ref64's R inside its bound -> (problems, figures per tensor);
    delta: what the backward formed delta from ("int8": the output completed by its residual byte, None: the bf16 output alone)"""
    todo = [("o", o_tol(R), False)]
    if "dq" in got:
        todo += [("dq", dq_tol(R, delta), False), ("dk", dk_tol(R, delta), True), ("dv", dv_tol(R), True)]
    problems, figs = [], {}
    for name, (tol, sigma), keys in todo:
        pr, figs[name] = compare(name, got[name], R[name], tol, sigma, where=where, row_ids=None if keys else R["rows"], keys=keys)
        problems += pr
    if "lse2" in got:
        pr, figs["lse2"] = compare_lse2(got["lse2"], R, where=where)
        problems += pr
    return problems, figs
