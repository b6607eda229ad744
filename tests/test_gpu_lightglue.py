"""LightGlue on the device: the kernels of csrc/lightglue.hip, videogpa_amd.lightglue.LightGlue and the epipolar metric end to end.  -m gpu only.

The oracle is tests/lightglue_ref.py (a torch restatement of upstream on the CPU).  Error = max-abs difference over max-abs of the float64 answer.
The attention and everything behind it is bounded by 2 x d16, d16 = that distance for the oracle's "ref16" mode (the reference's own fp16 arithmetic
around the attention products) on the same inputs; the fp32 row kernels by 8 x d32 (the fp32 evaluation on the CPU).  Decisions are exact: pruning and
the assignment must give what torch gives on the device's own sigmoids and log scores.  Every check prints `name err d ratio` before it asserts."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lightglue_ref as R

pytestmark = pytest.mark.gpu
PRUNE_CONF = {"pruning_threshold": 64}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops
    return ops


def check(name, got, want64, ref, factor):
    err, d = R.err(got.cpu(), want64), R.err(ref, want64)
    print(f"{name}: err {err:.3e} d {d:.3e} ratio {err / d if d > 0 else float('nan'):.2f}")
    assert math.isfinite(err) and err <= factor * d, (name, err, d)


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------- attention
def rope_tables(B, T, g):
    p = 3.0 * torch.randn(B, T, 32, generator=g)
    return p.cos(), p.sin()


def attn_oracle(q, k, v, nq, nk, rq, rk, premul, mode):
    """one sample: q [Tq,4,64], k, v [Tk,4,64] fp32 -> [nq,256] in the oracle's arithmetic"""
    dt = torch.float64 if mode == "f64" else torch.float32
    enc = lambda r, n: None if r is None else torch.stack([r[0][:n], r[1][:n]]).to(dt).repeat_interleave(2, -1)[:, None]
    qh, kh, vh = (t[:n].to(dt).transpose(0, 1) for t, n in ((q, nq), (k, nk), (v, nk)))
    if rq is not None:
        qh = R.rope(enc(rq, nq), qh)
    if rk is not None:
        kh = R.rope(enc(rk, nk), kh)
    return R.attention(qh * premul, kh * premul, vh, mode).transpose(0, 1).flatten(1)


def run_attention(ops, dirs, premul, ds):
    """dirs: [dict(q, k, v [B,T,4,64] CPU fp32, nq, nk lists, rq, rk (cos, sin) | None)] -> per direction the device output [B,Tq,256] (sentinel 777 in
    rows never written)"""
    dev = []
    for d in dirs:
        def put(t):
            if ds == 1:
                return t.cuda()
            big = torch.randn(*t.shape, 3).cuda()
            big[..., 1] = t.cuda()
            return big[..., 1]
        B, Tq = d["q"].shape[:2]
        out = torch.full((B, Tq, 256), 777.0, device="cuda")
        cu = lambda r: None if r is None else (r[0].cuda(), r[1].cuda())
        dev.append({"q": put(d["q"]), "k": put(d["k"]), "v": put(d["v"]), "nq": i32(d["nq"]), "nk": i32(d["nk"]), "rope_q": cu(d["rq"]), "rope_k": cu(d["rk"]),
                    "out": out})
    return ops.lg_attention(dev, q_premul=premul)


def attention_case(ops, name, counts, ds, rope, premul, seed, pad=7):
    """counts: per direction [(nq, nk) per sample].  Checks the bound, the sentinel and the B = 1 calls at another Nmax."""
    g = torch.Generator().manual_seed(seed)
    dirs = []
    for c in counts:
        B, Tq, Tk = len(c), max(a for a, _ in c) + pad, max(max(b for _, b in c), 1) + pad
        dirs.append({"q": torch.randn(B, Tq, 4, 64, generator=g), "k": torch.randn(B, Tk, 4, 64, generator=g), "v": torch.randn(B, Tk, 4, 64, generator=g),
                     "nq": [a for a, _ in c], "nk": [b for _, b in c], "rq": rope_tables(B, Tq, g) if rope else None,
                     "rk": rope_tables(B, Tk, g) if rope else None})
    outs = run_attention(ops, dirs, premul, ds)
    got, want, ref = [], [], []
    for d, o in zip(dirs, outs):
        for b, (nq, nk) in enumerate(zip(d["nq"], d["nk"])):
            assert bool((o[b, nq:] == 777.0).all()), (name, "a padded row was written")
            if nk == 0:
                assert bool((o[b, :nq] == 0).all())                   # no key: defined as 0
                continue
            sl = lambda r: None if r is None else (r[0][b], r[1][b])
            args = (d["q"][b], d["k"][b], d["v"][b], nq, nk, sl(d["rq"]), sl(d["rk"]), premul)
            got.append(o[b, :nq].cpu())
            want.append(attn_oracle(*args, "f64"))
            ref.append(attn_oracle(*args, "ref16"))
            # the sample alone, at its own Nmax: bit-equal
            one = {"q": d["q"][b:b + 1, :nq], "k": d["k"][b:b + 1, :nk], "v": d["v"][b:b + 1, :nk], "nq": [nq], "nk": [nk],
                   "rq": None if d["rq"] is None else (d["rq"][0][b:b + 1, :nq], d["rq"][1][b:b + 1, :nq]),
                   "rk": None if d["rk"] is None else (d["rk"][0][b:b + 1, :nk], d["rk"][1][b:b + 1, :nk])}
            alone = run_attention(ops, [{k: (v.contiguous() if isinstance(v, torch.Tensor) else v) for k, v in one.items()}], premul, ds)[0]
            assert torch.equal(alone[0], o[b, :nq]), (name, b, "differs from its own B = 1 call")
    check(name, torch.cat(got), torch.cat(want), torch.cat(ref), 2.0)


def test_attention_interleaved_rotary_two_directions(ops):
    attention_case(ops, "attn ds3 rope", [[(1, 1), (65, 65), (257, 257)], [(130, 130), (17, 17), (64, 64)]], 3, True, 1.0, 1)


def test_attention_contiguous_premul_cross_with_an_empty_key_side(ops):
    s = 64 ** -0.25
    attention_case(ops, "attn ds1 cross", [[(257, 64), (17, 0), (65, 130)], [(64, 257), (1, 17), (130, 65)]], 1, False, s, 2)


def test_attention_other_stride_and_rotary_combinations(ops):
    attention_case(ops, "attn ds1 rope", [[(64, 130), (1, 257), (130, 1)]], 1, True, 1.0, 3)
    attention_case(ops, "attn ds3 plain", [[(17, 65), (257, 17), (65, 64)]], 3, False, 64 ** -0.25, 4)


def test_attention_2048(ops):
    attention_case(ops, "attn 2048", [[(2048, 2048)]], 3, True, 1.0, 5, pad=0)


# ---------------------------------------------------------------------------------------------------------------- row kernels
def test_posenc(ops):
    g = torch.Generator().manual_seed(6)
    B, N = 3, 200
    kp = torch.rand(B, N, 2, generator=g) * torch.tensor([160.0, 120.0])
    Wr = torch.randn(32, 2, generator=g)
    counts = [200, 1, 130]
    size = torch.tensor([[160.0, 120.0], [100.0, 300.0], [64.0, 64.0]])
    for name, sz in (("posenc size", size), ("posenc minmax", None)):
        c = torch.full((B, N, 32), 777.0, device="cuda")
        s = torch.full((B, N, 32), 777.0, device="cuda")
        ops.lg_posenc(kp.cuda(), i32(counts), Wr.cuda(), None if sz is None else sz.cuda(), out=(c, s))
        for b, n in enumerate(counts):
            assert bool((c[b, n:] == 777.0).all()) and bool((s[b, n:] == 777.0).all())
            p64 = R.normalize_keypoints(kp[b, :n].double(), None if sz is None else sz[b]) @ Wr.double().t()
            p32 = R.normalize_keypoints(kp[b, :n], None if sz is None else sz[b]) @ Wr.t()
            check(f"{name} cos b{b}", c[b, :n], p64.cos(), p32.cos(), 8.0)
            check(f"{name} sin b{b}", s[b, :n], p64.sin(), p32.sin(), 8.0)


def test_ln_gelu_and_confidence_grid_stride(ops):
    """3 x 3000 rows: more than the 8192 rows one sweep of the grid covers, two segments with ragged counts"""
    g = torch.Generator().manual_seed(7)
    B, R_, S0 = 3, 3000, 1700
    c0, c1 = [1700, 1, 65], [1300, 257, 0]
    valid = torch.zeros(B, R_, dtype=torch.bool)
    for b in range(B):
        valid[b, :c0[b]] = True
        valid[b, S0:S0 + c1[b]] = True
    u = torch.randn(B, R_, 512, generator=g) * 2 + 0.3
    gamma, beta, rb = 1 + 0.1 * torch.randn(512, generator=g), 0.1 * torch.randn(512, generator=g), torch.randn(256, generator=g)
    buf = torch.randn(B, R_, 512, generator=g)
    dbuf = buf.cuda()
    h = ops.lg_ln_gelu(u.cuda(), gamma.cuda(), beta.cuda(), (S0, i32(c0), i32(c1)), resid=dbuf[..., :256], resid_bias=rb.cuda())
    ln = lambda dt: F.gelu(F.layer_norm(u[valid].to(dt), (512,), gamma.to(dt), beta.to(dt), 1e-5))
    check("ln_gelu", h[valid.cuda()], ln(torch.float64), ln(torch.float32), 8.0)
    assert torch.equal(dbuf[..., :256].cpu()[valid], buf[..., :256][valid] + rb) and torch.equal(dbuf.cpu()[~valid], buf[~valid])
    assert torch.equal(dbuf[..., 256:].cpu(), buf[..., 256:])
    # confidence on the left half of the same buffer (row stride 512)
    w, bias, thr = torch.randn(256, generator=g) / 16, 0.3, 0.62
    x = dbuf[..., :256]
    below = torch.zeros(B, dtype=torch.int32, device="cuda")
    conf, z = ops.lg_confidence(x, w.cuda(), bias, (S0, i32(c0), i32(c1)), thr=f32(thr), below=below, want_z=True)
    xv = x.cpu()[valid]
    z64, z32 = xv.double() @ w.double() + bias, xv @ w + bias
    check("confidence z", z[valid.cuda()], z64, z32, 8.0)
    check("confidence sigmoid", conf[valid.cuda()], torch.sigmoid(z64), torch.sigmoid(z32), 8.0)
    assert bool((conf[~valid.cuda()] == 0).all())
    want = [int(((conf[b] < thr) & valid[b].cuda()).sum()) for b in range(B)]           # torch's own comparison on the device's sigmoids
    assert below.tolist() == want and sum(want) > 0


# ---------------------------------------------------------------------------------------------------------------- decisions, exact
def test_prune_is_exact(ops):
    g = torch.Generator().manual_seed(8)
    B, R_, S0 = 3, 400, 270
    c0, c1 = [257, 1, 65], [65, 130, 64]                              # prune_min 64: 64 and 1 keep everything
    x = torch.randn(B, R_, 512, generator=g).cuda()
    seg = (S0, i32(c0), i32(c1))
    conf, _ = ops.lg_confidence(x[..., :256], (torch.randn(256, generator=g) / 8).cuda(), 0.5, seg)
    match, _ = ops.lg_confidence(x[..., :256], (torch.randn(256, generator=g) / 2).cuda(), -3.0, seg)
    conf[0, 3], match[0, 3] = 0.75, 0.0                               # exactly at the confidence threshold: kept (<=)
    conf[0, 4], match[0, 4] = 0.9, f32(0.01)                          # exactly at the matchability threshold: not kept (>)
    cs, sn = torch.randn(B, R_, 32, generator=g).cuda(), torch.randn(B, R_, 32, generator=g).cuda()
    ind = torch.stack([torch.cat([torch.randperm(300, generator=g)[:S0], torch.randperm(200, generator=g)[:R_ - S0]]) for _ in range(B)]).int().cuda()
    xo, co, so, io = torch.full_like(x, 777.0), torch.full_like(cs, 777.0), torch.full_like(sn, 777.0), torch.full_like(ind, -7)
    p0, p1 = torch.ones(B, 300, dtype=torch.int32, device="cuda"), torch.ones(B, 200, dtype=torch.int32, device="cuda")
    n0, n1 = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    keep = ops.lg_prune(conf, match, 0.75, f32(0.01), 64, x[..., :256], xo[..., :256], (cs, sn), (co, so), ind, io, (p0, p1), seg, (n0, n1), want_keep=True)
    removed = 0
    for b in range(B):
        for lo, n, prune, cnt in ((0, c0[b], p0, n0), (S0, c1[b], p1, n1)):
            sl = slice(lo, lo + n)
            k = ((match[b, sl] > 0.01) | (conf[b, sl] <= 0.75)) if n > 64 else torch.ones(n, dtype=torch.bool, device="cuda")      # torch, fp32 vs scalar
            kn = int(k.sum())
            removed += n - kn
            assert torch.equal(keep[b, sl].bool(), k) and int(cnt[b]) == kn
            assert torch.equal(xo[b, lo:lo + kn, :256], x[b, sl, :256][k]) and torch.equal(co[b, lo:lo + kn], cs[b, sl][k]) and torch.equal(so[b, lo:lo + kn], sn[b, sl][k])
            assert torch.equal(io[b, lo:lo + kn], ind[b, sl][k])
            want = torch.ones(prune.shape[1], dtype=torch.int32, device="cuda")
            if n > 64:
                want[ind[b, sl][k].long()] += 1
            assert torch.equal(prune[b], want)
            assert bool((xo[b, lo + kn:(S0 if lo == 0 else R_)] == 777.0).all()) and bool((io[b, lo + kn:(S0 if lo == 0 else R_)] == -7).all())
    assert bool(keep[0, 3]) and not bool(keep[0, 4]) and removed > 50
    assert bool((xo[..., 256:] == 777.0).all())


def lowest_argmax(s, dim):
    mx = s.max(dim, keepdim=True).values
    ar = torch.arange(s.shape[dim]).view(-1, 1) if dim == 0 else torch.arange(s.shape[dim]).view(1, -1)
    idx = torch.where(s == mx, ar.expand_as(s), s.shape[dim]).min(dim).values
    assert torch.equal(idx, s.max(dim).indices)                       # torch.max on the CPU takes the lowest index too
    return mx.squeeze(dim), idx


def assign_checks(ops, sim, z0, z1, m, n):
    """lg_assign on CPU inputs: the log scores (and with them the log-sum-exps) against fp64, every decision against torch on the device's own log
    scores -> (the device outputs, the number of valid matches per sample)"""
    B = sim.shape[0]
    out = ops.lg_assign(sim.cuda(), z0.cuda(), z1.cuda(), i32(m), i32(n), f32(0.1), want_scores=True)
    la = out["log_assignment"].cpu()
    nvalid = []
    for b in range(B):
        S = la[b, :m[b], :n[b]]
        # the log-sum-exps, through the scores they produce
        s64 = sim[b, :m[b], :n[b]].double()
        w64 = F.log_softmax(s64, 1) + F.log_softmax(s64, 0) + F.logsigmoid(z0[b, :m[b]].double())[:, None] + F.logsigmoid(z1[b, :n[b]].double())[None]
        s32 = sim[b, :m[b], :n[b]]
        w32 = F.log_softmax(s32, 1) + F.log_softmax(s32, 0) + (F.logsigmoid(z0[b, :m[b]])[:, None] + F.logsigmoid(z1[b, :n[b]])[None])
        check(f"assign log score b{b}", S, w64, w32, 8.0)
        check(f"assign dustbin b{b}", la[b, :m[b], n[b]], F.logsigmoid(-z0[b, :m[b]].double()), F.logsigmoid(-z0[b, :m[b]]), 8.0)
        assert float(la[b, m[b], n[b]]) == 0.0
        # decisions: torch on the device's own log scores
        max0, a0 = lowest_argmax(S, 1)
        _, a1 = lowest_argmax(S, 0)
        mutual0, mutual1 = torch.arange(m[b]) == a1[a0], torch.arange(n[b]) == a0[a1]
        ms0 = torch.where(mutual0, torch.exp(max0.cuda()).cpu(), torch.zeros(()))
        valid0 = mutual0 & (ms0 > 0.1)
        ms1 = torch.where(mutual1, ms0[a1], torch.zeros(()))
        valid1 = mutual1 & valid0[a1]
        assert torch.equal(out["matches0"][b, :m[b]].cpu().long(), torch.where(valid0, a0, -1)), b
        assert torch.equal(out["matches1"][b, :n[b]].cpu().long(), torch.where(valid1, a1, -1)), b
        assert torch.equal(out["matching_scores0"][b, :m[b]].cpu(), ms0) and torch.equal(out["matching_scores1"][b, :n[b]].cpu(), ms1)
        k = int(valid0.sum())
        nvalid.append(k)
        assert int(out["count"][b]) == k
        assert torch.equal(out["matches"][b, :k].cpu().long(), torch.stack([torch.arange(m[b])[valid0], a0[valid0]], -1))
        assert torch.equal(out["scores"][b, :k].cpu(), ms0[valid0])
        assert bool((out["matches0"][b, m[b]:] == -1).all()) and bool((out["matches1"][b, n[b]:] == -1).all())
    return out, nvalid


def test_assign_is_exact_with_ties_and_gives_the_log_sum_exps(ops):
    g = torch.Generator().manual_seed(9)
    B, M, N = 4, 260, 270
    m, n = [257, 65, 65, 1], [65, 130, 257, 65]
    sim = torch.randint(-8, 9, (B, M, N), generator=g).float() / 4
    z0, z1 = 2 * torch.randn(B, M, generator=g), 2 * torch.randn(B, N, generator=g)
    sim, z0, z1 = (t[[0, 3, 1, 2]].clone() for t in (sim, z0, z1))
    sim[0] += 6 * torch.eye(M, N)                                      # mutual matches on the diagonal
    sim[2] += 6 * torch.eye(M, N)
    z0[0, 2] = z1[0, 2] = z0[2, 4] = z1[2, 4] = 5.0
    sim[0, 2, 2] = sim[2, 4, 4] = 9.0                                  # strong enough to stay valid with the tie halving its row / column weight
    sim[0, :, 7], z1[0, 7] = sim[0, :, 2].clone(), z1[0, 2]           # a duplicated column: every row ties between 2 and 7
    sim[2, 9, :], z0[2, 9] = sim[2, 4, :].clone(), z0[2, 4]           # a duplicated row: every column ties between 4 and 9
    z0[1], z1[1] = -9.0, -9.0                                          # sample 1, between two full ones: no score reaches 0.1
    out, nvalid = assign_checks(ops, sim, z0, z1, m, n)
    assert nvalid[0] >= 10 and nvalid[2] >= 10 and nvalid[1] == 0, nvalid
    assert int(out["matches0"][0, 2]) == 2 and int(out["matches1"][2, 4]) == 4 and int(out["matches0"][2, 9]) == -1      # ties went to the lowest index


def test_assign_grid_stride(ops):
    """3 x 3000 rows against the 8192 one sweep of the row kernels covers, and 3001 x 101 log scores of a sample against the 262144 one sweep of the
    scores kernel covers: both loops go round twice, over rows that hold matches"""
    g = torch.Generator().manual_seed(10)
    B, M, N = 3, 3000, 100
    m, n = [3000, 65, 2900], [100, 100, 90]
    sim = torch.randint(-8, 9, (B, M, N), generator=g).float() / 4
    z0, z1 = 2 * torch.randn(B, M, generator=g), 2 * torch.randn(B, N, generator=g)
    for b, rows in ((0, range(2900, 2990)), (2, range(2800, 2890))):   # rows only the second sweep of either loop reaches
        for j, i in enumerate(rows):
            sim[b, i, j], z0[b, i], z1[b, j] = 12.0, 5.0, 5.0
    out, nvalid = assign_checks(ops, sim, z0, z1, m, n)
    assert nvalid[0] >= 80 and nvalid[2] >= 80, nvalid
    assert int(out["matches0"][0, 2950]) == 50 and int(out["matches0"][2, 2850]) == 50


def test_assign_threshold_is_strict_and_compared_in_double(ops):
    """The last stage alone on planted maxima.  exp's image need not hold fp32(0.1), so: the floats around log(0.1) whose exp straddles 0.1 against
    thr = 0.1, and a score exactly AT a threshold (thr = that score as a double) and one fp32 ulp either side of it."""
    x = torch.tensor(math.log(0.1), dtype=torch.float32)
    xs = [x]
    for _ in range(8):
        xs = [torch.nextafter(xs[0], torch.tensor(-9.0))] + xs + [torch.nextafter(xs[-1], torch.tensor(0.0))]
    xs = torch.stack(xs).cuda()
    K = xs.numel()
    e = torch.exp(xs)
    assert bool((e > 0.1).any()) and bool((e <= 0.1).any())
    e0 = e[K // 2].cpu()
    up, down = torch.nextafter(e0, torch.tensor(1.0)), torch.nextafter(e0, torch.tensor(0.0))
    for thr, want in ((f32(0.1), e > 0.1), (float(e0), e > e0.cuda()), (float(up), e > up.cuda()), (float(down), e > down.cuda())):
        ws, v = ops.lg_assign_workspace(1, K, K, "cuda")
        v["rbest"][0] = xs
        v["rarg"][0] = torch.arange(K, dtype=torch.int32)
        v["carg"][0] = torch.arange(K, dtype=torch.int32)
        dummy = torch.zeros(1, K, K, device="cuda")
        out = ops.lg_assign(dummy, dummy[:, 0].contiguous(), dummy[:, 0].contiguous(), i32([K]), i32([K]), thr, stages=4, workspace=ws)
        assert torch.equal(out["matches0"][0] >= 0, want), thr
        assert torch.equal(out["matching_scores0"][0], e) and int(out["count"][0]) == int(want.sum())
    assert not bool((e > e0.cuda())[K // 2]) and bool((e > down.cuda())[K // 2])


# ---------------------------------------------------------------------------------------------------------------- the whole module
_NETS = {}


def make_net(key, sd, pth=None, **conf):
    from videogpa_amd.lightglue import LightGlue
    if key not in _NETS:
        net = LightGlue(**conf)
        net.load_state_dict(sd)
        if pth is not None:
            net.pruning_keypoint_thresholds = {**LightGlue.pruning_keypoint_thresholds, "flash": pth}
        _NETS[key] = net.cuda()
    return _NETS[key]


def feats(d, side):
    return {"keypoints": d[f"keypoints{side}"][None].cuda(), "descriptors": d[f"descriptors{side}"][None].cuda(), "image_size": d[f"image_size{side}"][None].cuda()}


def run(net, d, **kw):
    return net({"image0": feats(d, 0), "image1": feats(d, 1)}, **kw)


@functools.lru_cache(maxsize=None)
def margin():
    sd, d = R.matching_state(0), R.pair(330, 300, 1)
    return 16.0 * float((R.forward(sd, d, "ref16")["scores"] - R.forward(sd, d, "f64")["scores"]).abs().max())


@pytest.mark.parametrize("shape", [(130, 257), (330, 300)])
def test_per_layer_descriptors(ops, shape):
    sd, free = R.state(0), {"depth_confidence": -1, "width_confidence": -1}
    d = R.pair(130, 130, 3, extra=127) if shape == (130, 257) else R.pair(330, 300, 1)
    assert (d["keypoints0"].shape[0], d["keypoints1"].shape[0]) == shape
    ref, r16 = R.forward(sd, d, "f64", free), R.forward(sd, d, "ref16", free)
    taps = {}
    out = run(make_net("plain", sd, **free), d, taps=taps)
    assert out["stop"] == 9 and len(taps["desc"]) == 9
    m, n = shape
    for layer, (_, x) in enumerate(taps["desc"]):
        for side, got in ((0, x[0, :m]), (1, x[0, m:m + n])):
            check(f"desc {shape} layer {layer} side {side}", got, ref["desc"][layer][side], r16["desc"][layer][side], 2.0)


def compare_matches(name, out, ref, mg):
    """the match set on every row whose fp64 top-two gap exceeds the margin, the scores within it"""
    gap = torch.full((ref["matches0"].shape[0],), float("inf"), dtype=torch.float64)
    gap[ref["ind0"]] = R.top2_gap(ref["scores"]).double()
    clear = gap > mg
    got0 = out["matches0"][0].cpu()
    print(f"{name}: {int((got0 > -1).sum())} matches, oracle {int((ref['matches0'] > -1).sum())}, rows excluded {int((~clear).sum())}")
    assert float((~clear).float().mean()) <= 0.05
    assert torch.equal(got0[clear], ref["matches0"][clear])
    ds = float((out["matching_scores0"][0].cpu().double() - ref["matching_scores0"].double())[clear].abs().max())
    print(f"{name}: matching_scores err {ds:.3e} margin {mg:.3e} ratio {ds / mg:.2f}")
    assert ds <= mg
    pairs = {tuple(p) for p in out["matches"][0].cpu().tolist()}
    assert pairs == {(i, int(j)) for i, j in enumerate(got0.tolist()) if j > -1}


def test_matching_state_returns_the_oracle_matches(ops):
    sd, d = R.matching_state(0), R.pair(330, 300, 1)
    ref = R.forward(sd, d, "f64")
    out = run(make_net("matching", sd), d, want_scores=True)
    assert out["stop"] == ref["stop"] == 9
    compare_matches("matching", out, ref, margin())
    assert int((out["matches0"][0] > -1).sum()) >= 290
    ls = float((out["log_assignment"][0].cpu().double() - ref["scores"]).abs().max())
    print(f"matching: log score err {ls:.3e} margin {margin():.3e} ratio {ls / margin():.2f}")
    assert ls <= margin()
    assert torch.equal(out["prune0"][0].cpu(), ref["prune0"]) and out["prune0"].dtype == torch.int64


@pytest.mark.parametrize("layer", [1, 4])
def test_forced_stop(ops, layer):
    sd, d = R.stop_state(0, layer), R.pair(130, 130, 3, extra=127)
    ref = R.forward(sd, d, "f64")
    out = run(make_net(f"stop{layer}", sd), d, want_scores=True)
    assert out["stop"] == ref["stop"] == layer + 1
    ls = float((out["log_assignment"][0].cpu().double() - ref["scores"]).abs().max())        # that layer's log_assignment, not the last one's
    print(f"stop {layer}: log score err {ls:.3e} margin {margin():.3e} ratio {ls / margin():.2f}")
    assert ls <= margin()
    compare_matches(f"stop {layer}", out, ref, margin())


def test_pruning_follows_the_oracle(ops):
    sd, d = R.prune_state(1), R.pair(200, 150, 11, extra=40)
    ref = R.forward(sd, d, "f64", PRUNE_CONF)
    taps = {}
    out = run(make_net("prune", sd, pth=64), d, taps=taps)
    assert out["stop"] == ref["stop"]
    launched = [k for k in ref["keep"] if k[0] is not None or k[1] is not None]
    assert len(taps["keep"]) == len(launched) >= 2
    counts = [200, 190]
    for (_, keep), want in zip(taps["keep"], launched):
        for side, lo in ((0, 0), (1, 200)):
            got = keep[0, lo:lo + counts[side]].bool().cpu()
            if want[side] is None:
                assert bool(got.all())                                # a side at or below the threshold keeps everything
            else:
                assert torch.equal(got, want[side])
                counts[side] = int(want[side].sum())
    assert torch.equal(out["prune0"][0].cpu(), ref["prune0"]) and torch.equal(out["prune1"][0].cpu(), ref["prune1"])
    compare_matches("prune", out, ref, margin())
    assert int((out["matches0"][0] > -1).sum()) >= 8


def chain():
    sd = R.prune_state(1)
    return sd, [R.pair(200, 150, 11, extra=40), R.steer(R.pair(150, 150, 8), sd, 2), R.steer(R.pair(90, 70, 5, extra=10), sd, 5)]


def test_batch_equals_the_single_calls_bit_for_bit(ops):
    sd, data = chain()
    net = make_net("prune", sd, pth=64)
    want = [R.forward(sd, d, "f64", PRUNE_CONF)["stop"] for d in data]
    assert len(set(want)) == 3
    with torch.no_grad():
        batch = net._pairs([(feats(d, 0), feats(d, 1)) for d in data])
    assert [b["stop"] for b in batch] == want
    assert len({tuple(b["prune0"].unique().tolist()) for b in batch}) >= 2               # they prune differently
    for d, b in zip(data, batch):
        one = run(net, d)
        for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "prune0", "prune1"):
            assert torch.equal(one[k][0], b[k]), k
        assert torch.equal(one["matches"][0], b["matches"]) and torch.equal(one["scores"][0], b["scores"]) and one["stop"] == b["stop"]
    again = net._pairs([(feats(d, 0), feats(d, 1)) for d in data])                        # run to run
    for a, b in zip(again, batch):
        assert all(torch.equal(a[k], b[k]) for k in ("matches0", "matching_scores0", "matching_scores1", "matches", "scores", "prune1"))


def test_match_batch_and_an_empty_side(ops):
    sd = R.matching_state(0)
    net = make_net("matching", sd)
    d = R.pair(130, 100, 4)
    f0, f1 = feats(d, 0), feats(d, 1)
    empty = {"keypoints": torch.zeros(1, 0, 2, device="cuda"), "descriptors": torch.zeros(1, 0, 256, device="cuda"), "image_size": f0["image_size"]}
    outs = net.match_batch([f0, f1, empty, f0])
    assert len(outs) == 3
    one = net({"image0": f0, "image1": f1})
    assert torch.equal(outs[0]["matches"][0], one["matches"][0]) and torch.equal(outs[0]["matching_scores0"], one["matching_scores0"])
    assert len(one["matches"][0]) == 100
    for o, (a, b) in zip(outs[1:], ((100, 0), (0, 130))):
        assert o["matches"][0].shape == (0, 2) and o["matches0"].shape == (1, a) and o["matches1"].shape == (1, b)
        assert bool((o["matches0"] == -1).all()) and bool((o["matches1"] == -1).all())
    two = net({"image0": {k: torch.cat([v, v]) for k, v in f0.items()}, "image1": {k: torch.cat([v, v]) for k, v in f1.items()}})
    assert two["matches0"].shape == (2, 130) and torch.equal(two["matches0"][1], one["matches0"][0]) and two["stop"] == [9, 9]


# ---------------------------------------------------------------------------------------------------------------- the metric end to end
def test_epipolar_metric_end_to_end(ops):
    """SuperPoint (seeded) in front of LightGlue (matching_state) on three crops of one smooth frame, two and four pixels apart.  min_matches is lowered
    to 8 as in tests/test_gpu_superpoint.py: seeded SuperPoint descriptors are not trained to match.  Observed on an MI355X: they are all alike (mean
    cosine between different keypoints of one frame 0.93), so under the default filter_threshold 0.1 no pair has a match at all (largest matching score
    8e-4; 1e-3 even between two copies of one frame) and every pair is "Too few matches".  The same comparisons therefore run a second time with
    filter_threshold = 0, where every mutual match counts, so that keypoints really travel through match_clip and the Sampson error."""
    import superpoint_ref as SR
    from videogpa_amd import scorer as S
    from videogpa_amd.superpoint import SuperPoint
    big = SR.smooth_frames(1, 128, 168, seed=31)[0]
    frames = torch.stack([big[dy:dy + 120, dx:dx + 160] for dy, dx in ((0, 0), (2, 3), (4, 6))]).contiguous()
    sp = SuperPoint(pretrained=False, max_num_keypoints=512, preprocess_conf={"resize": None}).cuda()
    for key, conf in (("matching", {}), ("matching_all_mutual", {"filter_threshold": 0.0})):
        lg = make_net(key, R.matching_state(0), **conf)
        m = S.LightGlueMatcher(min_matches=8, extractor=sp, matcher=lg)
        pairs = m.match_clip(frames.numpy())
        assert len(pairs) == 2
        for i, (p1, p2) in enumerate(pairs):
            q1, q2, k, meta = m.get_matched_points(frames[i].numpy(), frames[i + 1].numpy())
            print(f"{key} pair {i}: {k} matches")
            if p1 is None:
                assert q1 is None and k < 8 and "Too few matches" in meta["error"]
            else:
                assert np.array_equal(q1, p1) and np.array_equal(q2, p2) and k == len(p1) >= 8 and p1.dtype == np.float32
        em = S.EpipolarMetric(descriptor_type="lightglue", min_matches=8, matcher=m)
        val = em.compute(gt=frames.numpy())
        print(f"{key}: metric {val}")
        assert val == em.compute_from_matches([a for a, _ in pairs], [b for _, b in pairs])
        if conf:
            assert any(p1 is not None for p1, _ in pairs) and val >= 0
        else:
            assert val == -1.0 or val >= 0
