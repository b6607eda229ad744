"""vgpa_lg_gemm (csrc/lightglue.hip): the Linears and sim of LightGlue in exact fp32.  -m gpu only.

Against float64 the bound is 8 x d32, d32 = the distance of torch's own fp32 evaluation on the CPU (the convention of the fp32 row kernels); error =
max-abs difference over max-abs of the float64 answer (lightglue_ref.err).  What the kernel is for is exact: a sample's rows are the same bits whatever
the batch, the padding and the tile row they land in, rows and columns past the counts keep a planted sentinel.  Every check prints `name err d ratio`."""
import math

import pytest
import torch

import lightglue_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = 777.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops
    return ops


def check(name, got, want64, ref):
    err, d = R.err(got.cpu(), want64), R.err(ref, want64)
    print(f"{name}: err {err:.3e} d {d:.3e} ratio {err / d if d > 0 else float('nan'):.2f}")
    assert math.isfinite(err) and err <= 8.0 * d, (name, err, d)


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def valid_rows(S0, R, c0, c1):
    m = torch.zeros(R, dtype=torch.bool)
    m[:c0] = True
    m[S0:S0 + c1] = True
    return m


@pytest.mark.parametrize("K,N", [(512, 256), (256, 768)])
def test_linear_into_a_strided_half_against_f64_and_alone(ops, K, N):
    """three samples whose counts end inside, at and before a 128-row tile, one with an empty image, one whose last tiles hold no valid row;
    a is the [., K] front of a wider buffer, the output the right part of a sentinel buffer (as out_proj writes cat[x, msg]'s right half)"""
    g = torch.Generator().manual_seed(K + N)
    B, S0, R = 4, 130, 130 + 257
    c0, c1 = [1, 65, 130, 128], [257, 17, 0, 129]
    a, w, bias = torch.randn(B, R, K + 64, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    a[0, 1:S0] = float("nan")                                     # padding may hold anything: it reaches no valid row
    buf = torch.full((B, R, N + 32), SENTINEL, device="cuda")
    ad, wd, bd = a.cuda(), w.cuda(), bias.cuda()
    ops.lg_gemm(ad[..., :K], wd, out=buf[..., 32:], bias=bd, seg=(S0, i32(c0), i32(c1)))
    assert bool((buf[..., :32] == SENTINEL).all())
    got = buf[..., 32:].cpu()
    for b in range(B):
        m = valid_rows(S0, R, c0[b], c1[b])
        assert bool((got[b][~m] == SENTINEL).all()), b
        x = a[b, m, :K]
        check(f"linear K {K} N {N} sample {b}", got[b][m], x.double() @ w.double().t() + bias.double(), x @ w.t() + bias)
        # alone, at its own tight sizes: the rows sit in other tile rows and the grid is another one
        s0, r = max(c0[b], 1), max(c0[b], 1) + max(c1[b], 1)
        tight = torch.zeros(1, r, K)
        tight[0, :c0[b]] = a[b, :c0[b], :K]
        tight[0, s0:s0 + c1[b]] = a[b, S0:S0 + c1[b], :K]
        one = ops.lg_gemm(tight.cuda(), wd, bias=bd, seg=(s0, i32([c0[b]]), i32([c1[b]])))[0].cpu()
        assert torch.equal(one[valid_rows(s0, r, c0[b], c1[b])], got[b][m]), b


def test_accumulate_and_the_unsegmented_form(ops):
    g = torch.Generator().manual_seed(3)
    B, Rr, K, N = 2, 300, 512, 256                               # 300 rows: the last tile is partial
    a, w, pre = torch.randn(B, Rr, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(B, Rr, N, generator=g)
    out = pre.cuda()
    ops.lg_gemm(a.cuda(), w.cuda(), out=out, accumulate=True)
    check("accumulate", out, pre.double() + a.double() @ w.double().t(), pre + a @ w.t())
    again = pre.cuda()
    ops.lg_gemm(a.cuda(), w.cuda(), out=again, accumulate=True)
    assert torch.equal(out, again)
    half = pre[:1, :77].cuda()                                   # one sample, fewer rows: the same bits
    ops.lg_gemm(a[:1, :77].cuda(), w.cuda(), out=half, accumulate=True)
    assert torch.equal(half, out[:1, :77])
    with pytest.raises(RuntimeError):
        ops.lg_gemm(a.cuda(), w.cuda(), out=out, bias=torch.zeros(N, device="cuda"), accumulate=True)
    with pytest.raises(RuntimeError):
        ops.lg_gemm(a[..., :500].cuda(), w[:, :500].cuda())      # K is a multiple of 16


def test_sim_form_per_sample_operand_and_column_counts(ops):
    """sim = md0 md1^T / 16 with both operands views of one [B, M + N, 256] activation, N no multiple of 32"""
    g = torch.Generator().manual_seed(5)
    B, M, N = 3, 200, 190
    m, n = [200, 1, 65], [190, 129, 0]
    md = torch.randn(B, M + N, 256, generator=g)
    mdd = md.cuda()
    sim = torch.full((B, M, N), SENTINEL, device="cuda")
    ops.lg_gemm(mdd[:, :M], mdd[:, M:], out=sim, alpha=0.0625, seg=(M, i32(m), None), ncount=i32(n))
    got = sim.cpu()
    for b in range(B):
        keep = torch.zeros(M, N, dtype=torch.bool)
        keep[:m[b], :n[b]] = True
        assert bool((got[b][~keep] == SENTINEL).all()), b
        if n[b] == 0:
            continue
        x, y = md[b, :m[b]], md[b, M:M + n[b]]
        check(f"sim sample {b}", got[b, :m[b], :n[b]], x.double() @ y.double().t() / 16, x @ y.t() / 16)
        tight = torch.cat([x, y])[None].cuda()
        one = ops.lg_gemm(tight[:, :m[b]], tight[:, m[b]:], alpha=0.0625)[0].cpu()
        assert torch.equal(one, got[b, :m[b], :n[b]]), b
