"""The LoRA kernels of csrc/lora.hip, each C entry called on raw buffers at every dispatch arm and judged twice: on integer data the result must EQUAL the int64
one (a dropped, doubled or misplaced term changes it), on random data every element is held to the bound counted in tests/lora_tol.py against fp64 computed on the
device (tests/test_lora_tol_host.py shows on the CPU that those bounds reject wrong kernels).

Every operand and every result is a view into a NaN-filled parent: the columns right behind K / R / rp / P / Q, the rows behind M and the rows of A behind R are NaN, so
whatever the DMA ring requests past K or a tile load past a bound must not reach a result, and everything outside the result's view must keep its bits.

    down    lora_down_dma_kernel<1 | 2, 4> (R <= 64), lora_down_kernel<3..8> (R 96..256), the scalar tail store of both (R 18, 33, 61, 250); K / 64 = 1 (the whole
            prologue and the refill past K), 2, 3, 4 (= ring stages), 5, 48; M 1, 63, 64, 65, 130; contiguous, the forward layout (X head, T tail of one buffer) and the
            backward layout (X a middle slice, T a tail slice, A a slice of [2, rp, Dn]).  Not reached: lora_down_kernel<1 | 2> (needs 64 ldx or R K past the 32-bit
            descriptor range, more than 4 GB of X) and the variant builds (LORA_DOWN_DMA=0, LORA_DOWN_NS=3)
    up_add  all seven ranks, accumulate on / off (off over a NaN-filled Y), s 2 / -0.375, N 8 / 96 / 128 / 136, M 1 / 64 / 65, Y always a column slice
    grad    six (P, Q) x six M, split counts asserted against the Python copy of lora_grad_plan (one; ceil(M / 256) with a last split of 20 rows; 768 / tiles with a
            last split of 10), NaN-filled workspace and G, ldg = Q and Q + 8, U and V slices of one parent, two launches bit-identical.  Not reached: the atomicAdd
            branch (the entry refuses a NULL workspace)
    refresh r 1 / 12 / 64 at 150, 3264 and 20 480 elements, padded ld_wt / ld_w, values of B on which rounding before the product with s matters; bit for bit
`-s` prints the largest device error over its bound per family.  -m gpu only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import lora_tol as L

NAN = float("nan")
GUARD = 4              # rows behind the last one
BF = torch.bfloat16


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


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(rows, cols, dtype=BF):
    return torch.full((rows, cols), NAN, dtype=dtype, device="cuda")


def _up8(n):
    return (n + 7) // 8 * 8


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


class Kept:
    """snapshots of parents; after the launch every bit outside the result views must be what it was"""

    def __init__(self, *parents):
        self.parents = [(p, _bits(p).clone()) for p in parents]

    def ok(self, *results):
        """results: views (of the parents) that the launch may write"""
        torch.cuda.synchronize()
        for p, before in self.parents:
            now = _bits(p).clone()
            for r in results:
                if r.untyped_storage().data_ptr() == p.untyped_storage().data_ptr():
                    off = r.storage_offset() - p.storage_offset()
                    r0, c0 = off // p.stride(0), off % p.stride(0)
                    now[r0:r0 + r.shape[0], c0:c0 + r.shape[1]] = 0
                    before[r0:r0 + r.shape[0], c0:c0 + r.shape[1]] = 0
            if not torch.equal(now, before):
                return False
        return True


class Worst(dict):
    def see(self, name, got, ref, tol):
        self[name] = max(self.get(name, 0.0), L.worst(got, ref, tol)[0])

    def __str__(self):
        return " ".join(f"{k} {v:.3f}" for k, v in self.items())


def _check(what, kind, got, ref, tol, w, name):
    if kind == "exact":
        assert torch.equal(got.double(), ref), f"{what}: not the integer result at {(got.double() != ref).nonzero()[:5].tolist()}"
    else:
        w.see(f"{name}/{kind}", got, ref, tol)
    assert not L.judge(what, got, ref, tol)


# ------------------------------------------------------------------------------------------ down
def _down_buffers(M, K, R, layout):
    """-> X, A, T views and the parents"""
    if layout == "contig":
        xp, tp, ap = _nan(M + GUARD, K + 264), _nan(M + GUARD, _up8(R) + 16), _nan(R + GUARD, K)
        return xp[:M, :K], ap[:R], tp[:M, 8:8 + R], (xp, tp, ap)
    if layout == "fwd":
        buf, ap = _nan(M + GUARD, K + _up8(R) + 8), _nan(R + GUARD, K)
        return buf[:M, :K], ap[:R], buf[:M, K:K + R], (buf, ap)
    j = layout[1]                                                  # the backward layout: Dn = K, three slices, three adapters of rank R
    buf, ap = _nan(M + GUARD, 3 * K + 3 * R), torch.full((2, R, K), NAN, dtype=BF, device="cuda")
    return buf[:M, K:2 * K], ap[0], buf[:M, 3 * K + j * R:3 * K + (j + 1) * R], (buf, ap.view(2 * R, K))


@pytest.mark.parametrize("group", L.DOWN_GROUPS)
def test_down_every_arm(lib, group):
    w = Worst()
    for M, K, R, layout, kinds in L.down_cases(group):
        for kind in kinds:
            x, a = L.down_inputs(M, K, R, kind)
            X, A, T, parents = _down_buffers(M, K, R, layout)
            X.copy_(x.cuda())
            A.copy_(a.cuda())
            kept = Kept(*parents)
            lib.call("vgpa_lora_down", X, X.stride(0), A, T, T.stride(0), M, K, R, _stream())
            what = f"down {(M, K, R, layout, kind)}"
            assert kept.ok(T), f"{what}: wrote outside T"
            ref, S = L.down_ref64(X, A)
            _check(what, kind, T, ref, L.down_tol(ref, S, K), w, "down")
    print(f"down {group}: device / bound {w}")


# ------------------------------------------------------------------------------------------ up_add
def test_up_add_every_rank_and_edge(lib):
    w = Worst()
    for M, N, rp, s, acc in L.up_cases():
        for kind in ("exact", "randn", "mean"):
            t, b, y = L.up_inputs(M, N, rp, kind)
            sc = L.up_scale(s, kind)
            tp, bp, yp = _nan(M + GUARD, rp + 8), _nan(N + GUARD, rp + 8), _nan(M + GUARD, 8 + N + 16)
            T, B, Y = tp[:M, :rp], bp[:N, :rp], yp[:M, 8:8 + N]
            T.copy_(t.cuda())
            B.copy_(b.cuda())
            if acc:
                Y.copy_(y.cuda())
            ref, dot, S = L.up_ref64(Y.clone() if acc else None, T, B, sc)
            kept = Kept(tp, bp, yp)
            lib.call("vgpa_lora_up_add", Y, Y.stride(0), T, T.stride(0), B, B.stride(0), sc, M, N, rp, acc, _stream())
            what = f"up_add {(M, N, rp, sc, acc, kind)}"
            assert kept.ok(Y), f"{what}: wrote outside Y"
            assert bool(torch.isfinite(Y).all()), f"{what}: a result is not finite"
            _check(what, kind, Y, ref, L.up_tol(ref, dot, S, sc, rp, acc), w, "up_add")
    print(f"up_add: device / bound {w}")


# ------------------------------------------------------------------------------------------ grad
def _grad_once(lib, U, V, M, P, Q, ldg, ws_bytes):
    gp = _nan(P + GUARD, ldg, torch.float32)
    ws = torch.full((ws_bytes // 4 + 64,), NAN, device="cuda")
    G = gp[:P, :Q]
    kept = Kept(gp)
    lib.call("vgpa_lora_grad_ws", U, U.stride(0), V, V.stride(0), G, ldg, L.GRAD_S, M, P, Q, ws, ws_bytes, _stream())
    clean = kept.ok(G) and bool(torch.isnan(ws[ws_bytes // 4:]).all())
    return G, clean


@pytest.mark.parametrize("P,Q", L.GRAD_PQ)
def test_grad_every_plan(lib, P, Q):
    w, regimes = Worst(), set()
    for i, (M, P_, Q_) in enumerate(c for c in L.grad_cases() if c[1:] == (P, Q)):
        plan = L.grad_plan(M, P, Q)
        regimes.add((plan["regime"], plan["last"] < 64))
        ws_bytes = lib.query("vgpa_lora_grad_workspace_bytes", M, P, Q)
        assert ws_bytes == plan["splits"] * P * Q * 4, f"grad {(M, P, Q)}: {ws_bytes // (4 * P * Q)} splits where the plan has {plan['splits']}"
        for kind in ("exact", "randn") + (("mean",) if (P, Q) == (192, 320) else ()):
            u, v = L.grad_inputs(M, P, Q, kind)
            par = _nan(M + GUARD, 8 + P + 8 + Q + 8)
            U, V = par[:M, 8:8 + P], par[:M, 16 + P:16 + P + Q]
            U.copy_(u.cuda())
            V.copy_(v.cuda())
            kept = Kept(par)
            ldg = Q + 8 * ((i + (kind == "randn")) % 2)
            G, clean = _grad_once(lib, U, V, M, P, Q, ldg, ws_bytes)
            G2, clean2 = _grad_once(lib, U, V, M, P, Q, ldg, ws_bytes)
            what = f"grad {(M, P, Q, kind)} ldg {ldg} {plan['splits']} splits"
            assert clean and clean2 and kept.ok(), f"{what}: wrote outside G or its workspace"
            assert torch.equal(G, G2), f"{what}: two launches differ"
            ref, S = L.grad_ref64(U, V, L.GRAD_S)
            _check(what, kind, G, ref, L.grad_tol(ref, S, L.GRAD_S, M), w, "grad")
    if (P, Q) == (8, 8):
        assert regimes >= {("one", True), ("one", False), ("rows", True), ("rows", False)}, regimes       # M = 1300: six splits of 256 rows, the last of 20
    if (P, Q) == (3072, 64):
        assert regimes >= {("target", True), ("target", False)}, regimes                                 # M = 4810 / 5000: 768 / 48 = 16 splits of 320 rows, the last of 10 / 200
    print(f"grad {(P, Q)}: device / bound {w}")


# ------------------------------------------------------------------------------------------ refresh
@pytest.mark.parametrize("r,K,Dn,s", L.REFRESH_CASES)
def test_ext_refresh_is_bit_exact(lib, r, K, Dn, s):
    A, B, planted = L.refresh_inputs(r, K, Dn, s)
    assert planted > 0
    A, B = A.cuda(), B.cuda()
    ap, wtp, wp, sp = _nan(r + GUARD, K), _nan(K + GUARD, 8 + r + 8), _nan(Dn + GUARD, 16 + r + 8), _nan(r + GUARD, Dn)
    a_cat, wt, wv, sbt = ap[:r], wtp[:K, 8:8 + r], wp[:Dn, 16:16 + r], sp[:r]
    kept = Kept(ap, wtp, wp, sp)
    lib.call("vgpa_lora_ext_refresh", A, B, s, r, K, Dn, a_cat, wt, wt.stride(0), wv, wv.stride(0), sbt, _stream())
    assert kept.ok(a_cat, wt, wv, sbt), "refresh wrote outside its four results"
    a, sB = L.refresh_ref(A, B, s)
    for name, got, want in (("a_cat", a_cat, a), ("wt_tail", wt, a.t()), ("w_tail", wv, sB), ("sbt", sbt, sB.t())):
        assert torch.equal(_bits(got.contiguous()), _bits(want.contiguous())), f"refresh {(r, K, Dn)}: {name} is not the torch statement's"
    assert not torch.equal(sB, (B * s).to(BF))                                     # the planted values: a kernel that rounds B once would differ


# ------------------------------------------------------------------------------------------ refusals
def test_lora_entries_refuse_what_no_kernel_handles(lib):
    """VGPA_ERR_INVALID (-1) or VGPA_ERR_WORKSPACE (-3) before any launch.  Every buffer is 64 rows of 16 384 zeros, so a call accepted by mistake would still be a valid
    launch at any width or stride used here."""
    Lb = lib.load()
    big = lambda dt=BF: torch.zeros(64, 16384, dtype=dt, device="cuda")
    X, A, T, Y, Bw, U, V = (big() for _ in range(7))
    G, ws, Af, Bf = (big(torch.float32) for _ in range(4))
    st = _stream()
    p = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()

    def down(X=X, ldx=128, A=A, T=T, ldt=64, M=8, K=128, R=33):
        return Lb.vgpa_lora_down(p(X), ldx, p(A), p(T), ldt, M, K, R, st)

    def up(Y=Y, ldy=96, T=T, ldt=64, Bw=Bw, ldb=64, M=8, N=96, rp=64, acc=1):
        return Lb.vgpa_lora_up_add(p(Y), ldy, p(T), ldt, p(Bw), ldb, 2.0, M, N, rp, acc, st)

    need = Lb.vgpa_lora_grad_workspace_bytes(300, 16, 72)

    def grad(U=U, ldu=16, V=V, ldv=72, G=G, ldg=72, M=300, P=16, Q=72, ws=ws, nb=None):
        return Lb.vgpa_lora_grad_ws(p(U), ldu, p(V), ldv, p(G), ldg, 0.5, M, P, Q, p(ws), Lb.vgpa_lora_grad_workspace_bytes(M, P, Q) if nb is None else nb, st)

    def refresh(A=Af, B=Bf, r=12, K=64, Dn=40, a_cat=X, wt=T, ld_wt=16, wv=Y, ld_w=24, sbt=Bw):
        return Lb.vgpa_lora_ext_refresh(p(A), p(B), 1.5, r, K, Dn, p(a_cat), p(wt), ld_wt, p(wv), ld_w, p(sbt), st)

    accepted = [down(), down(ldx=136, ldt=40), down(R=256, ldt=256), up(), up(ldy=104, ldt=72, ldb=72, acc=0), up(rp=192, ldt=192, ldb=192), grad(), grad(ldg=80, ldu=24, ldv=80),
                refresh(), refresh(ld_wt=12, ld_w=12)]
    assert all(rc == 0 for rc in accepted), accepted
    assert need == 2 * 16 * 72 * 4 and Lb.vgpa_lora_grad_workspace_bytes(0, 16, 72) == 0
    refused = {
        "down X NULL": down(X=None), "down A NULL": down(A=None), "down T NULL": down(T=None), "down M 0": down(M=0), "down K 0": down(K=0), "down K % 64": down(K=96),
        "down R 0": down(R=0), "down R 257": down(R=257, ldt=264), "down ldx % 8": down(ldx=132), "down ldt % 8": down(ldt=60), "down ldt < R": down(ldt=32),
        "down ldx < K": down(ldx=120), "down ldx 0": down(ldx=0), "down ldx < 0": down(ldx=-128), "down X off 16 bytes": down(X=X.data_ptr() + 8),
        "down A off 16 bytes": down(A=A.data_ptr() + 8), "down T off 8 bytes": down(T=T.data_ptr() + 4), "down T odd": down(T=T.data_ptr() + 2), "down M > 2^36": down(M=(1 << 36) + 1),
        "up Y NULL": up(Y=None), "up T NULL": up(T=None), "up Bw NULL": up(Bw=None), "up M 0": up(M=0), "up N 0": up(N=0), "up N % 8": up(N=100, ldy=104),
        "up ldy % 8": up(ldy=100), "up ldt % 8": up(ldt=68), "up ldb % 8": up(ldb=68), "up Y off 16 bytes": up(Y=Y.data_ptr() + 8), "up T off 16 bytes": up(T=T.data_ptr() + 8),
        "up Bw off 16 bytes": up(Bw=Bw.data_ptr() + 8), "up rp 80": up(rp=80, ldt=80, ldb=80), "up rp 0": up(rp=0), "up rp 256": up(rp=256, ldt=256, ldb=256),
        "up ldy < N": up(ldy=88), "up ldy < 0": up(ldy=-96), "up ldt < rp": up(ldt=56), "up ldt 0": up(ldt=0), "up ldb < rp": up(ldb=56), "up ldb < 0": up(ldb=-64),
        "grad U NULL": grad(U=None), "grad V NULL": grad(V=None), "grad G NULL": grad(G=None), "grad workspace NULL": grad(ws=None), "grad M 0": grad(M=0, nb=need),
        "grad P 0": grad(P=0, nb=need), "grad Q 0": grad(Q=0, nb=need), "grad P % 8": grad(P=20, ldu=24), "grad Q % 8": grad(Q=76, ldv=80, ldg=80), "grad ldu % 8": grad(ldu=20),
        "grad ldv % 8": grad(ldv=76), "grad U off 16 bytes": grad(U=U.data_ptr() + 8), "grad V off 16 bytes": grad(V=V.data_ptr() + 8),
        "grad workspace off 16 bytes": grad(ws=ws.data_ptr() + 8), "grad ldu < P": grad(ldu=8), "grad ldu < 0": grad(ldu=-16), "grad ldv < Q": grad(ldv=64), "grad ldg < Q": grad(ldg=64),
        "grad ldg < 0": grad(ldg=-72), "grad G off 4 bytes": grad(G=G.data_ptr() + 2),
        "refresh A NULL": refresh(A=None), "refresh B NULL": refresh(B=None), "refresh a_cat NULL": refresh(a_cat=None), "refresh wt NULL": refresh(wt=None),
        "refresh w NULL": refresh(wv=None), "refresh sbt NULL": refresh(sbt=None), "refresh r 0": refresh(r=0), "refresh K 0": refresh(K=0), "refresh Dn 0": refresh(Dn=0),
        "refresh ld_wt < r": refresh(ld_wt=8), "refresh ld_w < r": refresh(ld_w=8), "refresh 2^31 elements": refresh(r=1 << 16, K=1 << 15, ld_wt=1 << 16, ld_w=1 << 16),
    }
    assert all(rc == -1 for rc in refused.values()), {k: v for k, v in refused.items() if v != -1}
    M, P, Q = 1300, 16, 72
    full = Lb.vgpa_lora_grad_workspace_bytes(M, P, Q)
    assert full == 6 * P * Q * 4
    assert grad(M=M, nb=full - 1) == -3 and grad(M=M, nb=0) == -3
    torch.cuda.synchronize()
