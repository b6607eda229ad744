"""The one-wave-per-row LayerNorm / RMS-norm kernels (csrc/norm.hip, csrc/residual_ln.hip, csrc/wan.hip over csrc/row_ln.h), each entry called on raw buffers
at every chunk count NV = 1..8 and judged per element against fp64 with the bounds counted in tests/row_tol.py (tests/test_row_tol_host.py shows on the CPU that
those bounds reject wrong kernels).  Output buffers are filled with a sentinel first: padding columns and the rows past `rows` must keep it.  fp64 references are
computed on the device.  `-s` prints the largest device error over its bound per family and width.  -m gpu only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import row_tol as R

SENT = -776.0          # exact in bf16 and fp32: what every output buffer holds before a launch
GUARD = 4              # rows behind the last one that a launch must leave alone
F32, BF16 = 0, 1       # VGPA_DTYPE_*
_DT = {torch.float32: F32, torch.bfloat16: BF16}


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


def _buf(rows, D, ld=None, dtype=torch.bfloat16):
    """sentinel-filled [rows + GUARD, ld] and its [rows, D] view"""
    b = torch.full((rows + GUARD, ld or D), SENT, dtype=dtype, device="cuda")
    return b, b[:rows, :D]


def _vec(rows):
    b = torch.full((rows + GUARD,), SENT, device="cuda")
    return b, b[:rows]


def _untouched(b, rows, D=None):
    """the guard rows and (with D) the padding columns of a _buf / _vec still hold the sentinel"""
    ok = bool((b[rows:] == SENT).all())
    return ok and (D is None or D == b.shape[1] or bool((b[:rows, D:] == SENT).all()))


def _problems(pairs):
    return [m for name, got, ref, tol in pairs for m in R.judge(name, got, ref, tol)]


class Worst(dict):
    def see(self, name, got, ref, tol):
        self[name] = max(self.get(name, 0.0), R.worst(got, ref, tol)[0])

    def __str__(self):
        return " ".join(f"{k} {v:.3f}" for k, v in self.items())


# ------------------------------------------------------------------------------------------ CogVideoX: residual add + LayerNorm + modulation
def _cog(B, S, Lt, D):
    c = {k: dev(v) for k, v in R.cog_case(B, S, Lt, D).items()}
    m = c["mod"]
    c["s1p"], c["shift"] = R.cog_rows(m[:, 1], m[:, 3], B, S, Lt), R.cog_rows(m[:, 0], m[:, 2], B, S, Lt)
    c["gfull"] = R.cog_rows(c["gates"][:, 0], c["gates"][:, 1], B, S, Lt)
    c["xn"] = R.cog_x_new(c, B, S, Lt)
    return c


def _mod_ptrs(c, mod):
    m = c["mod"]
    return (m[:, 0], m[:, 1], m[:, 2], m[:, 3]) if mod else (None, None, None, None)


def _residual_ln_fwd(lib, c, B, S, Lt, D, with_y, mod, ld, q8=False):
    """-> (x_new view or None, n view or (q, scale), mean, rstd, clean?)"""
    rows = B * S
    g = c["gates"]
    sh_v, sc_v, sh_t, sc_t = _mod_ptrs(c, mod)
    xb, xv = _buf(rows, D) if with_y else (None, None)
    mb, mean = _vec(rows)
    rb, rstd = _vec(rows)
    head = (c["x"], c["y"] if with_y else None, g[:, 0] if with_y else None, g[:, 1] if with_y else None, g.stride(0), c["w"], c["b"], sh_v, sc_v, sh_t, sc_t,
            c["mod"].stride(0), B, S, D, Lt, 1e-5, xv)
    if q8:
        q = torch.full((rows + GUARD, D), 0x55, dtype=torch.uint8, device="cuda")
        sb, sc = _vec(rows)
        lib.call("vgpa_residual_ln_fwd_q8", *head, q, sc, mean, rstd, _stream())
        clean = bool((q[rows:] == 0x55).all()) and _untouched(sb, rows)
        out = (q[:rows], sc)
    else:
        nb, out = _buf(rows, D, ld)
        lib.call("vgpa_residual_ln_fwd", *head, out, ld, mean, rstd, _stream())
        clean = _untouched(nb, rows, D)
    torch.cuda.synchronize()
    clean = clean and _untouched(mb, rows) and _untouched(rb, rows) and (xb is None or _untouched(xb, rows))
    return xv, out, mean, rstd, clean


# residual_ln_fwd_kernel<NV, HAS_Y>: blocks of 32 rows aligned to the (batch, text | video) ranges, 8 rows per wave; the row is NV chunks of 512 columns.
#   widths R.ROW_WIDTHS     one per NV = 1..8, full and partly filled last chunks alternating; 8 and 4096 the extremes (one lane of one chunk; every lane of all eight)
#   layouts R.COG_LAYOUTS   (2, 37, 6) text fills part of one wave, video ends inside wave 3; (3, 70, 33) two blocks per range; (2, 33, 0) / (2, 33, 33) one range empty;
#                           (3, 5, 2) both ranges inside one wave (the three small ones up to D = 1288)
@pytest.mark.parametrize("D", R.ROW_WIDTHS)
def test_residual_ln_fwd_every_width(lib, D):
    w = Worst()
    for B, S, Lt in R.cog_layouts(D):
        c = _cog(B, S, Lt, D)
        for with_y in (True, False):
            xn = c["xn"] if with_y else c["x"]
            for mod in (True, False):
                s1p, shift = (c["s1p"], c["shift"]) if mod else (None, None)
                ref = R.cog_ln_fwd_ref64(xn, c["w"], c["b"], s1p, shift, 1e-5)
                tols = R.cog_ln_fwd_tol(xn, c["w"], c["b"], s1p, shift, 1e-5, ref[0])
                for ld in (D, D + 64):
                    xv, n, mean, rstd, clean = _residual_ln_fwd(lib, c, B, S, Lt, D, with_y, mod, ld)
                    what = f"residual_ln_fwd D {D} {(B, S, Lt)} y {with_y} mod {mod} ld {ld}"
                    assert clean, f"{what}: wrote outside its rows or columns"
                    if with_y:
                        assert torch.equal(xv.view(B, S, D), xn), f"{what}: x_new is not bf16(x + bf16(gate y))"
                    got = (n.reshape(B, S, D), mean.view(B, S), rstd.view(B, S))
                    for i, name in enumerate(("n", "mean", "rstd")):
                        w.see(name, got[i], ref[i], tols[i])
                    assert not _problems((f"{what} {name}", got[i], ref[i], tols[i]) for i, name in enumerate(("n", "mean", "rstd")))
    print(f"residual_ln_fwd D {D}: device / bound {w}")


def _cog_bwd_ref(c, xn, mean, rstd, mod, dres):
    alpha = c["w"].double() * c["s1p"].double() if mod else c["w"].double()
    g = c["dn"].double() * alpha
    B, S, _ = xn.shape
    ref = R.ln_bwd_ref64(g, xn, mean.view(B, S), rstd.view(B, S), dres)
    return ref, R.bf16_tol(ref, R.ln_bwd_rest(g, xn, mean.view(B, S), rstd.view(B, S), 2.0 if mod else 0.0, dres))


# residual_ln_bwd_kernel<NV, HAS_DRES, HAS_DY>: 32 instantiations, every one launched here (8 widths NV x 4 forms), on the fp32 mean / rstd the forward wrote
@pytest.mark.parametrize("D", R.ROW_WIDTHS)
def test_residual_ln_bwd_every_width(lib, D):
    w = Worst()
    for B, S, Lt in R.cog_layouts(D):
        rows = B * S
        c = _cog(B, S, Lt, D)
        g = c["gates"]
        for mod in (True, False):
            _, _, mean, rstd, _ = _residual_ln_fwd(lib, c, B, S, Lt, D, True, mod, D)
            sc_v, sc_t = (c["mod"][:, 1], c["mod"][:, 3]) if mod else (None, None)
            for dres in (c["dres"], None):
                ref, tol = _cog_bwd_ref(c, c["xn"], mean, rstd, mod, dres)
                for with_dy, ld in ((False, D), (True, D), (True, D + 64)):
                    dxb, dx = _buf(rows, D)
                    dyb, dy = _buf(rows, D, ld)
                    lib.call("vgpa_residual_ln_bwd", c["dn"], c["xn"], mean, rstd, c["w"], sc_v, sc_t, c["mod"].stride(0), g[:, 0] if with_dy else None,
                             g[:, 1] if with_dy else None, g.stride(0), dres, B, S, D, Lt, dx, dy if with_dy else None, ld, _stream())
                    torch.cuda.synchronize()
                    what = f"residual_ln_bwd D {D} {(B, S, Lt)} mod {mod} dres {dres is not None} dy {with_dy} ld {ld}"
                    assert _untouched(dxb, rows) and _untouched(dyb, rows, D if with_dy else 0), f"{what}: wrote outside its rows or columns"
                    w.see("dx", dx.view(B, S, D), ref, tol)
                    assert not R.judge(f"{what} dx", dx.view(B, S, D), ref, tol)
                    if with_dy:
                        assert torch.equal(dy.reshape(B, S, D), (c["gfull"] * dx.view(B, S, D).float()).to(torch.bfloat16)), f"{what}: dy is not bf16(gate dx)"
    print(f"residual_ln_bwd D {D}: device / bound {w}")


# ln_modulate_{fwd,bwd}_kernel<NV> (v1): blocks of 16 consecutive rows, 4 per wave, the affine reloaded when a wave's rows cross a range or batch boundary:
# (3, 5, 2) puts both boundaries inside one wave and is run at every width
@pytest.mark.parametrize("D", R.ROW_WIDTHS)
def test_ln_modulate_v1_every_width(lib, D):
    w = Worst()
    for B, S, Lt in R.cog_layouts(D) + ([] if D <= 1288 else [R.COG_LAYOUTS[4]]):
        rows = B * S
        c = _cog(B, S, Lt, D)
        for mod in (True, False):
            sh_v, sc_v, sh_t, sc_t = _mod_ptrs(c, mod)
            s1p, shift = (c["s1p"], c["shift"]) if mod else (None, None)
            ref = R.cog_ln_fwd_ref64(c["x"], c["w"], c["b"], s1p, shift, 1e-5)
            tols = R.cog_ln_fwd_tol(c["x"], c["w"], c["b"], s1p, shift, 1e-5, ref[0])
            nb, n = _buf(rows, D)
            mb, mean = _vec(rows)
            rb, rstd = _vec(rows)
            lib.call("vgpa_ln_modulate_fwd", c["x"], c["w"], c["b"], sh_v, sc_v, sh_t, sc_t, c["mod"].stride(0), B, S, D, Lt, 1e-5, n, mean, rstd, _stream())
            torch.cuda.synchronize()
            what = f"ln_modulate v1 D {D} {(B, S, Lt)} mod {mod}"
            assert _untouched(nb, rows) and _untouched(mb, rows) and _untouched(rb, rows), f"{what}: forward wrote past its rows"
            got = (n.view(B, S, D), mean.view(B, S), rstd.view(B, S))
            for i, name in enumerate(("n", "mean", "rstd")):
                w.see(name, got[i], ref[i], tols[i])
            assert not _problems((f"{what} {name}", got[i], ref[i], tols[i]) for i, name in enumerate(("n", "mean", "rstd")))
            for dres in (c["dres"], None):
                gref, gtol = _cog_bwd_ref(c, c["x"], mean, rstd, mod, dres)
                dxb, dx = _buf(rows, D)
                lib.call("vgpa_ln_modulate_bwd", c["dn"], c["x"], mean, rstd, c["w"], sc_v, sc_t, c["mod"].stride(0), B, S, D, Lt, dres, dx, _stream())
                torch.cuda.synchronize()
                assert _untouched(dxb, rows), f"{what}: backward wrote past its rows"
                w.see("dx", dx.view(B, S, D), gref, gtol)
                assert not R.judge(f"{what} dres {dres is not None} dx", dx.view(B, S, D), gref, gtol)
    print(f"ln_modulate v1 D {D}: device / bound {w}")


# the e4m3 producers at all eight NV (they had run at NV 1, 4 and 6): the bytes and scales of the bf16 entry followed by quant_fp8_rows; x_new, mean, rstd and dx the
# bf16 entry's bits
@pytest.mark.parametrize("D", R.ROW_WIDTHS)
def test_q8_entries_every_width(ops, lib, D):
    B, S, Lt = R.COG_LAYOUTS[0]
    rows = B * S
    c = _cog(B, S, Lt, D)
    g = c["gates"]
    for with_y in (True, False):
        xv, n, mean, rstd, _ = _residual_ln_fwd(lib, c, B, S, Lt, D, with_y, True, D)
        xq, (q, sc), mean8, rstd8, clean = _residual_ln_fwd(lib, c, B, S, Lt, D, with_y, True, D, q8=True)
        rq, rs = ops.quant_fp8_rows(n)
        what = f"residual_ln_fwd_q8 D {D} y {with_y}"
        print(f"{what}: bytes differing {(q != rq.view(torch.uint8)).float().mean().item():.2e}")
        assert clean, f"{what}: wrote past its rows"
        assert torch.equal(mean8, mean) and torch.equal(rstd8, rstd) and (not with_y or torch.equal(xq, xv)), what
        assert torch.equal(sc, rs.view(-1)) and torch.equal(q, rq.view(torch.uint8)), what
    xn = c["xn"]
    _, _, mean, rstd, _ = _residual_ln_fwd(lib, c, B, S, Lt, D, True, True, D)
    for dres in (c["dres"], None):
        dx, dy, dx8 = (torch.empty_like(xn) for _ in range(3))
        q = torch.full((rows + GUARD, D), 0x55, dtype=torch.uint8, device="cuda")
        sb, sc = _vec(rows)
        tail = (dres, B, S, D, Lt)
        head = (c["dn"], xn, mean, rstd, c["w"], c["mod"][:, 1], c["mod"][:, 3], c["mod"].stride(0), g[:, 0], g[:, 1], g.stride(0))
        lib.call("vgpa_residual_ln_bwd", *head, *tail, dx, dy, D, _stream())
        lib.call("vgpa_residual_ln_bwd_q8", *head, *tail, dx8, q, sc, _stream())
        rq, rs = ops.quant_fp8_rows(dy.view(rows, D))
        what = f"residual_ln_bwd_q8 D {D} dres {dres is not None}"
        print(f"{what}: bytes differing {(q[:rows] != rq.view(torch.uint8)).float().mean().item():.2e}")
        assert bool((q[rows:] == 0x55).all()) and _untouched(sb, rows), f"{what}: wrote past its rows"
        assert torch.equal(dx8, dx), what
        assert torch.equal(sc, rs.view(-1)) and torch.equal(q[:rows], rq.view(torch.uint8)), what
    for xdt in (torch.float32, torch.bfloat16):                              # vgpa_wan_ln_mod_fwd with q8, next to out and alone
        rows = 9
        k = {a: dev(b) for a, b in R.wan_ln_case(rows, D, xdt).items()}
        tab = k["tab"]
        out = torch.empty(rows, D, dtype=torch.bfloat16, device="cuda")
        lib.call("vgpa_wan_ln_mod_fwd", k["x"], _DT[xdt], None, None, None, k["gid"], k["w"], k["b"], tab[:, 3], tab[:, 4], tab.stride(0), rows, D, 1e-6, 0, out, BF16, D,
                 None, None, None, None, _stream())
        rq, rs = ops.quant_fp8_rows(out)
        for with_out in (True, False):
            out2 = torch.empty_like(out)
            q = torch.full((rows + GUARD, D), 0x55, dtype=torch.uint8, device="cuda")
            sb, sc = _vec(rows)
            lib.call("vgpa_wan_ln_mod_fwd", k["x"], _DT[xdt], None, None, None, k["gid"], k["w"], k["b"], tab[:, 3], tab[:, 4], tab.stride(0), rows, D, 1e-6, 0,
                     out2 if with_out else None, BF16, D, q, sc, None, None, _stream())
            torch.cuda.synchronize()
            what = f"wan_ln_mod_fwd q8 D {D} {xdt} out {with_out}"
            assert bool((q[rows:] == 0x55).all()) and _untouched(sb, rows), f"{what}: wrote past its rows"
            assert not with_out or torch.equal(out2, out), what
            assert torch.equal(sc, rs.view(-1)) and torch.equal(q[:rows], rq.view(torch.uint8)), what


# ------------------------------------------------------------------------------------------ Wan: LayerNorm + per-token modulation
def _wan_fwd_call(lib, k, xdt, rows, D, affine, mod, rnd, out_dt, x=None, y=None, gate=None, x_out=None):
    tab = k["tab"]
    ob, out = _buf(rows, D, D + 64, out_dt)
    mb, mean = _vec(rows)
    rb, rstd = _vec(rows)
    lib.call("vgpa_wan_ln_mod_fwd", k["x"] if x is None else x, _DT[xdt], y, gate, x_out, k["gid"] if (mod or gate is not None) else None, k["w"] if affine else None,
             k["b"] if affine else None, tab[:, 3] if mod else None, tab[:, 4] if mod else None, tab.stride(0), rows, D, 1e-6, rnd, out, _DT[out_dt], D + 64,
             None, None, mean, rstd, _stream())
    torch.cuda.synchronize()
    return out, mean, rstd, _untouched(ob, rows, D) and _untouched(mb, rows) and _untouched(rb, rows)


def _wan_fwd_judge(w, what, k, x, rows, D, affine, mod, rnd, out_bf16, got):
    a = (x, k["gid"] if mod else None, k["w"] if affine else None, k["b"] if affine else None, k["tab"][:, 3] if mod else None, k["tab"][:, 4] if mod else None, 1e-6)
    ref = R.wan_ln_fwd_ref64(*a)
    tols = R.wan_ln_fwd_tol(*a, rnd, ref[0], out_bf16)
    for i, name in enumerate(("out", "mean", "rstd")):
        w.see("fwd " + name, got[i], ref[i], tols[i])
    assert not _problems((f"{what} {name}", got[i], ref[i], tols[i]) for i, name in enumerate(("out", "mean", "rstd")))


def _wan_forms():
    for xdt in (torch.float32, torch.bfloat16):
        for affine in (False, True):
            for mod in (False, True):
                for rnd in (0, 1):
                    yield xdt, affine, mod, rnd, torch.bfloat16
    yield torch.float32, False, True, 0, torch.float32
    yield torch.float32, False, False, 0, torch.float32


# wan_ln_mod_fwd_kernel: one wave per row, 4 per workgroup, always WAN_NV = 8 chunks of which ceil(D / 512) are live.
#   rows 1, 5, 9     three waves of the only workgroup idle; a second and a third workgroup holding one row each
#   D 8 .. 4096      one lane; a partly filled first chunk (264); a second chunk of one lane (520); six full; 4088 = all eight with the last lane idle; all lanes
# out_ld = D + 64; shift / scale / gates are slices of one [3, 6, D] table (mod_stride 6 D) and gid runs 2, 0, 1, 0, 2, 1, ...
@pytest.mark.parametrize("D", R.WAN_LN_WIDTHS)
def test_wan_ln_mod_fwd_every_form(lib, D):
    w = Worst()
    for rows in R.WAN_LN_ROWS:
        ks = {xdt: {a: dev(b) for a, b in R.wan_ln_case(rows, D, xdt).items()} for xdt in (torch.float32, torch.bfloat16)}
        for xdt, affine, mod, rnd, out_dt in _wan_forms():
            k = ks[xdt]
            out, mean, rstd, clean = _wan_fwd_call(lib, k, xdt, rows, D, affine, mod, rnd, out_dt)
            what = f"wan_ln_mod_fwd D {D} rows {rows} {xdt} affine {affine} mod {mod} round_xhat {rnd} -> {out_dt}"
            assert clean, f"{what}: wrote outside its rows or columns"
            _wan_fwd_judge(w, what, k, k["x"], rows, D, affine, mod, rnd, out_dt == torch.bfloat16, (out, mean, rstd))
            if rnd and not affine and not mod:           # two exactly rounded fp32 operations and the store: what a missing intermediate rounding cannot equal ...
                assert torch.equal(out, ((k["x"].float() - mean[:, None]) * rstd[:, None]).to(torch.bfloat16)), f"{what}: not bf16((x - mean) rstd)"
            if rnd and affine and not mod:               # ... and behind the affine: bf16(bf16(xhat) w + b), the sum within its last fp32 bit of either contraction
                xh = ((k["x"].float() - mean[:, None]) * rstd[:, None]).to(torch.bfloat16).double()
                v = xh * k["w"].double() + k["b"].double()
                e = 2.0 * R.U * ((xh * k["w"].double()).abs() + v.abs())
                assert not R.judge(f"{what} from the rounded xhat", out, v, R.bf16_tol(v, e))
        # GR: x' = x + y gate[g] (gate NULL = 1) stored as fp32 and normalised in the same pass
        k = ks[torch.float32]
        for gate in (k["tab"][:, 2], None):
            xref, xtol = R.wan_gate_ref64(k["x"], k["y"], k["gid"], gate)
            for affine in (False, True):
                for mod in (False, True):
                    xb, xo = _buf(rows, D, None, torch.float32)
                    out, mean, rstd, clean = _wan_fwd_call(lib, k, torch.float32, rows, D, affine, mod, 0, torch.bfloat16, y=k["y"], gate=gate, x_out=xo)
                    what = f"wan_ln_mod_fwd GR D {D} rows {rows} gate {gate is not None} affine {affine} mod {mod}"
                    assert clean and _untouched(xb, rows), f"{what}: wrote outside its rows or columns"
                    w.see("x_out", xo, xref, xtol)
                    assert not R.judge(f"{what} x_out", xo, xref, xtol)
                    _wan_fwd_judge(w, what, k, xo, rows, D, affine, mod, 0, True, (out, mean, rstd))
    print(f"wan_ln_mod_fwd D {D}: device / bound {w}")


# wan_ln_mod_bwd_kernel: dy bf16 with x fp32 | bf16; GB (dy_prev = bf16(dx gate_prev[g]), ld_dy_prev = D + 64); dy fp32 (the output head).  dres absent, a buffer of
# its own, and the dx buffer itself
@pytest.mark.parametrize("D", R.WAN_LN_WIDTHS)
def test_wan_ln_mod_bwd_every_form(lib, D):
    w = Worst()
    for rows in R.WAN_LN_ROWS:
        for xdt in (torch.float32, torch.bfloat16):
            k = {a: dev(b) for a, b in R.wan_ln_case(rows, D, xdt).items()}
            tab = k["tab"]
            _, mean, rstd, _ = _wan_fwd_call(lib, k, xdt, rows, D, False, False, 0, torch.bfloat16)
            forms = [("bf16", af, md, dr, None) for af in (False, True) for md in (False, True) for dr in (None, "own", "alias")]
            if xdt == torch.float32:
                forms += [("gb", af, md, dr, gp) for af, md in ((True, True), (False, False)) for dr in ("own", "alias") for gp in (True, False)]
                forms += [("fp32", False, md, None, None) for md in (True, False)]
            for kind, affine, mod, dres_kind, gp in forms:
                dy = k["dy32"] if kind == "fp32" else k["dy"]
                gid = k["gid"] if (mod or gp) else None
                wt, scale = k["w"] if affine else None, tab[:, 4] if mod else None
                g, cg = R.wan_ln_bwd_g64(dy, gid, wt, scale)
                dres = None if dres_kind is None else k["dres"]
                ref = R.ln_bwd_ref64(g, k["x"], mean, rstd, dres)
                tol = R.ln_bwd_rest(g, k["x"], mean, rstd, cg, dres)
                dxb, dx = _buf(rows, D, None, torch.float32)
                if dres_kind == "alias":
                    dx.copy_(dres)
                pb, dyp = _buf(rows, D, D + 64)
                lib.call("vgpa_wan_ln_mod_bwd", dy, _DT[dy.dtype], k["x"], _DT[xdt], mean, rstd, gid, wt, scale, tab.stride(0), rows, D,
                         dx if dres_kind == "alias" else dres, dx, tab[:, 5] if gp else None, dyp if kind == "gb" else None, D + 64, _stream())
                torch.cuda.synchronize()
                what = f"wan_ln_mod_bwd D {D} rows {rows} {xdt} {kind} affine {affine} mod {mod} dres {dres_kind} gate_prev {gp}"
                assert _untouched(dxb, rows) and _untouched(pb, rows, D if kind == "gb" else 0), f"{what}: wrote outside its rows or columns"
                w.see("dx " + kind, dx, ref, tol)
                assert not R.judge(f"{what} dx", dx, ref, tol)
                if kind == "gb":
                    want = (dx * tab[:, 5][gid.long()]) if gp else dx
                    assert torch.equal(dyp, want.to(torch.bfloat16)), f"{what}: dy_prev is not bf16(dx gate_prev)"
    print(f"wan_ln_mod_bwd D {D}: device / bound {w}")


# ------------------------------------------------------------------------------------------ Wan: RMS-norm + RoPE
# wan_rms_rope_{fwd,bwd}_kernel: L = 7, B = 3: 21 rows, the sixth workgroup holds one row (`row >= rows` leaves three waves) and `row % L` wraps inside a workgroup.
#   (264, 24) (264, 8)   a partly filled first chunk; heads of 24 (a lane's eight columns straddle no head, the table offset is 0, 4, 8) and of 8 (one lane = one head)
#   (520, 40)            the second chunk holds one lane; (3072, 128), (4096, 128) the model's head width, six and eight full chunks
# "fused": u / out / dout / du are the middle column slice of [rows, 3 D] buffers (ld = 3 D)
@pytest.mark.parametrize("D,hd", R.RMS_SHAPES)
@pytest.mark.parametrize("tables", [True, False])
def test_wan_rms_rope_every_shape(lib, tables, D, hd):
    rows, L = R.RMS_B * R.RMS_L, R.RMS_L
    k = {a: dev(b) for a, b in R.rms_case(D, hd).items()}
    cos, sin = (k["cos"], k["sin"]) if tables else (None, None)
    ref, rs_ref = R.rms_rope_ref64(k["u"], k["w"], cos, sin, L, hd, 1e-6)
    tol, tol_rs = R.rms_rope_fwd_tol(k["u"], k["w"], cos, sin, L, hd, 1e-6, ref)
    w = Worst()
    for fused in (True, False):
        ld = 3 * D if fused else D
        col = slice(D, 2 * D) if fused else slice(0, D)
        src = torch.full((rows, ld), 1000.0, dtype=torch.bfloat16, device="cuda")            # read by mistake, the neighbours would show in every sum
        src[:, col] = k["u"]
        gsrc = torch.full((rows, ld), 1000.0, dtype=torch.bfloat16, device="cuda")
        gsrc[:, col] = k["dout"]
        ob = torch.full((rows + GUARD, ld), SENT, dtype=torch.bfloat16, device="cuda")
        rb, rs = _vec(rows)
        lib.call("vgpa_wan_rms_rope_fwd", src[:, col], ld, k["w"], cos, sin, L, hd, rows, D, 1e-6, ob[:, col], ld, rs, _stream())
        torch.cuda.synchronize()
        what = f"wan_rms_rope D {D} head_dim {hd} tables {tables} fused {fused}"
        out = ob[:rows, col]
        ob_rest = ob.clone()
        ob_rest[:rows, col] = SENT
        assert bool((ob_rest == SENT).all()) and _untouched(rb, rows), f"{what}: forward wrote outside its slice"
        w.see("out", out, ref, tol)
        w.see("rstd", rs, rs_ref, tol_rs)
        assert not _problems(((f"{what} out", out, ref, tol), (f"{what} rstd", rs, rs_ref, tol_rs)))
        if not tables:
            want = ((k["u"].float() * rs[:, None]).to(torch.bfloat16).float() * k["w"].float()).to(torch.bfloat16)
            assert torch.equal(out, want), f"{what}: not bf16(bf16(u rs) w)"
        gref = R.rms_rope_bwd_ref64(k["dout"], k["u"], rs, k["w"], cos, sin, L, hd)
        gtol = R.rms_rope_bwd_tol(k["dout"], k["u"], rs, k["w"], cos, sin, L, hd, gref)
        db = torch.full((rows + GUARD, ld), SENT, dtype=torch.bfloat16, device="cuda")
        lib.call("vgpa_wan_rms_rope_bwd", gsrc[:, col], ld, src[:, col], ld, rs, k["w"], cos, sin, L, hd, rows, D, db[:, col], ld, _stream())
        torch.cuda.synchronize()
        du = db[:rows, col]
        db_rest = db.clone()
        db_rest[:rows, col] = SENT
        assert bool((db_rest == SENT).all()), f"{what}: backward wrote outside its slice"
        w.see("du", du, gref, gtol)
        assert not R.judge(f"{what} du", du, gref, gtol)
    print(f"wan_rms_rope D {D} head_dim {hd} tables {tables}: device / bound {w}")


# ------------------------------------------------------------------------------------------ Wan: gated residual add and its backward
def _gate_check(lib, what, x, y, gid, gate, tab_stride, rows, D, alias=False):
    ref, tol = R.wan_gate_ref64(x, y, gid, gate)
    ob, out = _buf(rows, D, None, torch.float32)
    if alias:
        out.copy_(x)
    lib.call("vgpa_wan_gate_residual", out if alias else x, y, gid, gate, tab_stride, rows, D, out, _stream())
    torch.cuda.synchronize()
    assert _untouched(ob, rows), f"{what}: wrote past its rows"
    return out, ref, tol


def _gate_bwd_check(lib, what, dout, gid, gate, tab_stride, rows, D, ld):
    db, dy = _buf(rows, D, ld)
    lib.call("vgpa_wan_gate_bwd", dout, gid, gate, tab_stride, rows, D, dy, ld, _stream())
    torch.cuda.synchronize()
    assert _untouched(db, rows, D), f"{what}: wrote outside its rows or columns"
    want = dout if gate is None else dout * gate[torch.zeros(rows, dtype=torch.long, device="cuda") if gid is None else gid.long()]
    return dy, want.to(torch.bfloat16)


# wan_gate_residual_kernel / wan_gate_bwd_kernel at rows = 5, D = 264: 165 vectors of eight in one workgroup of 256, every optional pointer present and absent
def test_wan_gate_residual_and_bwd_small(lib):
    rows, D = 5, 264
    k = {a: dev(b) for a, b in R.wan_ln_case(rows, D).items()}
    tab, gid = k["tab"], k["gid"]
    y = (k["y"].float() + k["dy"].float()).to(torch.bfloat16)                  # the case's y is zero in the planted rows
    for name, x, gi, gate, alias in (("all", k["x"], gid, tab[:, 2], False), ("x NULL", None, gid, tab[:, 2], False), ("gate NULL", k["x"], None, None, False),
                                      ("gid NULL", k["x"], None, tab[:, 2], False), ("out = x", k["x"], gid, tab[:, 2], True)):
        out, ref, tol = _gate_check(lib, f"wan_gate_residual {name}", x, y, gi, gate, tab.stride(0), rows, D, alias)
        print(f"wan_gate_residual {name}: device / bound {R.worst(out, ref, tol)[0]:.3f}")
        assert not R.judge(f"wan_gate_residual {name}", out, ref, tol)
    for name, gi, gate, ld in (("all", gid, tab[:, 2], D), ("ld D + 64", gid, tab[:, 2], D + 64), ("gate NULL", None, None, D + 64), ("gid NULL", None, tab[:, 2], D)):
        dy, want = _gate_bwd_check(lib, f"wan_gate_bwd {name}", k["dres"], gi, gate, tab.stride(0), rows, D, ld)
        assert torch.equal(dy, want), f"wan_gate_bwd {name}: not bf16(dout gate)"


# wan_ew_grid caps the grid at 65 536 blocks of 256: rows = 32 776, D = 4096 is 16 781 312 vectors of eight against 16 777 216 threads, so the last 8 rows are the
# second trip of the grid-stride loop.  They are asserted first and separately: a dropped second trip names itself
CAP_ROWS, CAP_D = 32776, 4096


def _cap_inputs():
    g = torch.Generator(device="cuda").manual_seed(65536)
    gid = (torch.arange(CAP_ROWS, device="cuda") % 3).int()
    tab = 0.5 * torch.randn(3, 6, CAP_D, device="cuda", generator=g)
    return g, gid, tab


def test_wan_gate_residual_at_the_grid_cap(lib):
    g, gid, tab = _cap_inputs()
    x = torch.randn(CAP_ROWS, CAP_D, device="cuda", generator=g) * 2 + 0.3
    y = torch.randn(CAP_ROWS, CAP_D, device="cuda", generator=g).to(torch.bfloat16)
    out, ref, tol = _gate_check(lib, "wan_gate_residual at the cap", x, y, gid, tab[:, 2], tab.stride(0), CAP_ROWS, CAP_D)
    last = slice(CAP_ROWS - 8, CAP_ROWS)
    assert not R.judge("wan_gate_residual, the last 8 rows (second trip of the loop)", out[last], ref[last], tol[last])
    print(f"wan_gate_residual at the cap: device / bound {R.worst(out, ref, tol)[0]:.3f}")
    assert not R.judge("wan_gate_residual at the cap", out, ref, tol)


def test_wan_gate_bwd_at_the_grid_cap(lib):
    g, gid, tab = _cap_inputs()
    dout = torch.randn(CAP_ROWS, CAP_D, device="cuda", generator=g)
    dy, want = _gate_bwd_check(lib, "wan_gate_bwd at the cap", dout, gid, tab[:, 2], tab.stride(0), CAP_ROWS, CAP_D, CAP_D)
    assert torch.equal(dy[CAP_ROWS - 8:], want[CAP_ROWS - 8:]), "wan_gate_bwd: the last 8 rows (second trip of the loop) are not bf16(dout gate)"
    assert torch.equal(dy, want)


# ------------------------------------------------------------------------------------------ refusals
def test_wan_rms_rope_and_gate_entries_refuse_what_no_kernel_handles(lib):
    """VGPA_ERR_INVALID before any launch.  Every buffer holds 8 rows of 16 384 fp32 elements and the tables as much, so a call accepted by mistake would still be a
    valid launch at any width, stride or table row used here."""
    L = lib.load()
    rows, D, hd, Lr = 8, 264, 24, 4
    big = lambda: torch.zeros(rows, 16384, device="cuda")
    u, wt, out, rs, dout, du, cos, sin, x, y, gate = (big() for _ in range(11))
    gid = torch.zeros(rows, dtype=torch.int32, device="cuda")
    st = _stream()
    p = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()

    def fwd(D=D, ld_u=D, ld_out=D, cos=cos, sin=sin, L_=Lr, hd=hd, rows=rows, u=u, out=out):
        return L.vgpa_wan_rms_rope_fwd(p(u), ld_u, p(wt), p(cos), p(sin), L_, hd, rows, D, 1e-6, p(out), ld_out, p(rs), st)

    def bwd(D=D, ld_dout=D, ld_u=D, ld_du=D, cos=cos, sin=sin, L_=Lr, hd=hd, rows=rows, rs=rs):
        return L.vgpa_wan_rms_rope_bwd(p(dout), ld_dout, p(u), ld_u, p(rs), p(wt), p(cos), p(sin), L_, hd, rows, D, p(du), ld_du, st)

    def gres(D=D, rows=rows, y=y, out=out):
        return L.vgpa_wan_gate_residual(p(x), p(y), p(gid), p(gate), D, rows, D, p(out), st)

    def gbwd(D=D, rows=rows, ld=D, dout=dout, dy=du):
        return L.vgpa_wan_gate_bwd(p(dout), p(gid), p(gate), D, rows, D, p(dy), ld, st)

    def gq8(D=D, rows=rows):
        return L.vgpa_wan_gate_bwd_q8(p(dout), p(gid), p(gate), D, rows, D, p(out), p(rs), st)

    accepted = [fwd(), bwd(), fwd(cos=None, sin=None), bwd(cos=None, sin=None), fwd(cos=None, sin=None, L_=0, hd=0), fwd(ld_u=D + 8, ld_out=3 * D), gres(), gbwd(),
                gbwd(ld=D + 64), gq8(), gres(D=4104), gbwd(D=4104, ld=4104)]        # the two element-wise entries have no width limit: they hold no row
    assert all(rc == 0 for rc in accepted), accepted
    off = cos.data_ptr() + 4
    refused = {
        "fwd D % 8": fwd(D=260, hd=20), "bwd D % 8": bwd(D=260, hd=20), "fwd D > 4096": fwd(D=4104, ld_u=4104, ld_out=4104), "bwd D > 4096": bwd(D=4104, ld_dout=4104, ld_u=4104, ld_du=4104),
        "fwd ld_u < D": fwd(ld_u=D - 8), "fwd ld_out < D": fwd(ld_out=D - 8), "fwd ld_u % 8": fwd(ld_u=D + 4), "fwd ld_out % 8": fwd(ld_out=D + 4),
        "bwd ld_dout < D": bwd(ld_dout=D - 8), "bwd ld_u < D": bwd(ld_u=D - 8), "bwd ld_du < D": bwd(ld_du=D - 8),
        "bwd ld_dout % 8": bwd(ld_dout=D + 4), "bwd ld_u % 8": bwd(ld_u=D + 4), "bwd ld_du % 8": bwd(ld_du=D + 4),
        "fwd cos without sin": fwd(sin=None), "fwd sin without cos": fwd(cos=None), "bwd cos without sin": bwd(sin=None), "bwd sin without cos": bwd(cos=None),
        "fwd cos off 16 bytes": fwd(cos=off), "fwd sin off 16 bytes": fwd(sin=sin.data_ptr() + 8),
        "fwd L 0": fwd(L_=0), "fwd L -1": fwd(L_=-1), "bwd L 0": bwd(L_=0),
        "fwd head_dim not dividing D": fwd(hd=40), "bwd head_dim not dividing D": bwd(hd=40), "fwd head_dim % 8": fwd(hd=12), "bwd head_dim % 8": bwd(hd=12),
        "fwd head_dim 0": fwd(hd=0), "fwd rows 0": fwd(rows=0), "bwd rows 0": bwd(rows=0), "fwd u NULL": fwd(u=None), "fwd out NULL": fwd(out=None), "bwd rstd NULL": bwd(rs=None),
        "gate_residual D % 8": gres(D=260), "gate_residual rows 0": gres(rows=0), "gate_residual y NULL": gres(y=None), "gate_residual out NULL": gres(out=None),
        "gate_bwd D % 8": gbwd(D=260, ld=264), "gate_bwd ld < D": gbwd(ld=D - 8), "gate_bwd ld % 8": gbwd(ld=D + 4), "gate_bwd rows 0": gbwd(rows=0),
        "gate_bwd dout NULL": gbwd(dout=None), "gate_bwd dy NULL": gbwd(dy=None), "gate_bwd_q8 D % 8": gq8(D=260), "gate_bwd_q8 D > 4096": gq8(D=4104),
    }
    assert all(rc == -1 for rc in refused.values()), {k: v for k, v in refused.items() if v != -1}
    torch.cuda.synchronize()
