"""tests/scorer_ref.py checked on the CPU: its fp64 references against the results the reference project stored (tests/golden/scorer.pt, scorer2.pt), every input
builder against the conditions it promises, the fp32 oracle's own distance from the fp64 reference against half of every cap, and `judge` against deliberately
wrong fp32 restatements on the families meant to catch them.  `-s` prints every family's oracle-to-fp64 distance and the rejected restatements."""
import os

import numpy as np
import torch

import scorer_ref as R
from oracle import scorer as osc

f32, f64 = np.float32, np.float64


def _load(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), weights_only=False)


# ---------------------------------------------------------------------------------------------- the references against the stored results
def test_fp64_references_agree_with_the_stored_reference_results(golden_dir):
    """tolerances: the ones tests/test_oracle_golden.py uses for the same quantity; where that file asks the fp32 oracle for equality (motion, same-size MSE), an fp64
    evaluation gets the cap of the quantity (2e-6) instead, and the float32 restatement of the pose decode is held to the equality"""
    g1, g2 = _load(golden_dir, "scorer.pt"), _load(golden_dir, "scorer2.pt")
    for c in g1["project"]:
        assert np.array_equal(R.splat_restated(c["pc"], c["colors"], c["K"], c["E"], c["H"], c["W"]), c["canvas"].numpy())
    for c in g1["motion"]:
        assert abs(R.motion(c["E"]) - c["score"]) <= 2e-6 * max(1.0, abs(c["score"]))
    for c in g1["mse"]:
        assert abs(R.frame_metric(c["gt"], c["rep"]) - c["val"]) <= 2e-6 * c["val"]
    for c in g2["psnr"]:
        assert abs(R.frame_metric(c["gt"], c["rep"], psnr=True) - c["val"]) <= 2e-5 * max(1.0, abs(c["val"]))
    for c in g2["mse_resize"]:
        assert abs(R.frame_metric(c["gt"], c["rep"]) - c["val"]) <= 2e-6 * max(1.0, abs(c["val"]))
    for c in g2["mvcs"]:
        got = R.mvcs(c["depths"].numpy(), c["intrinsics"].numpy(), c["extrinsics"].numpy())
        assert abs(got - c["val"]) <= 1e-5 * max(1.0, abs(c["val"]))
    assert g2["mvcs"][-1]["val"] == 0.0 and R.mvcs(g2["mvcs"][-1]["depths"].numpy(), g2["mvcs"][-1]["intrinsics"].numpy(), g2["mvcs"][-1]["extrinsics"].numpy()) == 0.0
    for c in g2["pointcloud"]:
        conf = c["conf"].numpy().ravel()
        with np.errstate(invalid="ignore"):
            keep = R.conf_valid(conf) & (conf >= R.kth_threshold(conf, c["conf_thres"]))
        assert np.array_equal(c["points"].numpy().reshape(-1, 3)[keep], c["vertices"].numpy())
    for c in g2["pose_enc"]:
        ext, intr = R.pose_decode(c["pose_enc"].numpy(), c["image_size_hw"], f32)
        assert np.array_equal(ext.reshape(c["extrinsics"].shape), c["extrinsics"].numpy())
        assert np.allclose(intr.reshape(c["intrinsics"].shape), c["intrinsics"].numpy(), rtol=2e-6, atol=1e-4)
        ext64, intr64 = R.pose_decode(c["pose_enc"].numpy(), c["image_size_hw"])
        assert np.allclose(ext64.reshape(c["extrinsics"].shape), c["extrinsics"].numpy(), rtol=1e-6, atol=1e-6)
        assert np.allclose(intr64.reshape(c["intrinsics"].shape), c["intrinsics"].numpy(), rtol=2e-6, atol=1e-4)
    for c in g2["da3_unproject"]:
        for dt in (f64, f32):
            wp = R.unproject(c["depths"].numpy(), c["intrinsics"].numpy(), c["extrinsics"].numpy(), dt)
            assert np.allclose(wp, c["world_points"].numpy(), rtol=1e-5, atol=1e-6)
    for c in g2["lpips"]:                                                            # the input side of LPIPS: the oracle's own, pinned through the `lpips` goldens
        size = R.nchw(c["gt"], f32).shape[-2:]
        rep = osc.to_pm1(c["rep"]).numpy()
        assert np.array_equal(R.frames_pm1(c["gt"], dt=f32), osc.to_pm1(c["gt"]).numpy())
        assert np.array_equal(R.frames_pm1(c["rep"], size, f32), rep if rep.shape[-2:] == size else osc.bilinear_resize(rep, size))


def test_float32_restatements_equal_the_oracle_where_the_order_is_the_same():
    """the restatements the device is held to bit for bit are themselves the oracle's arithmetic"""
    for name, x, size in R.pm1_cases():
        a = osc.to_pm1(x).numpy()
        want = a if size is None or tuple(size) == a.shape[-2:] else osc.bilinear_resize(a, size)
        assert np.array_equal(R.frames_pm1(x, size, f32), want), name
    for n in (1, 64, 65, 130):
        pe = R.pose_family(n, n)
        ext, intr = R.pose_decode(pe, (294, 518), f32)
        o_ext, o_intr = osc.pose_encoding_to_extri_intri(pe, (294, 518))
        assert np.array_equal(ext, o_ext.numpy()), n                                # torch sums the four squares in the kernel's order
        assert np.allclose(intr, o_intr.numpy(), rtol=1e-6)
    K, E = R.eye_cams(1)
    for pc, colors, H, W in (R.splat_edge_family(8, 6) + (6, 8), R.splat_edge_family(7, 5) + (5, 7), R.splat_tie_family()):
        with np.errstate(invalid="ignore"):                                         # the z = +inf point: 0 * inf, on purpose
            assert np.array_equal(R.splat_restated(pc, colors, K[0], E[0], H, W), osc.project_points(pc, colors, K[0], E[0], H, W))
    pc, colors, K, E, H, W = R.splat_range_family()
    for t in range(3):
        assert np.array_equal(R.splat_restated(pc, colors, K[t], E[t], H, W), osc.project_points(pc, colors, K[t], E[t], H, W))


# ---------------------------------------------------------------------------------------------- builders meet their conditions
def test_confidence_builders_and_the_rank_that_float32_moves():
    for thres, n_valid in ((0.7, 1000), (5.1, 1000), (33.3, 1000), (40.1, 1000), (99.99, 9998), (99.99, 9999)):
        k64, k32 = R.kth_rank(n_valid, thres), R.kth_rank(n_valid, thres, "k_from_f32")
        print(f"conf_thres {thres} n_valid {n_valid}: k {k64} (double) vs {k32} (float32 threshold)")
        assert k64 != k32 and abs(k64 - k32) == 1
        conf = R.conf_distinct(n_valid, n_valid + 137, seed=n_valid)
        assert int(R.conf_valid(conf).sum()) == n_valid and len(np.unique(conf[R.conf_valid(conf)])) == n_valid
        assert R.kth_threshold(conf, thres) != R.kth_threshold(conf, thres, "k_from_f32")       # distinct values: the device test can see the rank
    for thres in (50, 100):
        assert R.kth_rank(1000, thres) == R.kth_rank(1000, thres, "k_from_f32")                   # float32 holds these thresholds
    for byte in range(4):
        bits = R.conf_byte_family(byte, 300, byte).view(np.uint32)
        assert R.conf_valid(bits.view(f32)).all()
        x = np.bitwise_or.reduce(bits ^ bits[0])
        assert x != 0 and (x & ~np.uint32(0xFF << (8 * byte))) == 0 and len(np.unique(bits)) > 40
    v = R.conf_tie(0)
    for thres in (33.3, 50, 65):
        k = R.kth_rank(1000, thres)
        s = np.sort(v)[::-1]
        assert s[k - 1] == f32(0.5) and s[k] == f32(0.5)                                         # the cut falls inside the tie
    m = R.conf_mixed()
    assert int(R.conf_valid(m).sum()) == 5 and not R.conf_valid(m[7:8])[0] and R.conf_valid(m[8:9])[0] and m[8] > m[7] == f32(1e-5)
    assert R.kth_threshold(np.array(R.INVALID, f32), 30.0) == -np.inf and not R.conf_valid(np.array(R.INVALID, f32)).any()


def test_frame_builders():
    for d, l, t in R.ARMS:
        for k in R.RANGES[d]:
            x = R.make_frames(3, 2, 3, 5, 7, d, l, t, k)
            a = x.numpy() if t else x
            assert torch.is_tensor(x) == t and a.dtype == (np.uint8 if d == "u8" else f32) and a.shape == ((2, 5, 7, 3) if l else (2, 3, 5, 7))
            if k == "bin":
                assert set(np.unique(a)) == {0, 1}                                   # max is not > 1: no division by 255
            elif k == "255":
                assert a.min() >= 0 and 1 < a.max() <= 255
            elif k == "01":
                assert a.min() == 0 and a.max() == 1.0 and np.signbit(a[a == 0]).any() and not (a < 0).any()      # the minimum is -0.0, which is not < 0
            else:
                assert a.min() == -1.0 and a.max() == 1.0
    sizes = {(tuple(R.nchw(g, f32).shape[-2:]), tuple(R.nchw(r, f32).shape[-2:])) for _, g, r, _ in R.frame_metric_cases()}
    assert {((5, 7), (1, 1)), ((5, 7), (1, 9)), ((11, 13), (3, 4)), ((5, 7), (37, 41)), ((5, 7), (5, 9)), ((5, 7), (4, 9)), ((300, 300), (300, 300))} <= sizes
    n, g, r, _ = R.frame_metric_cases()[-3]
    assert "overshooting" in n and g.min() < 0 and g.max() > 1 and r.min() < 0 and r.max() > 1


def test_splat_builders():
    for W, H in ((8, 6), (7, 5)):
        pc, colors = R.splat_edge_family(W, H)
        u, v, z = osc._project_uvz(pc, np.eye(3, dtype=f32), np.eye(4, dtype=f32))
        assert np.array_equal(u, np.rint(pc[:, 0])) and np.array_equal(v, np.rint(pc[:, 1])) and (z == 1).all()      # exact by construction
        assert np.signbit(u[u == 0]).any() and (u == W).any() == (W % 2 == 0) and (v == H).any() == (H % 2 == 0)      # -0.0 is kept; W - 0.5 rounds to even
        assert len({tuple(c) for c in colors}) == len(colors)
    pc, colors, K, E, H, W = R.splat_range_family()
    vis = [np.nonzero((lambda u, v, z: (u >= 0) & (u < W) & (v >= 0) & (v < H) & (z > 0))(*osc._project_uvz(pc, K[t], E[t])))[0] for t in range(3)]
    assert colors[vis[0]].max() == 1.0 and colors[vis[1]].max() == 200.0 and colors[vis[1]].min() <= 1.0 and len(vis[1]) >= 3 and len(vis[2]) == 0
    for (N, T, H, W, seed) in ((524_288 + 300, 2, 48, 64, 1), (6000, 1, 512, 520, 2)):
        pc, colors, K, E = R.splat_random(N, T, H, W, seed)
        assert R.splat_margin(pc, K, E, H, W).min() >= 1e-3
    pc, colors, K, E = R.splat_random(6000, 1, 512, 520, 2)
    canvas, _ = R.splat_ref(pc, colors, K, E, 512, 520)
    assert canvas.reshape(-1, 3)[1024 * 256:].any()                                  # pixels of the resolve loop's second pass are drawn
    pc, colors, K, E = R.splat_big()
    canvas, _ = R.splat_ref(pc, colors, K, E, 48, 64)
    only_head, _ = R.splat_ref(pc[:2048 * 256], colors[:2048 * 256], K, E, 48, 64)
    assert (canvas != only_head).any()                                               # points of the point loop's second pass win pixels


def test_mvcs_builders():
    for name, d, K, E in R.mvcs_cases():
        d64, d32 = [], []
        R.mvcs(d, K, E, f64, diag=d64)
        R.mvcs(d, K, E, f32, diag=d32)
        for a, b in zip(d64, d32):
            assert a["margin"] >= 1e-3, (name, a["margin"])                          # no pixel within 1e-3 px of a mask boundary
            assert int((a["mask"] != b["mask"]).sum()) == 0, name                    # at most 0 pixels left out of (or added to) a comparison
        assert K[0][0, 1] != 0 and abs(K[0][0, 2] - d.shape[2] / 2) > 0.5            # skew, off-centre principal point
        if name.startswith("T=") or name.startswith("affine"):
            assert all(a["n_edge"] > 0 and a["mask"].any() for a in d64), name       # some bilinear footprints leave the image: zero padding matters
        if name.startswith("skipped"):
            assert not d64[0]["mask"].any() and d64[1]["mask"].any()
        if name.startswith("affine"):
            A = E[1, :3, :3].astype(f64)
            assert 1e-3 < np.abs(A @ A.T - np.eye(3)).max() < 0.2
    d, K, E = R.mvcs_away_family(True)
    assert R.mvcs(d, K, E) == 0.0 and osc.mvcs(d, K, E) == 0.0
    d, K, E = R.mvcs_boundary_family()
    dg = []
    R.mvcs(d, K, E, f32, diag=dg)
    assert dg[0]["margin"] == 0.0 and int(dg[0]["mask"].sum()) == d.shape[1] * (d.shape[2] - 1)       # the last column sits exactly on u = W
    # the sizes meant to make a grid-stride loop go round twice do pass the grid caps of scorer.hip / scorer2.hip (blocks x 256 threads)
    assert 200 * 340 > 256 * 256 and 512 * 520 > 1024 * 256 and 3 * 300 * 300 > 1024 * 256 and 3 * 420 * 420 > 2048 * 256 and 3 * 424 * 416 > 2048 * 256


def test_epipolar_builders():
    pairs = R.epipolar_pairs()
    kinds = [p[0] for p in pairs]
    assert kinds[0] == "empty" and kinds[-1] == "empty" and kinds[-2] == "few" and "empty" in kinds[1:-2] and len(pairs[-2][1]) == 7
    assert sorted(len(p[1]) for p in pairs if p[0] == "F") == [8, 9, 255, 256, 257, 2048]
    for kind, p1, p2 in pairs:
        if kind == "F":
            ev = R.design_eigs(p1, p2)
            print(f"epipolar n={len(p1)}: smallest eigenvalues {ev[0]:.3e} {ev[1]:.3e}")
            assert ev[1] >= 1e3 * max(ev[0], 0.0) and ev[1] > 1e-6, (len(p1), ev[:3])
        if kind == "same":
            assert np.array_equal(p1, p2) and len(p1) == 300
        if kind == "line":
            d = p1 - p1[0]
            assert len(p1) == 20 and np.abs(d[:, 0] * d[-1, 1] - d[:, 1] * d[-1, 0]).max() < 1e-2


# ---------------------------------------------------------------------------------------------- the fp32 oracle uses at most half of every cap
def test_oracle_distance_is_at_most_half_of_every_cap():
    worst = {}

    def note(fam, cap, ref32, ref64):
        scale = R.SCALE[cap](ref64)
        d = abs(ref32 - ref64) / scale if scale > 0 else 0.0
        worst[fam] = max(worst.get(fam, 0.0), d)
        assert d <= 0.5 * R.CAP[cap], (fam, cap, ref32, ref64, d)

    for name, gt, rep, cap in R.frame_metric_cases():
        fam = "frame metric 64 arms" if " vs " in name and "300" not in name else "frame metric " + name
        note(fam + " mse", cap, osc.mse_any_size(gt, rep), R.frame_metric(gt, rep))
        note(fam + " psnr", "psnr", osc.psnr(gt, rep), R.frame_metric(gt, rep, psnr=True))
    for name, d, K, E in R.mvcs_cases() + [("boundary", *R.mvcs_boundary_family())]:
        note("mvcs " + name, "mvcs", osc.mvcs(d, K, E), R.mvcs(d, K, E))
    for name, E in R.motion_cases():
        note("motion " + name.split()[0], "motion", osc.motion_score(E), R.motion(E))
    for fam, d in worst.items():
        print(f"{fam}: oracle-to-fp64 distance {d:.3e}")
    for T, H, W in ((3, 9, 13), (1, 512, 520)):
        K, E = R.unproject_cams(T, H, W, T)
        depth = R.mvcs_depth(T, H, W, 3, noise=0.05)
        o = osc.unproject_depth(depth, K, osc.affine_inverse(E)).numpy()
        print(f"unproject {T}x{H}x{W}: oracle d32 {R.rel_err(o, R.unproject(depth, K, E)):.3e}, restatement {R.rel_err(R.unproject(depth, K, E, f32), R.unproject(depth, K, E)):.3e}")
    for n in (1, 64, 65, 130):
        pe = R.pose_family(n, n)
        print(f"pose decode n={n}: intr oracle d32 {R.rel_err(osc.pose_encoding_to_extri_intri(pe, (294, 518))[1].numpy(), R.pose_decode(pe, (294, 518))[1]):.3e}")
    for kind, p1, p2 in R.epipolar_pairs():                                      # the oracle of F and the Sampson error IS fp64: distance 0 by construction
        if kind == "same":
            assert abs(osc.epipolar_pair_error(p1, p2) - 1e-4) <= 1e-4 * 1e-4


# ---------------------------------------------------------------------------------------------- wrong restatements are rejected
def _first_rejected(cases):
    """cases: iterable of (name, thunk) where thunk() runs judge / judge_exact on a wrong restatement -> the names that were rejected"""
    hit = []
    for name, thunk in cases:
        try:
            thunk()
        except AssertionError:
            hit.append(name)
    return hit


def test_judge_rejects_wrong_restatements():
    with R.quiet():
        rejected = _rejected_restatements()
    assert set(R.WRONG) <= {k.split(" ")[0] for k in rejected}
    for k, v in rejected.items():
        print(f"rejected {k}: {len(v)} cases, e.g. {v[0]}")


def _rejected_restatements():
    rejected = {}
    fm = R.frame_metric_cases()
    resized = [c for c in fm if c[3] == "mse_resize"]
    # the correct fp32 restatement passes everywhere: the rejections below are the mistakes', not the restatement's
    for name, gt, rep, cap in fm:
        R.judge(name, R.frame_metric(gt, rep, dt=f32), R.frame_metric(gt, rep), osc.mse_any_size(gt, rep), cap)

    def metric_cases(wrong, pool):
        return [(n, (lambda g=g, r=r, c=c: R.judge(n, R.frame_metric(g, r, dt=f32, wrong=wrong), R.frame_metric(g, r), osc.mse_any_size(g, r), c))) for n, g, r, c in pool]

    rejected["align_corners"] = _first_rejected(metric_cases("align_corners", resized))
    rejected["rules_swapped"] = _first_rejected(metric_cases("rules_swapped", fm))
    rejected["max_first"] = _first_rejected(metric_cases("max_first", fm))
    rejected["hwc_as_chw"] = _first_rejected(metric_cases("hwc_as_chw", fm))
    assert len(rejected["align_corners"]) >= len(resized) // 2
    assert any("pm1" in n for n in rejected["rules_swapped"]) and len(rejected["hwc_as_chw"]) > 100
    assert not any(" vs " in n and "THWC" not in n for n in rejected["hwc_as_chw"])                 # a pair without a [T,H,W,C] side cannot tell
    assert len(rejected["max_first"]) == 2 and all("overshooting" in n for n in rejected["max_first"])       # shows only on a tensor with min < 0 AND max > 1
    # frames_to_pm1 is held to equality: every mistake that touches it shows
    pm = R.pm1_cases()
    for wrong in ("align_corners", "rules_swapped", "hwc_as_chw"):
        hit = _first_rejected([(n, (lambda x=x, s=s: R.judge_exact(n, R.frames_pm1(x, s, f32, wrong), R.frames_pm1(x, s, f32)))) for n, x, s in pm])
        assert hit, wrong
        rejected[wrong + " (pm1)"] = hit

    mv = R.mvcs_cases()[:4]
    ok = lambda w, d, K, E, n: R.judge(n, R.mvcs(d, K, E, f32, w), R.mvcs(d, K, E), osc.mvcs(d, K, E), "mvcs")
    for n, d, K, E in mv + [("boundary", *R.mvcs_boundary_family())]:
        ok(None, d, K, E, n)
    rejected["no_zero_pad"] = _first_rejected([(n, (lambda d=d, K=K, E=E, n=n: ok("no_zero_pad", d, K, E, n))) for n, d, K, E in mv])
    assert len(rejected["no_zero_pad"]) == len(mv)
    rejected["mask_u_le_W"] = _first_rejected([("boundary", lambda: ok("mask_u_le_W", *R.mvcs_boundary_family(), "boundary"))])
    assert rejected["mask_u_le_W"] == ["boundary"]

    conf = R.conf_distinct(1000, 1137, seed=1000)
    rejected["k_from_f32"] = _first_rejected([(f"conf_thres {t}", (lambda t=t: R.judge_exact(f"conf_thres {t}", np.array([R.kth_threshold(conf, t, "k_from_f32")]),
                                                                                              np.array([R.kth_threshold(conf, t)])))) for t in R.THRESHOLDS])
    assert rejected["k_from_f32"] == ["conf_thres 0.7", "conf_thres 5.1", "conf_thres 33.3", "conf_thres 40.1"]

    def splat_fams():
        K, E = R.eye_cams(1)
        yield "edges 8x6", R.splat_edge_family(8, 6) + (K, E, 6, 8)
        yield "edges 7x5", R.splat_edge_family(7, 5) + (K, E, 5, 7)
        pc, col, H, W = R.splat_tie_family()
        yield "ties", (pc, col, K, E, H, W)
        yield "ranges", R.splat_range_family()

    for wrong, must in (("tie_highest", {"edges 8x6", "edges 7x5", "ties"}), ("range_all_points", {"ranges"}), ("round_half_away", {"edges 8x6", "edges 7x5"})):
        hit = _first_rejected([(n, (lambda f=f: R.judge_exact(n, R.splat_ref(*f, wrong=wrong)[0], R.splat_ref(*f)[0]))) for n, f in splat_fams()])
        assert must <= set(hit), (wrong, hit)
        rejected[wrong] = hit
    return rejected
