"""Every dispatch arm, grid-stride loop and deciding edge of the geometry-scorer kernels (csrc/scorer.hip, csrc/scorer2.hip) against the references, builders and
judging rule of tests/scorer_ref.py (tests/test_scorer_ref_host.py shows on the CPU that the rule rejects wrong kernels).  -m gpu only.

  exact       confidence cut, splat (canvas and float frames), `ext` of the pose decode, frames_to_pm1, the unprojection against its float32 restatement, and the
              (k_dim, e_rows) variants against each other
  per-element unprojected points and `intr` against fp64: max-abs error over max-abs at most 8 x d32 (d32: the fp32 oracle's same distance)
  scalar      MSE 2e-6 / resized 5e-6 / PSNR 2e-5 / MVCS 1e-5 / motion 2e-6 / Sampson 1e-4 / F rtol 2e-3 against fp64: the caps of tests/test_gpu_scorer.py

Every judged case prints `name err d32 ratio` before it asserts (`-s`).

Observed on an MI355X (also in DESIGN.md, section 5l).  Bit-equal: confidence cut, splat, `ext`, frames_to_pm1 (62 of 62 cases), the unprojection against its float32
restatement, the four MVCS layouts.  err / d32: unprojected points 0.88 (3 x 9 x 13), 1.00 (512 x 520); intr 1.00, 1.00, 0.57, 0.94 at n = 1, 64, 65, 130.  Scalars, largest
error as a fraction of the cap: MSE 0.038, resized MSE 0.012, PSNR 0.023, MVCS 0.015, motion 0.10 (the 1e-4 rad family), Sampson below 0.001, F 0.000.

Before `vgpa_conf_threshold` took its threshold as a double, test_conf_threshold_rank_from_the_double_threshold failed at (0.7 | 5.1 | 33.3 | 40.1, 1000) and (99.99, 9998 | 9999),
and with it the N = 1000 row of the small-N test and the get_colored_pointcloud / reproject_predictions test: the rank was one off (33.3 at 1000: 668 for 667)."""
import numpy as np
import pytest
import torch

import scorer_ref as R
from oracle import scorer as osc

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def sc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import scorer
    return scorer


# ---------------------------------------------------------------------------------------------- confidence cut
def _cut(sc, conf, thres):
    return sc.confidence_threshold(torch.from_numpy(np.asarray(conf, f32)), thres).cpu().numpy()


def _check_cut(sc, name, conf, thres):
    R.judge_exact(f"{name} conf_thres {thres}", _cut(sc, conf, thres), np.array([R.kth_threshold(conf, thres)], f32))


def test_conf_threshold_small_n_every_threshold(sc):
    for N in R.SMALL_N:
        conf = R.conf_distinct(N, N, seed=N)
        for thres in R.THRESHOLDS:
            _check_cut(sc, f"N={N}", conf, thres)


@pytest.mark.parametrize("thres,n_valid", [(0.7, 1000), (5.1, 1000), (33.3, 1000), (40.1, 1000), (50, 1000), (100, 1000), (99.99, 1000), (99.99, 9998), (99.99, 9999)])
def test_conf_threshold_rank_from_the_double_threshold(sc, thres, n_valid):
    """n_valid = 1000 (9998 / 9999 for 99.99) among invalid values: a threshold rounded to float32 moves k by one here (the host test asserts that it does), and the
    valid values are distinct, so the returned value shows the rank"""
    conf = R.conf_distinct(n_valid, n_valid + 137, seed=n_valid)
    _check_cut(sc, f"n_valid={n_valid}", conf, thres)


def test_conf_threshold_values_edges(sc):
    for n in (1, 300, 1000):
        for thres in (0.7, 33.3, 50, 100):
            _check_cut(sc, f"all equal n={n}", np.full(n, 0.37, f32), thres)
    for byte in range(4):                                       # the values differ in one byte only: that radix pass alone decides
        conf = R.conf_byte_family(byte, 300, byte)
        for thres in (0.7, 33.3, 50, 99.99, 100):
            _check_cut(sc, f"byte {byte}", conf, thres)
    for thres in (25, 33.3, 50, 65, 75):                        # 30 % .. 70 %: the cut falls inside 400 equal values; 25 / 75: just outside
        _check_cut(sc, "tie", R.conf_tie(0), thres)
    m = R.conf_mixed()
    for thres in (0.7, 20, 33.3, 50, 80, 100):                  # 5 values count: NaN, +-inf, 0, -0, negatives and the float32 1e-5 itself do not, the next float does
        _check_cut(sc, "mixed", m, thres)
    assert _cut(sc, m, 100)[0] == f32(5.0) and _cut(sc, m, 0.7)[0] == np.nextafter(f32(1e-5), f32(1))
    bad = np.array(R.INVALID, f32)
    for thres in (0, -3, 30.0, 100):
        assert _cut(sc, bad, thres)[0] == -np.inf               # nothing valid
    assert _cut(sc, R.conf_distinct(10, 10, 0), 0)[0] == -np.inf and _cut(sc, R.conf_distinct(10, 10, 0), -1.5)[0] == -np.inf


def test_conf_threshold_through_pointcloud_and_reprojection(sc):
    """conf_thres 33.3 with exactly 1000 valid confidences (k = 667; 668 from a float32 threshold): the kept set of get_colored_pointcloud and the frames of
    reproject_predictions equal oracle.scorer.pointcloud_filter + batch_reproject bit for bit"""
    T, h, w = 2, 20, 30
    rng = np.random.default_rng(8)
    conf = R.conf_distinct(1000, T * h * w, seed=3).reshape(T, h, w)
    pts = (rng.normal(size=(T, h, w, 3)) * [1.0, 0.8, 0.3] + [0, 0, 3.0]).astype(f32)
    imgs = rng.random((T, 3, h, w)).astype(f32)
    K = np.stack([np.array([[28.0, 0, w / 2], [0, 28.0, h / 2], [0, 0, 1]], f32)] * T)
    E = np.stack([np.eye(4, dtype=f32)] * T)
    E[1, 0, 3] = 0.2
    for thres in (33.3, 40.1, 50):
        v, c = sc.get_colored_pointcloud({"images": torch.from_numpy(imgs), "world_points": torch.from_numpy(pts), "world_points_conf": torch.from_numpy(conf)},
                                         conf_thres=thres)
        rv, rc = osc.pointcloud_filter(pts, conf, imgs, thres)
        assert len(rv) == R.kth_rank(1000, thres)
        R.judge_exact(f"kept vertices {thres}", v, rv)
        R.judge_exact(f"kept colours {thres}", c, rc)
        out = sc.reproject_predictions(torch.from_numpy(pts), torch.from_numpy(conf), torch.from_numpy(imgs), K, E, h, w, conf_thres=thres)
        R.judge_exact(f"reprojected frames {thres}", out, osc.batch_reproject(rv.numpy(), rc.numpy(), K, E, h, w))


# ---------------------------------------------------------------------------------------------- splat
def _check_splat(sc, name, pc, colors, K, E, H, W, conf=None, thr=-np.inf, thr_dev=False):
    want_c, want_f = R.splat_ref(pc, colors, K, E, H, W, conf, thr)
    kw = {} if conf is None else {"conf": conf, "conf_thr": torch.tensor([thr], dtype=torch.float32, device="cuda") if thr_dev else float(thr)}
    canvas, out_f = sc.project_views(pc, colors, K, E, H, W, **kw)
    R.judge_exact(name + " canvas", canvas, want_c)
    R.judge_exact(name + " frames", out_f, want_f)
    only_c = sc.project_views(pc, colors, K, E, H, W, want_float=False, **kw)
    only_f = sc.project_views(pc, colors, K, E, H, W, want_canvas=False, **kw)
    assert only_c[1] is None and only_f[0] is None and torch.equal(only_c[0], canvas) and torch.equal(only_f[1], out_f)      # either output alone


@pytest.mark.parametrize("e_rows", [3, 4])
def test_splat_pixel_centres_ties_and_depth_edges(sc, e_rows):
    K, E = R.eye_cams(1, e_rows)
    for W, H in ((8, 6), (7, 5)):
        _check_splat(sc, f"edges {W}x{H}", *R.splat_edge_family(W, H), K, E, H, W)
    pc, colors, H, W = R.splat_tie_family()
    _check_splat(sc, "ties", pc, colors, K, E, H, W)
    canvas = sc.project_views(pc, colors, K, E, H, W)[0].cpu().numpy()[0]
    clip = lambda i: np.clip(colors[i], 0, 255).astype(np.uint8)
    assert (canvas[1, 1] == clip(0)).all() and (canvas[1, 2] == clip(2)).all() and (canvas[1, 3] == clip(6)).all() and (canvas[1, 4] == clip(7)).all()
    assert (canvas[3, 1] == clip(13)).all() and not canvas[1, 5:].any()                     # z = 0, z < 0, z = +inf draw nothing


def test_splat_colour_range_per_frame_clamp_and_empty(sc):
    pc, colors, K, E, H, W = R.splat_range_family()
    _check_splat(sc, "ranges", pc, colors, K, E, H, W)
    canvas, out_f = sc.project_views(pc, colors, K, E, H, W)
    assert canvas[0].max().item() == 255 and canvas[1].max().item() == 200 and canvas[2].max().item() == 0 and out_f[2].max().item() == -1.0
    pc, big, unit, H, W = R.splat_clamp_family()
    K1, E1 = R.eye_cams(1)
    _check_splat(sc, "clamp [0,255]", pc[:5], big, K1, E1, H, W)
    _check_splat(sc, "clamp [0,1]", pc[5:], unit, K1, E1, H, W)
    _check_splat(sc, "N = 0", np.zeros((0, 3), f32), np.zeros((0, 3), f32), K, E, H, W)


def test_splat_confidence_predicate_by_value_and_from_device(sc):
    pc, colors, K, E = R.splat_random(3000, 2, 24, 31, seed=5)
    conf = R.conf_distinct(2500, 3000, seed=6)
    for thr in (-np.inf, float(R.kth_threshold(conf, 33.3)), 1e9):
        for thr_dev in (False, True):
            _check_splat(sc, f"conf thr {thr:.4g} dev={thr_dev}", pc, colors, K, E, 24, 31, conf, thr, thr_dev)


def test_splat_second_pass_of_the_point_loop_and_of_the_resolve_loop(sc):
    pc, colors, K, E = R.splat_big()                                   # 2048 x 256 + 300 points, T = 2, 64 x 48
    _check_splat(sc, "N = 524288 + 300", pc, colors, K, E, 48, 64)
    pc, colors, K, E = R.splat_random(6000, 1, 512, 520, 2)            # 512 x 520 > 1024 x 256 pixels
    _check_splat(sc, "512 x 520", pc, colors, K, E, 512, 520)


# ---------------------------------------------------------------------------------------------- frame metric, frames_to_pm1
@pytest.fixture(scope="module")
def frame_cases():
    """the cases with both references, computed once"""
    with R.quiet():
        return [(n, g, r, cap, R.frame_metric(g, r), osc.mse_any_size(g, r), R.frame_metric(g, r, psnr=True), osc.psnr(g, r)) for n, g, r, cap in R.frame_metric_cases()]


def test_frame_metric_every_arm_range_and_resize(sc, frame_cases):
    ms, ps = sc.MSEMetric(), sc.PSNRMetric()
    worst, failed = {}, []
    with R.quiet():
        for n, g, r, cap, m64, m32, p64, p32 in frame_cases:
            for key, got, r64, r32 in ((cap, ms.compute(gt=g, rep=r), m64, m32), ("psnr", ps.compute(gt=g, rep=r), p64, p32)):
                try:
                    err, _ = R.judge(f"{n} {key}", got, r64, r32, key)
                    worst[key] = max(worst.get(key, 0.0), err / R.CAP[key])
                except AssertionError as e:
                    failed.append(str(e))
    print(f"{len(frame_cases)} cases; largest err over cap: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not failed, (len(failed), failed[:5])


def test_frame_metric_identical_inputs_give_psnr_100(sc):
    ps, ms = sc.PSNRMetric(), sc.MSEMetric()
    for d, l, t in R.ARMS:
        for k in R.RANGES[d]:
            x = R.make_frames(9, 2, 3, 5, 7, d, l, t, k)
            assert ps.compute(gt=x, rep=x) == 100.0 and ms.compute(gt=x, rep=x) == 0.0, (d, l, t, k)
    u8 = R.make_frames(10, 2, 3, 5, 7, "u8", 1, False, "255")
    as_float = torch.from_numpy(u8.astype(f32)).permute(0, 3, 1, 2).contiguous()            # the same whole numbers as a float tensor [T,C,H,W]: x / 255 on both sides
    assert ps.compute(gt=u8, rep=as_float) == 100.0 and ps.compute(gt=as_float, rep=u8) == 100.0


def test_frames_to_pm1_equals_the_float32_restatement(sc):
    bad = []
    cases = R.pm1_cases()
    with R.quiet():
        for n, x, size in cases:
            try:
                R.judge_exact(n, sc.frames_to_pm1(x, size), R.frames_pm1(x, size, f32))
            except AssertionError as e:
                bad.append(str(e))
    print(f"frames_to_pm1: {len(cases) - len(bad)} of {len(cases)} cases bit-equal")
    assert not bad, (len(bad), bad[:5])


# ---------------------------------------------------------------------------------------------- MVCS
def _mvcs(sc, d, K, E):
    return sc.MVCSMetric().compute(depths=d, intrinsics=K, extrinsics=E)


@pytest.fixture(scope="module")
def mvcs_cases():
    return [(n, d, K, E, R.mvcs(d, K, E), osc.mvcs(d, K, E)) for n, d, K, E in R.mvcs_cases() + [("boundary u = W", *R.mvcs_boundary_family())]]


def test_mvcs_against_fp64_and_the_four_layouts_agree(sc, mvcs_cases):
    for n, d, K, E, r64, r32 in mvcs_cases:
        got = {(kd, er): _mvcs(sc, d, R.pad_K4(K) if kd == 4 else K, E[:, :er]) for kd in (3, 4) for er in (3, 4)}
        R.judge("mvcs " + n, got[(3, 4)], r64, r32, "mvcs")
        assert len({np.float32(v).tobytes() for v in got.values()}) == 1, (n, got)           # k_dim 3 / 4 and e_rows 3 / 4 read the same numbers
    d, K, E = mvcs_cases[1][1:4]
    assert _mvcs(sc, d[:, None], K, E) == _mvcs(sc, d[..., None], K, E) == _mvcs(sc, d, K, E)          # [T,1,H,W] and [T,H,W,1]


def test_mvcs_nothing_to_compare(sc):
    d, K, E = R.mvcs_away_family(True)
    assert _mvcs(sc, d, K, E) == 0.0                            # the only pair has no valid pixel
    assert _mvcs(sc, d[:1], K[:1], E[:1]) == 0.0                # T = 1: no pair
    for shape in ((2, 1, 9), (2, 9, 1)):                        # H or W of 1: the grid normalisation would divide by zero
        with pytest.raises(RuntimeError, match="invalid argument"):
            _mvcs(sc, np.ones(shape, f32), K, E)


# ---------------------------------------------------------------------------------------------- unprojection, pose decode
@pytest.mark.parametrize("T,H,W", [(3, 9, 13), (1, 512, 520)])
def test_unprojection(sc, T, H, W):
    K, E = R.unproject_cams(T, H, W, T)
    depth = R.mvcs_depth(T, H, W, 3, noise=0.05)
    got4 = sc.unproject_depth_to_world(depth, K, E)
    got3 = sc.unproject_depth_to_world(depth, K, E[:, :3])
    assert torch.equal(got3, got4)
    R.judge_exact(f"unproject {T}x{H}x{W} vs float32 restatement", got4, R.unproject(depth, K, E, f32))
    R.judge(f"unproject {T}x{H}x{W}", got4, R.unproject(depth, K, E), osc.unproject_depth(depth, K, osc.affine_inverse(E)).numpy())


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_pose_decode(sc, n):
    pe = R.pose_family(n, n)
    ext, intr = sc.pose_encoding_to_extri_intri(torch.from_numpy(pe), (294, 518))
    o_ext, o_intr = osc.pose_encoding_to_extri_intri(pe, (294, 518))
    R.judge_exact(f"pose decode n={n} ext", ext, o_ext)
    r_ext64, r_intr64 = R.pose_decode(pe, (294, 518))
    R.judge(f"pose decode n={n} intr", intr, r_intr64, o_intr.numpy())
    zero = np.ones((3, 3), bool)
    zero[[0, 1, 0, 1, 2], [0, 1, 2, 2, 2]] = False
    assert not intr.cpu().numpy()[:, zero].any() and (intr[:, 0, 2] == 259.0).all() and (intr[:, 1, 2] == 147.0).all() and (intr[:, 2, 2] == 1.0).all()
    ext2, none = sc.pose_encoding_to_extri_intri(torch.from_numpy(pe), build_intrinsics=False)          # intr NULL
    assert none is None and torch.equal(ext2, ext)


# ---------------------------------------------------------------------------------------------- motion score
@pytest.fixture(scope="module")
def motion_cases():
    return [(n, E, R.motion(E), osc.motion_score(E)) for n, E in R.motion_cases()]


def test_motion_score(sc, motion_cases):
    for n, E, r64, r32 in motion_cases:
        got4 = float(sc.compute_motion_score_vectorized(E))
        got3 = float(sc.compute_motion_score_vectorized(E[:, :3]))
        assert got3 == got4, n
        R.judge("motion " + n, got4, r64, r32, "motion")
        if len(E) == 1:
            assert got4 == 0.0
    still = R.motion_family("still", 66)
    t = still[:, :3, 3].astype(f64)
    assert abs(float(sc.compute_motion_score_vectorized(still)) - np.linalg.norm(t[1:] - t[:-1], axis=1).mean()) <= 2e-6 * 3      # the angle term is exactly 0
    half = R.motion_family("half_turn", 3)
    t = half[:, :3, 3].astype(f64)
    assert abs(float(sc.compute_motion_score_vectorized(half)) - (np.linalg.norm(t[1:] - t[:-1], axis=1).mean() + 0.1 * np.pi)) <= 2e-6


# ---------------------------------------------------------------------------------------------- epipolar
def test_epipolar_every_pair_size_in_one_call(sc):
    pairs = R.epipolar_pairs()
    err, Fm = sc.epipolar_errors([p[1] for p in pairs], [p[2] for p in pairs], return_F=True)
    err, Fm = err.cpu().numpy(), Fm.cpu().numpy()
    for i, (kind, p1, p2) in enumerate(pairs):
        if kind in ("empty", "few"):
            assert err[i] == -1.0 and not Fm[i].any(), (i, kind, err[i])
        elif kind == "F":
            ref = osc.epipolar_pair_error(p1, p2)
            R.judge(f"sampson pair {i} n={len(p1)}", err[i], ref, ref, "sampson")
            Fr = osc.find_fundamental(p1, p2)
            print(f"F pair {i} n={len(p1)}: largest |dF| / (1e-6 + 2e-3 |F|) {np.max(np.abs(Fm[i] - Fr) / (1e-6 + 2e-3 * np.abs(Fr))):.3f}")
            assert np.allclose(Fm[i], Fr, rtol=R.CAP["F"], atol=1e-6), (i, Fm[i], Fr)
        elif kind == "same":
            print(f"p1 == p2: err {err[i]!r}")
            assert np.isfinite(err[i]) and abs(float(err[i]) - 1e-4) <= 2 * 2.0 ** -24 * 1e-4, err[i]            # sqrt(0 + 1e-8) to fp32 rounding
        else:
            assert np.isfinite(err[i]) and np.isfinite(Fm[i]).all(), (i, kind)
