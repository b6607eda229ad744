"""fp64 / exact references, float32 restatements, seeded input builders and the judging rule of the geometry-scorer kernels (csrc/scorer.hip, csrc/scorer2.hip).
tests/test_scorer_ref_host.py checks on the CPU that the references reproduce the reference project's stored results (tests/golden/scorer.pt, scorer2.pt), that
every builder meets its conditions and that `judge` rejects wrong restatements; tests/test_gpu_scorer_kernels.py holds the device to the same rule.  CPU only: no
device code in here.  No number below was fitted to a device result.

Three kinds of answer.
  exact      the confidence cut (k-th largest valid confidence by sorting, k formed in Python double exactly as utils/pointcloud_utils.py:60-61 forms it), the
             z-buffer splat (oracle.scorer.project_points: lowest index wins a z tie), `ext` of the pose decode, frames_to_pm1 and the unprojection against
             float32 restatements in the kernel's order of operations: only +, -, *, correctly rounded / and comparisons, contraction off.
  per-element  outputs behind a 3 x 3 inverse or tanf (unprojected points, `intr`): max-abs error over max-abs of the fp64 answer at most MARGIN x d32, d32 the same
             distance of the fp32 oracle (oracle/scorer.py) on the same inputs.  MARGIN = 8 as tests/test_gpu_vggt_heads.py: same class of arithmetic, another
             order or another inverse.
  scalar     MSE, PSNR, MVCS, motion, Sampson error, F: relative caps CAP (the ones tests/test_gpu_scorer.py already uses), against the fp64 reference; the host
             test shows the fp32 oracle within half of each cap.

Every fp routine takes the working dtype `dt` (np.float64: the reference; np.float32: the restatement) and `wrong=`, which switches in ONE deliberate mistake
(WRONG lists them); the host test shows that the family meant to catch each mistake does."""
import contextlib

import numpy as np
import torch

from oracle import scorer as osc

f32, f64 = np.float32, np.float64
MARGIN = 8.0
CAP = {"mse": 2e-6, "mse_resize": 5e-6, "psnr": 2e-5, "mvcs": 1e-5, "motion": 2e-6, "sampson": 1e-4, "F": 2e-3}
# what the relative cap multiplies (the expressions of tests/test_gpu_scorer.py)
SCALE = {"mse": lambda r: abs(r), "mse_resize": lambda r: max(1.0, abs(r)), "psnr": lambda r: max(1.0, abs(r)), "mvcs": lambda r: max(1.0, abs(r)),
         "motion": lambda r: max(1.0, abs(r)), "sampson": lambda r: max(r, 1e-3)}
WRONG = ("align_corners", "rules_swapped", "max_first", "hwc_as_chw", "mask_u_le_W", "no_zero_pad", "k_from_f32", "tie_highest", "range_all_points",
         "round_half_away")


# ---------------------------------------------------------------------------------------------- judging
_say = print


@contextlib.contextmanager
def quiet():
    """no `name err d32 ratio` lines inside: for loops over hundreds of cases whose summary is printed instead"""
    global _say
    old, _say = _say, (lambda *a, **k: None)
    try:
        yield
    finally:
        _say = old


def rel_err(got, want64):
    """max-abs error over max-abs of the float64 answer (tests/vggt_heads_ref.py::rel_err)"""
    got, want64 = np.asarray(got, f64), np.asarray(want64, f64)
    return float(np.abs(got - want64).max() / np.abs(want64).max())


def judge(name, got, ref64, ref32, cap=None):
    """Prints `name err d32 ratio`, then asserts.  cap None: per-element rule err <= MARGIN x d32.  cap a key of CAP: scalar rule |got - ref64| <= CAP x SCALE(ref64)
    (ratio is then err over the cap's half, which is what d32 may use).  -> (err, d32)"""
    if cap is None:
        got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
        err, d32 = rel_err(got, ref64), rel_err(ref32, ref64)
        ratio = err / d32 if d32 > 0 else (0.0 if err == 0 else float("inf"))
        _say(f"{name}: err {err:.3e} d32 {d32:.3e} ratio {ratio:.2f}")
        assert np.isfinite(err) and err <= MARGIN * d32, (name, err, d32)
        return err, d32
    got, ref64, ref32 = float(got), float(ref64), float(ref32)
    scale = SCALE[cap](ref64)
    err = abs(got - ref64) / scale if scale > 0 else (0.0 if got == ref64 else float("inf"))
    d32 = abs(ref32 - ref64) / scale if scale > 0 else (0.0 if ref32 == ref64 else float("inf"))
    _say(f"{name}: err {err:.3e} d32 {d32:.3e} ratio {err / CAP[cap]:.3f} of cap {CAP[cap]:.0e}")
    assert np.isfinite(got) and err <= CAP[cap], (name, got, ref64, err, CAP[cap])
    return err, d32


def judge_exact(name, got, ref):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ref = ref.detach().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, ref.shape, got.dtype, ref.dtype)
    same = (got == ref) | ((got != got) & (ref != ref))
    if got.dtype.kind == "f":                                   # bit for bit: -0.0 is not 0.0
        same &= np.signbit(got) == np.signbit(ref)
    bad = int((~same).sum())
    _say(f"{name}: {bad} of {got.size} differ")
    assert bad == 0, (name, bad, np.argwhere(~same)[:4].tolist())


# ---------------------------------------------------------------------------------------------- confidence cut
def conf_valid(conf):
    v = np.asarray(conf, f32).ravel()
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (v > f32(1e-5))


def kth_rank(n_valid, conf_thres, wrong=None):
    """k = max(1, int(ceil(n * keep))), keep = clamp(1 - conf_thres / 100) in Python double (utils/pointcloud_utils.py:60-61); wrong: from the float32 threshold"""
    t = float(f32(conf_thres)) if wrong == "k_from_f32" else float(conf_thres)
    keep = max(0.0, min(1.0, 1.0 - t / 100.0))
    return max(1, int(np.ceil(n_valid * keep)))


def kth_threshold(conf, conf_thres, wrong=None):
    """-> float32: the k-th largest valid confidence; -inf for conf_thres <= 0 or nothing valid"""
    v = np.asarray(conf, f32).ravel()
    v = v[conf_valid(v)]
    if conf_thres <= 0 or v.size == 0:
        return f32(-np.inf)
    return np.sort(v)[::-1][kth_rank(v.size, conf_thres, wrong) - 1]


THRESHOLDS = (0.7, 5.1, 33.3, 40.1, 50, 99.99, 100)
SMALL_N = (1, 2, 255, 256, 257, 1000)
INVALID = (np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, -3.5e-3, 1e-5, 9e-6, 1e-30)     # 1e-5 rounds to the float32 the predicate compares with: not above it


def conf_distinct(n_valid, n_total, seed):
    """n_total confidences of which exactly n_valid count, all valid ones distinct, in a seeded order"""
    rng = np.random.default_rng(seed)
    v = (np.arange(1, n_valid + 1, dtype=f64) * 0.013 + 0.002).astype(f32)
    bad = np.resize(np.array(INVALID, f32), n_total - n_valid)
    out = np.concatenate([v, bad])
    rng.shuffle(out)
    return out


def conf_byte_family(byte, n, seed):
    """valid confidences whose bit patterns differ in ONE byte only (3 = the top one): that radix pass alone finds the answer"""
    rng = np.random.default_rng(seed)
    if byte == 3:
        b = rng.integers(0x38, 0x7F, size=n, dtype=np.uint32)          # 0x38123456 = 3.5e-5 (valid) .. 0x7E123456 (finite)
        bits = (b << np.uint32(24)) | np.uint32(0x00123456)
    else:
        b = rng.integers(0, 256, size=n, dtype=np.uint32)
        bits = (np.uint32(0x3F123456) & ~np.uint32(0xFF << (8 * byte))) | (b << np.uint32(8 * byte))
    return bits.astype(np.uint32).view(f32)


def conf_tie(seed):
    """1000 valid: 300 distinct above 0.5, 400 equal to 0.5, 300 below: every cut from 30 % to 70 % lands inside the tie"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([0.6 + 0.001 * np.arange(300), np.full(400, 0.5), 0.1 + 0.001 * np.arange(300)]).astype(f32)
    rng.shuffle(v)
    return v


def conf_mixed():
    """every kind of value that does not count, the float32 1e-5 itself, the next float above it (counts), and a few that count"""
    e = f32(1e-5)
    return np.array([np.nan, 0.7, np.inf, -np.inf, 0.0, -0.0, -2.0, e, np.nextafter(e, f32(1)), 0.3, -1e-3, 0.3, 5.0, np.nan, 1e-6], f32)


# ---------------------------------------------------------------------------------------------- splat
def splat_restated(pc, colors, K, E, H, W, wrong=None):
    """oracle.scorer.project_points restated (equal to it bit for bit with wrong=None: shown in the host test) with the mistakes switched in"""
    pc, colors, K, E = np.asarray(pc, f32).reshape(-1, 3), np.asarray(colors, f32).reshape(-1, 3), np.asarray(K, f32), np.asarray(E, f32)
    canvas = np.zeros((H, W, 3), np.uint8)
    if len(pc) == 0:
        return canvas
    R, t = E[:3, :3], E[:3, 3]
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    with np.errstate(all="ignore"):
        cam = [((x * R[j, 0] + y * R[j, 1]) + z * R[j, 2]) + t[j] for j in range(3)]
        pr = [((cam[0] * K[i, 0] + cam[1] * K[i, 1]) + cam[2] * K[i, 2]) for i in range(3)]
        zz = pr[2]
        den = zz + f32(1e-8)
        qu, qv = pr[0] / den, pr[1] / den
        if wrong == "round_half_away":
            u, v = np.sign(qu) * np.floor(np.abs(qu) + f32(0.5)), np.sign(qv) * np.floor(np.abs(qv) + f32(0.5))
        else:
            u, v = np.rint(qu), np.rint(qv)
        valid = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (zz > 0) & np.isfinite(u) & np.isfinite(v)
    idx = np.nonzero(valid)[0]
    if idx.size == 0:
        return canvas
    unit = (colors.max() if wrong == "range_all_points" else colors[idx].max()) <= 1.0
    c = colors[idx]
    c = np.clip(c * f32(255), 0, 255).astype(np.uint8) if unit else np.clip(c, 0, 255).astype(np.uint8)
    pix = v[idx].astype(np.int64) * W + u[idx].astype(np.int64)
    order = np.lexsort((-idx if wrong == "tie_highest" else idx, zz[idx], pix))
    ps = pix[order]
    first = np.ones(ps.shape, bool)
    first[1:] = ps[1:] != ps[:-1]
    win = order[first]
    canvas.reshape(-1, 3)[pix[win]] = c[win]
    return canvas


def splat_ref(pc, colors, K, E, H, W, conf=None, thr=-np.inf, wrong=None):
    """-> (canvas u8 [T,H,W,3], frames f32 [T,3,H,W]) of the oracle; conf / thr: the predicate of the splat kernel (valid and >= thr)"""
    pc, colors = np.asarray(pc, f32).reshape(-1, 3), np.asarray(colors, f32).reshape(-1, 3)
    if conf is not None:
        c = np.asarray(conf, f32).ravel()
        with np.errstate(invalid="ignore"):
            keep = conf_valid(c) & (c >= f32(thr))
        pc, colors = pc[keep], colors[keep]
    one = (lambda k, e: osc.project_points(pc, colors, k, e, H, W)) if wrong is None else (lambda k, e: splat_restated(pc, colors, k, e, H, W, wrong))
    with np.errstate(all="ignore"):                                  # z = +inf: 0 * inf in the camera transform, on purpose
        canvas = np.stack([one(K[t], E[t]) for t in range(len(E))])
    frames = (canvas.transpose(0, 3, 1, 2).astype(f32) / f32(255.0)) * f32(2.0) - f32(1.0)
    return canvas, frames


def eye_cams(T, e_rows=4):
    return np.stack([np.eye(3, dtype=f32)] * T), np.stack([np.eye(4, dtype=f32)[:e_rows]] * T)


def splat_edge_family(W, H):
    """identity camera, z = 1: den = 1 + 1e-8 rounds to 1, so u = x and v = y exactly.  Every x of the list against every y: pixel centres (-0.5 -> -0.0, kept;
    0.5 -> 0; 1.5 and 2.5 -> 2; W - 0.5 -> W or W - 1 by the parity of W), all at one z: ties, lowest index wins.  Colours are distinct per point."""
    xs = [-0.5, 0.5, 1.5, 2.5, W - 1.5, W - 0.5]
    ys = [-0.5, 0.5, 1.5, 2.5, H - 1.5, H - 0.5]
    pc = np.array([[x, y, 1.0] for y in ys for x in xs], f32)
    colors = np.stack([10 + 6 * np.arange(len(pc)), 250 - 5 * np.arange(len(pc)), 3 + np.arange(len(pc))], 1).astype(f32)
    return pc, colors


def splat_tie_family():
    """8 x 6 canvas, identity camera: 2 and 3 points on one pixel at equal z in both index orders (colour order swapped on the second pixel), adjacent floats in z,
    and z = 0, z < 0, z = +inf (0 * inf = NaN in the camera transform), which must not draw"""
    z1 = f32(1.0)
    zn = np.nextafter(z1, f32(2))
    pc = np.array([[1, 1, 1], [1, 1, 1],                 # pixel (1,1): index 0 wins
                   [2, 1, 1], [2, 1, 1], [2, 1, 1],      # pixel (2,1): index 2 wins
                   [3, 1, zn], [3, 1, z1],               # pixel (3,1): the nearer, LATER point wins
                   [4, 1, z1], [4, 1, zn],               # pixel (4,1): the nearer, earlier point wins
                   [5, 1, 0], [6, 1, -1], [7, 1, np.inf],
                   [1, 3, 2], [1, 3, 1], [1, 3, 1]], f32)   # pixel (1,3): the two nearer ones tie, index 13 wins
    pc[:, :2] *= pc[:, 2:3].clip(1, 2)                   # u = x / z stays the integer meant above for z in {1, nextafter(1), 2}
    colors = np.stack([20 + 15 * np.arange(len(pc)), 240 - 15 * np.arange(len(pc)), 7 * np.arange(len(pc))], 1).astype(f32)
    return pc, colors, 6, 8


def splat_range_family():
    """T = 3, 6 x 5.  Frame 0 sees only colours <= 1.0 (one exactly 1.0): scaled by 255.  Frame 1 (x - 36) sees [0,1] colours and ALSO the point of colour 200
    that lies at x = 40, outside frame 0: nothing is scaled there, the [0,1] colours truncate to 0 or 1.  Frame 2 (z - 5 < 0) sees nothing: black."""
    pc = np.array([[1, 1, 1], [2, 1, 1], [3, 2, 1], [40, 3, 1], [0, 0, 1], [37, 0, 1], [38, 1, 1]], f32)
    colors = np.array([[1.0, 0.5, 0.25], [0.1, 0.9, 0.999], [0.0, 0.3, 0.7], [200.0, 100.5, 0.5], [0.6, 1.0, 0.2], [1.0, 0.999, 0.4], [0.5, 1.0, 0.0]], f32)
    K, E = eye_cams(3)
    E[1, 0, 3] = -36.0
    E[2, 2, 3] = -5.0
    return pc, colors, K, E, 5, 6


def splat_clamp_family():
    """colours below 0 and above 255, fractional ones (truncation), on separate pixels; one frame in [0,255] and one in [0,1] with negatives"""
    pc = np.array([[x, y, 1.0] for y in range(2) for x in range(5)], f32)
    big = np.array([[-3.5, 255.9, 300.0], [254.999, 0.999, 1.0], [127.5, 128.49, -0.0], [1e6, -1e6, 42.7], [255.0, 256.0, 254.5]], f32)
    unit = np.array([[-0.2, 1.0, 0.5], [0.999, 0.0039, 0.00392157], [0.5, 0.49999, 0.50001], [1.0, 1.0, -1.0], [0.1, 0.2, 0.3]], f32)
    return pc, big, unit, 2, 5


def splat_random(N, T, H, W, seed, margin=1e-3):
    """scattered cloud in front of T slightly different cameras; points whose fp64 image lies within `margin` px of a rounding / mask boundary that decides
    visibility (u or v at -0.5, W - 0.5, H - 0.5; z at 0) are moved to the optical axis"""
    rng = np.random.default_rng(seed)
    pc = (rng.normal(size=(N, 3)) * [1.0, 1.0, 0.4] + [0, 0, 3.0]).astype(f32)
    colors = (rng.random((N, 3)) * 255).astype(f32)
    K = np.stack([np.array([[W * 0.6 + 3 * t, 0, W / 2], [0, W * 0.62, H / 2], [0, 0, 1]], f32) for t in range(T)])
    E = np.stack([np.eye(4, dtype=f32) for _ in range(T)])
    for t in range(T):
        a = 0.05 * t
        E[t, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        E[t, :3, 3] = [0.1 * t, 0, 0.05 * t]
    pc[splat_margin(pc, K, E, H, W) < margin] = [0, 0, 3.0]
    return pc, colors, K, E


def splat_big():
    """N = 2048 x 256 + 300 points on 64 x 48, T = 2: the last 300 are what the point loop's second pass handles, and they lie nearer than the rest"""
    N = 2048 * 256 + 300
    pc, colors, K, E = splat_random(N, 2, 48, 64, 1)
    pc[-300:, 2] = pc[-300:, 2] * f32(0.25) + f32(0.75)
    pc[-300:][splat_margin(pc[-300:], K, E, 48, 64) < 1e-3] = [0, 0, 1.5]
    return pc, colors, K, E


def splat_margin(pc, K, E, H, W):
    """per point: the least fp64 distance, over the views, of (u, v, z) from a visibility boundary"""
    p = np.asarray(pc, f64)
    m = np.full(len(p), np.inf)
    for t in range(len(E)):
        cam = p @ np.asarray(E[t], f64)[:3, :3].T + np.asarray(E[t], f64)[:3, 3]
        pr = cam @ np.asarray(K[t], f64).T
        u, v, z = pr[:, 0] / pr[:, 2], pr[:, 1] / pr[:, 2], pr[:, 2]
        m = np.minimum(m, np.minimum.reduce([np.abs(u + 0.5), np.abs(u - (W - 0.5)), np.abs(v + 0.5), np.abs(v - (H - 0.5)), np.abs(z)]))
    return m


# ---------------------------------------------------------------------------------------------- frames: layout, range rules, bilinear resize
def nchw(x, dt, wrong=None):
    a = x.numpy() if torch.is_tensor(x) else np.asarray(x)
    if a.ndim == 3:
        a = a[None]
    if a.shape[-1] == 3:
        T, H, W, C = a.shape
        a = np.ascontiguousarray(a).reshape(T, C, H, W) if wrong == "hwc_as_chw" else a.transpose(0, 3, 1, 2)
    return np.ascontiguousarray(a).astype(f32).astype(dt)           # x.float() first: uint8 and float32 inputs are exact in both


def to_01(x, dt=f64, wrong=None):
    """metrics/mse.py:31-54.  Tensors: min < 0 -> (x + 1) / 2, elif max > 1 -> x / 255; numpy arrays: max > 1 -> x / 255."""
    a = nchw(x, dt, wrong)
    is_tensor = torch.is_tensor(x) != (wrong == "rules_swapped")
    mn, mx = a.min(), a.max()
    if wrong == "max_first" and is_tensor:
        return a / dt(255) if mx > 1 else ((a + dt(1)) / dt(2) if mn < 0 else a)
    if is_tensor and mn < 0:
        return (a + dt(1)) / dt(2)
    return a / dt(255) if mx > 1 else a


def to_pm1(x, dt=f64, wrong=None):
    """metrics/lpips.py:38-63.  Tensors: min >= 0 -> (max > 1 ? x / 255 : x) * 2 - 1, else unchanged; numpy arrays: (x / 255) * 2 - 1."""
    a = nchw(x, dt, wrong)
    is_tensor = torch.is_tensor(x) != (wrong == "rules_swapped")
    if not is_tensor:
        return (a / dt(255)) * dt(2) - dt(1)
    if a.min() >= 0:
        if a.max() > 1:
            a = a / dt(255)
        return a * dt(2) - dt(1)
    return a


def resize(t, size, dt=f64, wrong=None):
    """F.interpolate(t, size, mode='bilinear', align_corners=False): src = (dst + 0.5) * (in / out) - 0.5 clamped at 0, i0 = floor(src), i1 = min(i0 + 1, in - 1);
    combined as (a00 wx0 + a01 wx1) wy0 + (a10 wx0 + a11 wx1) wy1 (the order of oracle.scorer.bilinear_resize and of the kernels)"""
    t = np.asarray(t, dt)
    h, w = t.shape[-2:]
    H, W = size

    def axis(n_in, n_out):
        if wrong == "align_corners":
            src = np.arange(n_out, dtype=dt) * (dt(n_in - 1) / dt(max(n_out - 1, 1)))
        else:
            src = np.maximum((np.arange(n_out, dtype=dt) + dt(0.5)) * (dt(n_in) / dt(n_out)) - dt(0.5), dt(0))
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        l1 = (src - i0.astype(dt)).astype(dt)
        return i0, i1, (dt(1) - l1).astype(dt), l1

    y0, y1, wy0, wy1 = axis(h, H)
    x0, x1, wx0, wx1 = axis(w, W)
    top = t[:, :, y0][:, :, :, x0] * wx0 + t[:, :, y0][:, :, :, x1] * wx1
    bot = t[:, :, y1][:, :, :, x0] * wx0 + t[:, :, y1][:, :, :, x1] * wx1
    return (top * wy0[:, None] + bot * wy1[:, None]).astype(dt)


def frame_metric(gt, rep, psnr=False, dt=f64, wrong=None):
    """MSEMetric / PSNRMetric.compute (metrics/mse.py:14-29,61-74) in dt"""
    g, r = to_01(gt, dt, wrong), to_01(rep, dt, wrong)
    if g.shape[-2:] != r.shape[-2:]:
        r = resize(r, g.shape[-2:], dt, wrong)
    d = g - r
    m = np.mean(d * d, dtype=dt)
    if not psnr:
        return float(m)
    return 100.0 if m == 0 else float(dt(10) * np.log10(dt(1) / m))


def frames_pm1(x, size=None, dt=f64, wrong=None):
    """LPIPSMetric's input side: to [-1,1], then the resize of metrics/lpips.py:31-32"""
    a = to_pm1(x, dt, wrong)
    return a if size is None or tuple(size) == a.shape[-2:] else resize(a, size, dt, wrong)


ARMS = [(d, l, t) for d in ("f32", "u8") for l in (0, 1) for t in (True, False)]          # dtype, layout (0 [T,C,H,W] / 1 [T,H,W,C]), torch.Tensor or numpy
RANGES = {"f32": ("01", "pm1", "255"), "u8": ("bin", "255")}


def make_frames(seed, T, C, H, W, dtype, layout, is_tensor, kind):
    """a seeded frame container of one arm and value range.  "01": [0,1] with a 1.0 and a -0.0 in it (the minimum is -0.0: not < 0); "pm1": [-1,1]; "255": up to 255
    (uint8: whole numbers); "bin": uint8 zeros and ones (max is not > 1: no division)."""
    rng = np.random.default_rng(seed)
    shape = (T, H, W, C) if layout else (T, C, H, W)
    n = int(np.prod(shape))
    if dtype == "u8":
        a = rng.integers(0, 2 if kind == "bin" else 256, size=n, dtype=np.uint8)
        a[0], a[-1] = (1, 0) if kind == "bin" else (255, 0)
    else:
        a = rng.random(n).astype(f32)
        if kind == "01":
            a[n // 2], a[n // 3] = f32(1.0), f32(-0.0)
        elif kind == "pm1":
            a = a * f32(2) - f32(1)
            a[n // 2], a[n // 3] = f32(1.0), f32(-1.0)
        else:
            a = a * f32(255)
    a = a.reshape(shape)
    return torch.from_numpy(a) if is_tensor else a


# ---------------------------------------------------------------------------------------------- MVCS
def inv3_adj(a):
    """adjugate / determinant in double, in the order of scorer2.hip::inv3"""
    a = [float(v) for v in np.asarray(a, f64).ravel()]
    c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
    det = (a[0] * c00 + a[1] * c01) + a[2] * c02
    i = 1.0 / det
    return np.array([c00 * i, (a[2] * a[7] - a[1] * a[8]) * i, (a[1] * a[5] - a[2] * a[4]) * i,
                     c01 * i, (a[0] * a[8] - a[2] * a[6]) * i, (a[2] * a[3] - a[0] * a[5]) * i,
                     c02 * i, (a[1] * a[6] - a[0] * a[7]) * i, (a[0] * a[4] - a[1] * a[3]) * i], f64).reshape(3, 3)


def mvcs(depths, intrinsics, extrinsics, dt=f64, wrong=None, diag=None):
    """MVCSMetric.compute (metrics/mvcs.py:12-114) in dt; the 3 x 3 inverse and the relative pose are formed in double and rounded to dt once.  diag (a list) gets
    one dict per pair: mask, pixel_margin (each pixel's least distance of u, v, z from a mask boundary) and its minimum margin, n_edge (masked pixels whose bilinear footprint leaves the image)."""
    d = np.asarray(depths, f32)
    if d.ndim == 4:
        d = d[:, 0] if d.shape[1] == 1 else d[..., 0]
    d = d.astype(dt)
    K64 = np.asarray(intrinsics, f32)[..., :3, :3].astype(f64)
    E64 = np.asarray(extrinsics, f32).astype(f64)
    T, H, W = d.shape
    if E64.shape[-2:] == (3, 4):
        E64 = np.concatenate([E64, np.broadcast_to(np.array([0, 0, 0, 1.0]), (T, 1, 4))], axis=1)
    ys, xs = np.meshgrid(np.arange(H, dtype=dt), np.arange(W, dtype=dt), indexing="ij")
    x, y = xs.ravel(), ys.ravel()
    scores = []
    for i in range(T - 1):
        j = i + 1
        Ki = np.linalg.inv(K64[i]).astype(dt)
        rel = (E64[j] @ np.linalg.inv(E64[i])).astype(dt)
        Kj = K64[j].astype(dt)
        di = d[i].ravel()
        with np.errstate(all="ignore"):
            pi = [((Ki[r, 0] * x + Ki[r, 1] * y) + Ki[r, 2]) * di for r in range(3)]
            pj = [((rel[r, 0] * pi[0] + rel[r, 1] * pi[1]) + rel[r, 2] * pi[2]) + rel[r, 3] for r in range(3)]
            hj = [(Kj[r, 0] * pj[0] + Kj[r, 1] * pj[1]) + Kj[r, 2] * pj[2] for r in range(3)]
            zc = np.maximum(hj[2], dt(1e-8))
            u, v, z = hj[0] / zc, hj[1] / zc, pj[2]
            gx, gy = dt(2) * u / dt(W - 1) - dt(1), dt(2) * v / dt(H - 1) - dt(1)
            ix, iy = (gx + dt(1)) / dt(2) * dt(W - 1), (gy + dt(1)) / dt(2) * dt(H - 1)
            x0, y0 = np.floor(ix), np.floor(iy)
            wx1, wy1 = ix - x0, iy - y0
            wx0, wy0 = dt(1) - wx1, dt(1) - wy1

            def tap(xx, yy):
                ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
                val = d[j][np.clip(np.nan_to_num(yy), 0, H - 1).astype(np.int64), np.clip(np.nan_to_num(xx), 0, W - 1).astype(np.int64)]
                return val if wrong == "no_zero_pad" else np.where(ok, val, dt(0))

            s = tap(x0, y0) * (wx0 * wy0) + tap(x0 + 1, y0) * (wx1 * wy0) + tap(x0, y0 + 1) * (wx0 * wy1) + tap(x0 + 1, y0 + 1) * (wx1 * wy1)
            mask = (u >= 0) & ((u <= W) if wrong == "mask_u_le_W" else (u < W)) & (v >= 0) & (v < H) & (z > 0)
        if diag is not None:
            with np.errstate(all="ignore"):
                m = np.minimum.reduce([np.abs(u), np.abs(u - W), np.abs(v), np.abs(v - H), np.abs(z)])
            diag.append({"mask": mask, "pixel_margin": m, "margin": float(np.nanmin(m)), "n_edge": int((mask & ((u > W - 1) | (v > H - 1))).sum())})
        if mask.any():
            e = s[mask] - z[mask]
            scores.append(float(np.mean(e * e, dtype=dt)))
    return float(np.exp(-1.0 * np.mean(scores))) if scores else 0.0


def rot(axis, angle):
    """Rodrigues, double"""
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def mvcs_cams(T, H, W, seed, affine=False):
    """K with non-zero skew and an off-centre principal point, differing per view; E a rigid motion per view (affine: its 3 x 3 block mildly non-orthonormal,
    which the general inverse of the relative pose must handle)"""
    rng = np.random.default_rng(seed)
    K = np.stack([np.array([[1.1 * W + 0.5 * t, 0.7, 0.46 * W + 0.3 * t], [0, 1.05 * W, 0.55 * H], [0, 0, 1]], f32) for t in range(T)])
    E = np.stack([np.eye(4, dtype=f32) for _ in range(T)])
    for t in range(T):
        R = rot([0.3, 1.0, 0.2], 0.025 * t + 0.01)
        if affine:
            R = R @ (np.eye(3) + 0.02 * rng.normal(size=(3, 3)))
        E[t, :3, :3] = R
        E[t, :3, 3] = [0.04 * t, -0.015 * t, 0.02 * t]
    return K, E


def mvcs_depth(T, H, W, seed, noise=0.01):
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([2.0 + 0.3 * np.sin(xs / W * 3 + 0.2 * t) + 0.2 * np.cos(ys / H * 2) + noise * rng.normal(size=(H, W)) for t in range(T)]).astype(f32)


def nudge_depth(depth, K, E, margin=2e-3):
    """pixels whose fp64 reprojection comes within `margin` px of a mask boundary get a slightly larger depth until none does (at most a few pixels, a few rounds)"""
    depth = depth.copy()
    for _ in range(20):
        diag = []
        mvcs(depth, K, E, f64, diag=diag)
        moved = False
        for i, dg in enumerate(diag):
            if dg["margin"] < margin:
                depth[i][(dg["pixel_margin"] < margin).reshape(depth.shape[1:])] *= f32(1.013)
                moved = True
        if not moved:
            return depth
    raise AssertionError("nudge_depth did not converge")


def mvcs_family(T, H, W, seed, affine=False):
    K, E = mvcs_cams(T, H, W, seed, affine)
    return nudge_depth(mvcs_depth(T, H, W, seed + 1), K, E), K, E


def mvcs_away_family(all_pairs):
    """T = 3: view 1 and 2 look the other way (a half turn about y), so pair (0, 1) has no valid pixel and is skipped while pair (1, 2) counts;
    all_pairs: T = 2 of it, nothing counts, the score is 0.0"""
    H, W = 12, 17
    K, E = mvcs_cams(3, H, W, 5)
    flip = np.diag([-1.0, 1.0, -1.0])
    for t in (1, 2):
        E[t, :3, :3] = (flip @ E[t, :3, :3].astype(f64)).astype(f32)
        E[t, :3, 3] = (flip @ E[t, :3, 3].astype(f64)).astype(f32)
    d = mvcs_depth(3, H, W, 6)
    if all_pairs:
        return d[:2], K[:2], E[:2]
    return nudge_depth(d, K, E), K, E


def mvcs_boundary_family():
    """Built to sit ON the mask boundary (exempt from the margin condition): K = I, depth_i = 1, view j shifted by one pixel in x.  u = x + 1 exactly, so the last
    column has u = W exactly: not < W, masked out.  A mask `u <= W` takes it in with all four taps outside the image."""
    H, W = 7, 9
    K = np.stack([np.eye(3, dtype=f32)] * 2)
    E = np.stack([np.eye(4, dtype=f32)] * 2)
    E[1, 0, 3] = 1.0
    d = np.ones((2, H, W), f32)
    d[1] += (0.25 * np.sin(np.arange(H * W).reshape(H, W))).astype(f32)
    return d, K, E


def pad_K4(K):
    K4 = np.zeros(K.shape[:-2] + (4, 4), f32)
    K4[..., :3, :3] = K
    K4[..., 3, 3] = 1
    K4[..., :3, 3] = 7.5         # never read
    return K4


# ---------------------------------------------------------------------------------------------- unprojection, pose decode
def unproject(depths, K, E, dt=f64):
    """world = c2w [K^-1 (x, y, 1) depth], c2w = [R^T | -R^T t] (depth_anything_3/utils/geometry.py:54-59 assumes R orthonormal, and so does everything here).
    dt float32 is the kernel's order: K^-1 by the adjugate in double rounded once, ((k0 x + k1 y) + k2) d, ((r0 c0 + r1 c1) + r2 c2) + t."""
    d = np.asarray(depths, f32).astype(dt)
    T, H, W = d.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=dt), np.arange(W, dtype=dt), indexing="ij")
    out = np.empty((T, H, W, 3), dt)
    for t in range(T):
        Ki = inv3_adj(np.asarray(K[t], f32)).astype(dt)
        Et = np.asarray(E[t], f32).astype(dt)
        cam = [((Ki[r, 0] * xs + Ki[r, 1] * ys) + Ki[r, 2]) * d[t] for r in range(3)]
        for r in range(3):
            tr = -((Et[0, r] * Et[0, 3] + Et[1, r] * Et[1, 3]) + Et[2, r] * Et[2, 3])
            out[t, ..., r] = ((Et[0, r] * cam[0] + Et[1, r] * cam[1]) + Et[2, r] * cam[2]) + tr
    return out


def unproject_cams(T, H, W, seed):
    rng = np.random.default_rng(seed)
    K = np.stack([np.array([[0.9 * W + t, 1.3, 0.45 * W], [0, 0.95 * W, 0.52 * H + t], [0, 0, 1]], f32) for t in range(T)])
    E = np.stack([np.eye(4, dtype=f32) for _ in range(T)])
    for t in range(T):
        E[t, :3, :3] = rot(rng.normal(size=3), 0.2 + 0.3 * t)
        E[t, :3, 3] = rng.normal(size=3)
    return K, E


def pose_decode(pe, image_hw=None, dt=f64):
    """vggt/utils/pose_enc.py:62-124 + rotation.py:14-44 in dt, in the kernel's order: two_s = 2 / (((i i + j j) + k k) + r r) -> (ext [n,3,4], intr [n,3,3] | None)"""
    p = np.asarray(pe, f32).reshape(-1, 9).astype(dt)
    i, j, k, r = p[:, 3], p[:, 4], p[:, 5], p[:, 6]
    two_s = dt(2) / (((i * i + j * j) + k * k) + r * r)
    one = dt(1)
    R = np.stack([one - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                  two_s * (i * j + k * r), one - two_s * (i * i + k * k), two_s * (j * k - i * r),
                  two_s * (i * k - j * r), two_s * (j * k + i * r), one - two_s * (i * i + j * j)], -1).reshape(-1, 3, 3)
    ext = np.concatenate([R, p[:, :3, None]], -1).astype(dt)
    if image_hw is None:
        return ext, None
    H, W = image_hw
    intr = np.zeros((len(p), 3, 3), dt)
    intr[:, 1, 1] = (dt(H) / dt(2)) / np.tan(p[:, 7] / dt(2))
    intr[:, 0, 0] = (dt(W) / dt(2)) / np.tan(p[:, 8] / dt(2))
    intr[:, 0, 2], intr[:, 1, 2], intr[:, 2, 2] = dt(W) / dt(2), dt(H) / dt(2), one
    return ext, intr


def pose_family(n, seed):
    """non-unit quaternions (norms 0.3 .. 3), fields of view spread over 0.2 .. 2.5 rad"""
    rng = np.random.default_rng(seed)
    pe = np.empty((n, 9), f32)
    pe[:, :3] = rng.normal(size=(n, 3))
    q = rng.normal(size=(n, 4))
    pe[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.3, 3.0, size=(n, 1))
    pe[:, 7] = np.linspace(0.2, 2.5, n) if n > 1 else 0.2
    pe[:, 8] = np.linspace(2.5, 0.2, n) if n > 1 else 2.5
    return pe


# ---------------------------------------------------------------------------------------------- motion score
def motion(E, dt=f64):
    """compute_motion_score_vectorized (metrics/consistency_score.py:8-40) in dt: mean ||dt|| + 0.1 mean acos(clamp((tr(R_{i+1} R_i^T) - 1) / 2)), NaN (T = 1) -> 0"""
    E = np.asarray(E, f32).astype(dt)
    if len(E) < 2:
        return 0.0
    R, t = E[:, :3, :3], E[:, :3, 3]
    dtr = np.sqrt(((t[1:] - t[:-1]) ** 2).sum(-1))
    tr = (R[1:] * R[:-1]).sum((-1, -2))
    ang = np.arccos(np.clip((tr - dt(1)) / dt(2), dt(-1), dt(1)))
    return float(dtr.mean(dtype=dt) + dt(0.1) * ang.mean(dtype=dt))


MOTION_T = (1, 2, 3, 65, 66, 130)
_SIGNED_PERM = np.array([[0, -1, 0], [0, 0, 1], [-1, 0, 0]], f64)        # a rotation (det +1) whose products are exact in any precision


def motion_family(kind, T, seed=0):
    """[T,4,4] poses.  "walk": a random walk of well-conditioned turns (0.05 .. 0.3 rad per step).  "still": one signed-permutation rotation for every frame, only
    the translation moves: trace exactly 3, the clamp applies, angle 0.  "half_turn": consecutive frames differ by diag(-1,-1,1): trace exactly -1, angle pi.
    "tiny": turns of 1e-4 rad about a generic axis.  acos near 1 turns the ~1e-7 rounding of an fp32 trace into up to 5e-4 rad, 5e-5 of score, so this family
    moves ~60 units per step: the cap (relative to max(1, |score|)) then admits that, and still sees a wrong translation term.  "tiny_z": the same angle about z
    from the identity, alternating: cos(1e-4) rounds to 1.0f, every product is exact, fp32 and fp64 agree on angle 0 at unit-size translations."""
    rng = np.random.default_rng(seed + 17 * T)
    E = np.stack([np.eye(4) for _ in range(T)])
    R = np.eye(3)
    for i in range(T):
        if kind == "walk":
            R = rot(rng.normal(size=3), rng.uniform(0.05, 0.3)) @ R
            E[i, :3, 3] = 0.1 * i + 0.05 * rng.normal(size=3)
        elif kind == "still":
            R = _SIGNED_PERM
            E[i, :3, 3] = rng.normal(size=3)
        elif kind == "half_turn":
            R = np.diag([-1.0, -1.0, 1.0]) if i % 2 else np.eye(3)
            E[i, :3, 3] = [0.25 * i, 0.5, -0.125 * i]
        elif kind == "tiny":
            R = rot([0.5, -0.3, 0.8], 1e-4) @ R
            E[i, :3, 3] = [60.0 * i, 3.0 * (i % 3), -7.0 * i]
        elif kind == "tiny_z":
            R = rot([0, 0, 1], 1e-4) if i % 2 else np.eye(3)
            E[i, :3, 3] = rng.normal(size=3)
        E[i, :3, :3] = R
    return E.astype(f32)


# ---------------------------------------------------------------------------------------------- epipolar
def two_view(n, seed, noise, turn=0.08):
    """n matches of a scattered scene under two cameras (pixels, float32), Gaussian noise of `noise` px on both sides"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 3)) * [1.0, 0.8, 1.2] + np.array([0, 0, 5.0])
    K = np.array([[400.0, 0, 160], [0, 400.0, 120], [0, 0, 1]])
    R = rot([0.1, 1.0, 0.05], turn)
    t = np.array([0.3, 0.05, 0.1])
    a1 = (K @ X.T).T
    a2 = (K @ (R @ X.T + t[:, None])).T
    p1 = a1[:, :2] / a1[:, 2:] + noise * rng.normal(size=(n, 2))
    p2 = a2[:, :2] / a2[:, 2:] + noise * rng.normal(size=(n, 2))
    return p1.astype(f32), p2.astype(f32)


def design_eigs(p1, p2):
    """ascending eigenvalues of X^T X of the normalised 8-point design matrix"""
    n1, _ = osc._normalize_points(np.asarray(p1, f64))
    n2, _ = osc._normalize_points(np.asarray(p2, f64))
    x1, y1, x2, y2 = n1[:, 0], n1[:, 1], n2[:, 0], n2[:, 1]
    X = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], axis=1)
    return np.linalg.eigvalsh(X.T @ X)


def epipolar_pairs():
    """The pairs of the one call, in offsets order -> list of (kind, p1, p2).  kind "F": error and F compared; "empty" / "few": err -1, F zeros; "same": p1 == p2,
    error sqrt(1e-8), F not compared (a three-dimensional null space); "line": 20 collinear points, finite only.  Noise is 0.1 px (0.05 at 9 matches): at 0.5 px the
    two smallest eigenvalues of the design matrix are only a factor ~100 apart, and F is compared only where that factor is at least 1e3."""
    e = np.zeros((0, 2), f32)
    rng = np.random.default_rng(99)
    same = (rng.random((300, 2)) * [320, 240]).astype(f32)
    s = np.linspace(0, 1, 20)
    line1 = np.stack([20 + 250 * s, 30 + 170 * s], 1).astype(f32)
    line2 = np.stack([25 + 240 * s, 28 + 175 * s], 1).astype(f32)
    return [("empty", e, e),
            ("F",) + two_view(8, 1, 0.0),
            ("F",) + two_view(9, 2, 0.05),
            ("F",) + two_view(255, 3, 0.0),
            ("F",) + two_view(256, 4, 0.1),
            ("empty", e, e),
            ("F",) + two_view(257, 5, 0.1),
            ("F",) + two_view(2048, 6, 0.1),
            ("same", same, same.copy()),
            ("line", line1, line2),
            ("few",) + two_view(7, 7, 0.0),
            ("empty", e, e)]


# ---------------------------------------------------------------------------------------------- shared case lists (host and device tests walk the same ones)
def frame_metric_cases():
    """-> [(name, gt, rep, cap key)]: all 64 (dtype, layout, container) pairs x the value ranges each dtype allows x rep at gt's size and at 4 x 9; then the resize
    shapes, and 300 x 300 (more elements than one pass of the grid)"""
    out = []
    for gi, (gd, gl, gt_t) in enumerate(ARMS):
        for ri, (rd, rl, rt_t) in enumerate(ARMS):
            for gk in RANGES[gd]:
                for rk in RANGES[rd]:
                    for (h2, w2) in ((5, 7), (4, 9)):
                        seed = 1000 * gi + 100 * ri + 10 * RANGES[gd].index(gk) + RANGES[rd].index(rk)
                        gt = make_frames(seed, 2, 3, 5, 7, gd, gl, gt_t, gk)
                        rep = make_frames(seed + 7919, 2, 3, h2, w2, rd, rl, rt_t, rk)
                        tag = lambda d, l, t, k: f"{d}/{'THWC' if l else 'TCHW'}/{'tensor' if t else 'numpy'}/{k}"
                        out.append((f"{tag(gd, gl, gt_t, gk)} vs {tag(rd, rl, rt_t, rk)} {h2}x{w2}", gt, rep, "mse" if (h2, w2) == (5, 7) else "mse_resize"))
    for name, (H, W), (h2, w2) in (("rep 1x1", (5, 7), (1, 1)), ("rep 1x9", (5, 7), (1, 9)), ("up 3x4 -> 11x13", (11, 13), (3, 4)),
                                   ("down 37x41 -> 5x7", (5, 7), (37, 41)), ("equal height 5x9 -> 5x7", (5, 7), (5, 9))):
        out.append((name, make_frames(1, 2, 3, H, W, "f32", 0, True, "pm1"), make_frames(2, 2, 3, h2, w2, "u8", 1, False, "255"), "mse_resize"))
    over = lambda seed, h, w: torch.from_numpy(np.concatenate([[f32(1.004), f32(-1.0)], make_frames(seed, 2, 3, h, w, "f32", 0, False, "pm1").ravel()[2:]]).reshape(2, 3, h, w))
    out.append(("f32/TCHW/tensor/[-1,1] overshooting to 1.004 (min < 0 AND max > 1) 5x7", over(11, 5, 7), over(12, 5, 7), "mse"))
    out.append(("f32/TCHW/tensor/[-1,1] overshooting to 1.004 (min < 0 AND max > 1) 4x9", over(13, 5, 7), over(14, 4, 9), "mse_resize"))
    out.append(("1x3x300x300 float vs uint8 THWC", make_frames(3, 1, 3, 300, 300, "f32", 0, True, "01"), make_frames(4, 1, 3, 300, 300, "u8", 1, True, "255"), "mse"))
    return out


def pm1_cases():
    """-> [(name, x, size)]: all 8 arms x ranges x {same size, 5 x 7 -> 8 x 5, 9 x 9 -> 1 x 1}; 420 x 420 same size and -> 424 x 416 (past the grid cap)"""
    out = []
    for ai, (d, l, t) in enumerate(ARMS):
        for k in RANGES[d]:
            for (hw, size) in (((5, 7), None), ((5, 7), (8, 5)), ((9, 9), (1, 1))):
                out.append((f"{d}/{'THWC' if l else 'TCHW'}/{'tensor' if t else 'numpy'}/{k} {hw}->{size}", make_frames(50 * ai + len(out), 2, 3, hw[0], hw[1], d, l, t, k), size))
    out.append(("420x420 same", make_frames(5, 1, 3, 420, 420, "u8", 1, False, "255"), (420, 420)))
    out.append(("420x420 -> 424x416", make_frames(6, 1, 3, 420, 420, "f32", 0, True, "01"), (424, 416)))
    return out


def mvcs_cases():
    """-> [(name, depth [T,H,W], K [T,3,3], E [T,4,4])]: smooth depth + noise on 24 x 31 at T = 2, 3, 5 (skewed, off-centre K; rigid E), the affine E, the pair that
    is skipped, and 200 x 340 (more pixels than one pass of the grid)"""
    out = [(f"T={T} 24x31", *mvcs_family(T, 24, 31, 10 + T)) for T in (2, 3, 5)]
    out.append(("affine E T=3 24x31", *mvcs_family(3, 24, 31, 20, affine=True)))
    out.append(("skipped pair T=3 12x17", *mvcs_away_family(False)))
    out.append(("T=2 200x340", *mvcs_family(2, 200, 340, 30)))
    return out


def motion_cases():
    out = [(f"{kind} T={T}", motion_family(kind, T)) for kind in ("walk", "still", "half_turn", "tiny", "tiny_z") for T in MOTION_T]
    return out
