"""Depth Anything 3's ray-based cameras restated in plain torch, in any dtype and on any device: the oracle of tests/test_da3_raypose_host.py and
tests/test_gpu_da3_raypose.py, and the torch side of tools/da3_ray_pose_bench.py.  Not a test module.

What it states (depth_anything_3/utils/ray_utils.py:20-93,313-421 and model/da3.py:181-201 say the same with sorts, a batched SVD and a full SVD):
a point of the ray map pairs the plane-grid position (x, y, 1) with the direction ray[:3]; directions whose |z| exceeds 1e-4 (strictly, compared in
fp32) are divided by z, the others keep their xy and lose their confidence.  A homography H with H (x, y, 1) ~ (u, v, 1) is fitted to 8 of the most
confident points 100 times; the fit whose inliers (reprojection error < threshold) weigh most wins, lowest index on a tie, and H is fitted again to
those inliers (to a random 8000 of the top 95 % by weight when there are more).  A fit is the null direction of the weighted DLT system, here the
eigenvector of the smallest eigenvalue of its 9 x 9 normal matrix (`torch.linalg.eigh`), scaled to H[2,2] = 1.  H, negated when its determinant is
negative, factors into a rotation times a lower-triangular matrix with a positive diagonal; the triangle over its last entry gives 1 / focal on the
diagonal and the principal point minus 1 in its last row.  T is the confidence-weighted mean of ray[3:], with the lost confidences counting as zero.

`dtype` is the arithmetic behind the fp32 inputs: torch.float64 is the oracle; torch.float32 shows what rounding alone does to the result."""
import torch

N_ITER, SAMPLES, SAMPLE_RATIO, MAX_INLIERS, Z_THRESHOLD = 100, 8, 0.3, 8000, 1e-4


def plane_grid(ph, pw):
    """fp32 (x [pw], y [ph]): cell centres of a 2 x 2 image seen from its middle, as upstream builds them (fp32 linspace over (0, 2), minus 1)"""
    axis = lambda n: torch.linspace(-(1 - 1 / n) + 1.0, (1 - 1 / n) + 1.0, n, dtype=torch.float32) - 1.0
    return axis(pw), axis(ph)


def normalise(ray, conf, dtype=torch.float64):
    """ray fp32 [V,ph,pw,6], conf fp32 [V,ph,pw] -> x, y, u, v, w, each [V,N] in `dtype`, and the fp32 masked weights"""
    V, ph, pw, _ = ray.shape
    gx, gy = (t.to(ray.device) for t in plane_grid(ph, pw))
    x = gx.to(dtype).view(1, 1, pw).expand(V, ph, pw).reshape(V, -1)
    y = gy.to(dtype).view(1, ph, 1).expand(V, ph, pw).reshape(V, -1)
    d = ray[..., :3].reshape(V, -1, 3)
    valid = d[..., 2].abs() > Z_THRESHOLD                      # an fp32 comparison, as upstream's
    z = torch.where(valid, d[..., 2], torch.ones_like(d[..., 2])).to(dtype)
    wm = torch.where(valid, conf.reshape(V, -1), torch.zeros_like(conf.reshape(V, -1)))
    return x, y, d[..., 0].to(dtype) / z, d[..., 1].to(dtype) / z, wm.to(dtype), wm


def fit(x, y, u, v, w):
    """[..., K] each -> H [..., 3, 3] with H[2,2] = 1: the eigenvector of the smallest eigenvalue of the weighted DLT normal matrix"""
    s, one, zero = w.sqrt(), torch.ones_like(x), torch.zeros_like(x)
    r1 = torch.stack([-x, -y, -one, zero, zero, zero, x * u, y * u, u], dim=-1) * s[..., None]
    r2 = torch.stack([zero, zero, zero, -x, -y, -one, x * v, y * v, v], dim=-1) * s[..., None]
    A = torch.cat([r1, r2], dim=-2)
    _, vecs = torch.linalg.eigh(A.mT @ A)
    h = vecs[..., :, 0]
    return (h / h[..., 8:9]).reshape(*h.shape[:-1], 3, 3)


def reprojection_error(H, x, y, u, v):
    """H [V,M,3,3], points [V,N] -> [V,M,N]"""
    p = torch.stack([x, y, torch.ones_like(x)], dim=-1)
    q = torch.einsum("vmij,vnj->vmni", H, p)
    return ((q[..., 0] / q[..., 2] - u[:, None]) ** 2 + (q[..., 1] / q[..., 2] - v[:, None]) ** 2).sqrt()


def candidates(wm, n_sample):
    return torch.sort(wm, dim=1, descending=True, stable=True).indices[:, :n_sample]


def hypotheses(x, y, u, v, w, wm, sample_idx):
    """-> H [V,n_iter,3,3] of the sampled candidate octets"""
    N = x.shape[1]
    pick = candidates(wm, max(SAMPLES, int(N * SAMPLE_RATIO)))[:, sample_idx.long()]                 # [V,n_iter,8]
    take = lambda t: torch.gather(t[:, None].expand(-1, pick.shape[1], -1), 2, pick)
    return fit(take(x), take(y), take(u), take(v), take(w))


def scores(H, x, y, u, v, w, threshold):
    inl = reprojection_error(H, x, y, u, v) < threshold
    return (inl * w[:, None]).sum(dim=-1), inl


def decompose(H):
    """H [3,3] -> (R, focal [2], pp [2])"""
    A = -H if torch.linalg.det(H) < 0 else H
    Q, U = torch.linalg.qr(A.flip(1))                          # A with its columns reversed = Q U; un-reversing both makes U lower-triangular
    Q, L = Q.flip(1), U.flip(0).flip(1)
    sg = torch.sign(torch.diagonal(L))
    Q, L = Q * sg[None, :], L * sg[:, None]
    L = L / L[2, 2]
    return Q, 1.0 / torch.stack([L[0, 0], L[1, 1]]), torch.stack([L[2, 0], L[2, 1]]) + 1.0


def ray_pose(ray, conf, image_hw, sample_idx, reproj_threshold=0.2, dtype=torch.float64, generator=None):
    """ray fp32 [B,S,ph,pw,6], conf fp32 [B,S,ph,pw], sample_idx integer [n_iter,8] -> a dict of [B*S, ...] tensors in `dtype`: H, R, T, focal, pp,
    extrinsics [.,3,4], intrinsics [.,3,3], and best, n_inliers, n_used (int64), score [., n_iter], margin [.] (the smallest distance of any point's
    error from the threshold under the winner).  `generator` draws the 8000 when a winner has more inliers."""
    ray, conf = ray.flatten(0, 1), conf.flatten(0, 1)
    V = ray.shape[0]
    x, y, u, v, w, wm = normalise(ray, conf, dtype)
    H_all = hypotheses(x, y, u, v, w, wm, sample_idx.to(ray.device))
    score, inl = scores(H_all, x, y, u, v, w, reproj_threshold)
    best = torch.argmax(score, dim=1)
    ar = torch.arange(V, device=ray.device)
    mask = inl[ar, best]
    err = reprojection_error(H_all[ar, best][:, None], x, y, u, v)[:, 0]
    out = dict(best=best, n_inliers=mask.sum(dim=1), score=score, margin=(err - reproj_threshold).abs().min(dim=1).values)
    t = ray[..., 3:].reshape(V, -1, 3).to(dtype)
    out["T"] = (t * w[..., None]).sum(dim=1) / w.sum(dim=1, keepdim=True)
    rows = {k: [] for k in ("H", "R", "focal", "pp", "n_used")}
    for b in range(V):
        idx = torch.nonzero(mask[b])[:, 0]
        if idx.numel() < 4:
            raise ValueError("At least 4 points are required to compute homography.")
        if idx.numel() > MAX_INLIERS:
            keep = max(int(idx.numel() * 0.95), MAX_INLIERS)
            order = torch.sort(wm[b][idx], descending=True, stable=True).indices[:keep]
            perm = torch.randperm(keep, generator=generator, device=generator.device if generator is not None else ray.device)[:MAX_INLIERS]
            idx = idx[order[perm.to(ray.device)]]
        H = fit(x[b][idx], y[b][idx], u[b][idx], v[b][idx], w[b][idx])
        R, focal, pp = decompose(H)
        for k, val in (("H", H), ("R", R), ("focal", focal), ("pp", pp), ("n_used", torch.tensor(idx.numel()))):
            rows[k].append(val)
    out.update({k: torch.stack(vals) for k, vals in rows.items()})
    out["extrinsics"], out["intrinsics"] = cameras(out["R"], out["T"], out["focal"], out["pp"], image_hw)
    return out


def cameras(R, T, focal, pp, image_hw):
    """[R|T]^-1 = [R^T | -R^T T] (rows :3) and the pixel intrinsics of an image_hw = (H, W) frame"""
    Himg, Wimg = image_hw
    ext = torch.cat([R.mT, -(R.mT @ T[..., None])], dim=-1)
    K = torch.zeros(*R.shape[:-2], 3, 3, dtype=R.dtype, device=R.device)
    K[..., 0, 0], K[..., 1, 1] = focal[..., 0] / 2 * Wimg, focal[..., 1] / 2 * Himg
    K[..., 0, 2], K[..., 1, 2], K[..., 2, 2] = pp[..., 0] * Wimg * 0.5, pp[..., 1] * Himg * 0.5, 1.0
    return ext, K


OUTPUTS = ("H", "R", "T", "focal", "pp", "extrinsics", "intrinsics")
E_SEEDS = 8
_CACHE = {}


def fixture():
    """tests/golden/da3_raypose.pt (make_golden_raypose.py), loaded once"""
    if "fixture" not in _CACHE:
        import os
        _CACHE["fixture"] = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "da3_raypose.pt"))
    return _CACHE["fixture"]


def oracle(name):
    """The fp64 oracle of a fixture case on the CPU, computed once and shared: ray_pose in float64 on the stored fp32 inputs.  Case e draws its 8000
    points: there the outputs are the mean over E_SEEDS generator seeds, as the stored reference results are"""
    if name not in _CACHE:
        fx = fixture()
        c = fx[name]
        run = lambda seed: ray_pose(c["ray"], c["conf"], fx["image_hw"], c["sample_idx"], fx["threshold"], torch.float64, torch.Generator().manual_seed(seed))
        out = run(0)
        if name == "e":
            runs = [out] + [run(s) for s in range(1, E_SEEDS)]
            out = dict(out, **{k: torch.stack([r[k] for r in runs]).mean(0) for k in OUTPUTS})
        _CACHE[name] = out
    return _CACHE[name]


def bounds(name):
    """{output kind: (bound, d_ref)} of a fixture case: `bound` below on the stored fp32 results and the oracle; case e adds 3 x the reference's stored
    seed-to-seed deviation (the room a ninth draw gets over the largest of eight)"""
    c, o = fixture()[name], oracle(name)
    out = {}
    for k in OUTPUTS:
        b, d_ref = bound(k, c[f"{k}32"], o[k])
        out[k] = (b + (3 * c[f"{k}32_dev"] if name == "e" else 0.0), d_ref)
    return out


def distance(a, b):
    """the largest absolute difference, in fp64"""
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def bound(kind, stored32, oracle64):
    """The issue's bound for one output kind of one fixture case: twice the largest distance of the reference's stored fp32 result from the fp64 oracle
    over the case's views, and no less than 4 fp32 ulps of the output's largest magnitude"""
    d_ref = distance(stored32, oracle64)
    floor = 4 * 2.0 ** -23 * float(oracle64.abs().max())
    return max(2 * d_ref, floor), d_ref
