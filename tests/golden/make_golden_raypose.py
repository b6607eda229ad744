"""Writes tests/golden/da3_raypose.pt: Depth Anything 3's ray-based camera estimation (depth_anything_3/utils/ray_utils.py, model/da3.py:181-201)
imported from the reference and run on the CPU, on synthetic ray maps.

    python tests/golden/make_golden_raypose.py /path/to/reference

Tensors and numbers only, below 1 MiB.  A view is a known camera (rotation, focal lengths, principal-point terms) seen through the plane grid:
directions R L (x, y, 1) with Gaussian noise (sigma 0.01), 18 % outlier rays with low confidence, all confidences distinct, and per-point translations
around a known one.  A further 12 % of the rays are outliers with HIGH confidence, two fifths of the candidate pool: with Gaussian noise and low-confidence
outliers alone the screening below cannot pass, because every hypothesis then fits every inlier and the hundred scores tie, while noise large enough to
tell them apart puts points on the threshold (at 96 x 128 always).  With confident outliers a hypothesis is either clean or far off, so about one view
in three has exactly one clean hypothesis, a clear winner with every point far from the threshold.  Cases:
  a  3 views 16 x 24            b  2 views 15 x 21 (N = 315, no multiple of 64)
  c  as a, with target rays whose z is 0, +-1e-4 exactly, +-0.9e-4 and +-1.1e-4, all highly confident
  d  1 view 16 x 24 rotated by 2.2 rad about y: H / H[2,2] has a negative determinant
  e  1 view 96 x 128 whose winner has more than 8000 inliers: the reference's refit draws a random 8000, so it runs under 8 seeds
Per case: ray, conf, sample_idx (captured from get_params_for_ransac), the reference's fp32 R / T / focal / pp / extrinsics / intrinsics / H, its
homography in fp64 (ransac_find_homography_weighted_fast_batch on points normalised in fp64), best, n_inliers, n_used; for e the mean over the seeds
and the largest deviation from it per output (in fp32 and in fp64).

RANSAC is discrete: one borderline point moves a result by 1e-3 while everything else agrees to 1e-6.  A case is kept only if, for every view, the
fp32 and the fp64 evaluation pick the same winner, the winner leads the runner-up by at least 1 % of its score, and no point lies within 1e-3 of the
threshold under the winner in fp64; seeds are drawn until that holds (screened with tests/da3_raypose_ref.py, then asserted on the reference's own
hypotheses) and the number of discarded seeds is printed."""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import da3_raypose_ref as R  # noqa: E402

THRESHOLD = 0.2
NOISE, LOW_OUTLIERS, SURE_OUTLIERS = 0.01, 0.18, 0.12
IMAGE_HW = (280, 504)
E_SEEDS = 8


def rotation(axis, angle):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def make_view(g, ph, pw, rot, focal, pp_terms, t0, z_edits=False):
    """-> ray fp32 [ph,pw,6], conf fp32 [ph,pw]"""
    gx, gy = R.plane_grid(ph, pw)
    N = ph * pw
    p = torch.stack([gx.double().view(1, pw).expand(ph, pw), gy.double().view(ph, 1).expand(ph, pw), torch.ones(ph, pw, dtype=torch.float64)], -1).reshape(N, 3)
    L = torch.tensor([[1 / focal[0], 0, 0], [0, 1 / focal[1], 0], [pp_terms[0], pp_terms[1], 1]], dtype=torch.float64)
    d = p @ (rot @ L).T
    d = d / d.norm(dim=1, keepdim=True)
    d = d + NOISE * torch.randn(N, 3, generator=g, dtype=torch.float64)
    conf = 1 + torch.exp(0.5 * torch.randn(N, generator=g, dtype=torch.float64))
    order = torch.randperm(N, generator=g)
    low, sure = order[:int(LOW_OUTLIERS * N)], order[int(LOW_OUTLIERS * N):int((LOW_OUTLIERS + SURE_OUTLIERS) * N)]
    out = torch.cat([low, sure])
    ang = 2 * math.pi * torch.rand(out.numel(), generator=g, dtype=torch.float64)
    rad = 0.6 + 2.4 * torch.rand(out.numel(), generator=g, dtype=torch.float64)
    uv = d[out, :2] / d[out, 2:3] + rad[:, None] * torch.stack([ang.cos(), ang.sin()], -1)          # an outlier: off by 0.6 to 3 in the normalised plane
    d[out] = torch.cat([uv, torch.ones(out.numel(), 1, dtype=torch.float64)], -1) * d[out, 2:3]
    conf[low] = 1 + 0.1 * torch.rand(low.numel(), generator=g, dtype=torch.float64)
    conf[sure] = conf.max() + 1 + torch.rand(sure.numel(), generator=g, dtype=torch.float64)
    t = torch.tensor(t0, dtype=torch.float64) + 0.05 * torch.randn(N, 3, generator=g, dtype=torch.float64)
    ray, conf = torch.cat([d, t], -1).float(), conf.float()
    if z_edits:                                                 # about ten rays around the z threshold, more confident than every other
        zs = [0.0, 1e-4, -1e-4, 0.9e-4, -0.9e-4, 1.1e-4, -1.1e-4, 0.0, 1e-4, -0.9e-4]
        where = torch.randperm(N, generator=g)[:len(zs)]
        ray[where, 2] = torch.tensor(zs, dtype=torch.float32)
        conf[where] = conf.max() + 1 + torch.arange(len(zs), dtype=torch.float32)
    rank = torch.argsort(conf, stable=True)                     # fp32 rounding makes a few of 12 288 random numbers equal: the later one moves up an ulp
    c = conf[rank]
    for i in range(1, N):
        if c[i] <= c[i - 1]:
            c[i] = torch.nextafter(c[i - 1], torch.tensor(float("inf")))
    conf[rank] = c
    assert conf.unique().numel() == N, "confidences must be distinct"
    return ray.reshape(ph, pw, 6), conf.reshape(ph, pw)


def camera(g, big_rotation=False):
    r = torch.rand(8, generator=g, dtype=torch.float64).tolist()
    rot = rotation([0.05, 1.0, 0.02], 2.2) if big_rotation else rotation([r[0] - 0.5, r[1] - 0.5, r[2] - 0.5], 0.1 + 0.5 * r[3])
    return dict(rot=rot, focal=(0.9 + 0.8 * r[4], 0.9 + 0.8 * r[5]), pp_terms=(0.1 * (r[6] - 0.5), 0.1 * (r[7] - 0.5)), t0=(r[0] - 0.5, r[1] - 0.5, r[2]))


CASES = {"a": (3, 16, 24), "b": (2, 15, 21), "c": (3, 16, 24), "d": (1, 16, 24), "e": (1, 96, 128)}


def make_case_view(name, seed):
    g = torch.Generator().manual_seed(seed)
    _, ph, pw = CASES[name]
    ray, conf = make_view(g, ph, pw, **camera(g, big_rotation=name == "d"), z_edits=name == "c")
    return ray[None, None].contiguous(), conf[None, None].contiguous()


def screen(o64, o32, name):
    """the three conditions (and the case's own) on the restated evaluation -> None, or why not"""
    if not torch.equal(o64["best"], o32["best"]):
        return "fp32 and fp64 pick different winners"
    top = o64["score"].sort(dim=1, descending=True).values
    if bool(((top[:, 0] - top[:, 1]) < 0.01 * top[:, 0]).any()):
        return "the winner leads by less than 1 %"
    if float(o64["margin"].min()) < 1e-3 or float(o32["margin"].min()) < 1e-3:
        return "a point within 1e-3 of the threshold"
    if name == "e" and int(o64["n_inliers"].min()) <= R.MAX_INLIERS:
        return "no more than 8000 inliers"
    if name == "d" and float(torch.linalg.det(o64["H"][0])) >= 0:
        return "determinant not negative"
    return None


def run_reference(ru, geometry, ray, conf, table, seed=0):
    """get_extrinsic_from_camray + da3.py:192-198 in fp32 on clones, with the table fixed and the internals recorded"""
    rec = dict(H_batch=[], refit_n=[], fast_in=[], fast_out=[])
    keep = {k: getattr(ru, k) for k in ("get_params_for_ransac", "find_homography_least_squares_weighted_torch_batch",
                                        "find_homography_least_squares_weighted_torch", "ransac_find_homography_weighted_fast_batch")}

    def params(N, device):
        n_iter, k, n_sample, drawn = keep["get_params_for_ransac"](N, device)
        rec["drawn"] = drawn
        return n_iter, k, n_sample, (drawn if table is None else table)

    def fit_batch(*a):
        H = keep["find_homography_least_squares_weighted_torch_batch"](*a)
        rec["H_batch"].append(H.clone())
        return H

    def fit_one(src, dst, w):
        rec["refit_n"].append(src.shape[0])
        return keep["find_homography_least_squares_weighted_torch"](src, dst, w)

    def fast_batch(src, dst, w, **kw):
        H = keep["ransac_find_homography_weighted_fast_batch"](src, dst, w, **kw)
        rec["fast_in"].append((src.clone(), dst.clone(), w.clone(), dict(kw)))
        rec["fast_out"].append(H.clone())
        return H
    ru.get_params_for_ransac, ru.find_homography_least_squares_weighted_torch_batch = params, fit_batch
    ru.find_homography_least_squares_weighted_torch, ru.ransac_find_homography_weighted_fast_batch = fit_one, fast_batch
    try:
        torch.manual_seed(seed)
        r, c = ray.clone(), conf.clone()
        ext44, focal, pp = ru.get_extrinsic_from_camray(r, c, r.shape[-3], r.shape[-2])
    finally:
        for k, f in keep.items():
            setattr(ru, k, f)
    Himg, Wimg = IMAGE_HW
    ext = geometry.affine_inverse(ext44)[:, :, :3, :]
    K = torch.eye(3)[None, None].repeat(ext.shape[0], ext.shape[1], 1, 1).clone()
    K[:, :, 0, 0], K[:, :, 1, 1] = focal[:, :, 0] / 2 * Wimg, focal[:, :, 1] / 2 * Himg
    K[:, :, 0, 2], K[:, :, 1, 2] = pp[:, :, 0] * Wimg * 0.5, pp[:, :, 1] * Himg * 0.5
    out = dict(R=ext44[0, :, :3, :3], T=ext44[0, :, :3, 3], focal=focal[0], pp=pp[0], extrinsics=ext[0], intrinsics=K[0], H=torch.cat(rec["fast_out"]))
    return {k: v.clone() for k, v in out.items()}, rec, c


def reference_h64(ru, ray, conf, table, seed=0):
    """ransac_find_homography_weighted_fast_batch in fp64 on points normalised in fp64 from the fp32 inputs -> H [V,3,3] and the hypotheses [V,100,3,3]"""
    x, y, u, v, w, _ = R.normalise(ray.flatten(0, 1), conf.flatten(0, 1), torch.float64)
    got = []
    keep = ru.find_homography_least_squares_weighted_torch_batch

    def fit_batch(*a):
        got.append(keep(*a))
        return got[-1]
    ru.find_homography_least_squares_weighted_torch_batch = fit_batch
    try:
        torch.manual_seed(seed)
        H = ru.ransac_find_homography_weighted_fast_batch(torch.stack([x, y], -1), torch.stack([u, v], -1), w, n_sample=max(8, int(x.shape[1] * 0.3)),
                                                          n_iter=100, num_sample_for_ransac=8, reproj_threshold=THRESHOLD, rand_sample_iters_idx=table,
                                                          max_inlier_num=8000)
    finally:
        ru.find_homography_least_squares_weighted_torch_batch = keep
    return H, got[0].reshape(x.shape[0], -1, 3, 3)


def main(ref_root):
    sys.path.insert(0, ref_root)
    from depth_anything_3.utils import geometry, ray_utils as ru
    fixture, discarded, seed = {"image_hw": IMAGE_HW, "threshold": THRESHOLD}, 0, 1000
    for name in "abcde":
        views, ph, pw = CASES[name]
        N = ph * pw
        seed += 1
        torch.manual_seed(seed)
        table = ru.get_params_for_ransac(N, torch.device("cpu"))[3]
        kept = []
        while len(kept) < views:                                # one table per case, as upstream; every view is screened on its own against it
            seed += 1
            ray, conf = make_case_view(name, seed)
            try:
                o64 = R.ray_pose(ray, conf, IMAGE_HW, table, THRESHOLD, torch.float64, torch.Generator().manual_seed(0))
                o32 = R.ray_pose(ray, conf, IMAGE_HW, table, THRESHOLD, torch.float32, torch.Generator().manual_seed(0))
                why = screen(o64, o32, name)
            except ValueError as e:
                why = str(e)
            if why is None:
                kept.append((ray, conf))
            else:
                discarded += 1
                print(f"case {name}: seed {seed} discarded ({why})")
        ray, conf = torch.cat([k[0] for k in kept], dim=1).contiguous(), torch.cat([k[1] for k in kept], dim=1).contiguous()
        o64 = R.ray_pose(ray, conf, IMAGE_HW, table, THRESHOLD, torch.float64, torch.Generator().manual_seed(0))
        # the table is get_params_for_ransac's own draw under the case's seed; the hook hands the same one to every later run
        ref, rec, c_after = run_reference(ru, geometry, ray, conf, table)
        assert rec["drawn"].shape == table.shape and int(rec["drawn"].max()) < max(8, int(N * 0.3))
        V = ray.shape[1]
        # the reference's own hypotheses, scored: same winner in fp32 and fp64, 1 % lead, no borderline point
        x, y, u, v, w, wm = R.normalise(ray.flatten(0, 1), conf.flatten(0, 1), torch.float64)
        H64, hyp64 = reference_h64(ru, ray, conf, table)
        hyp32 = torch.cat(rec["H_batch"]).reshape(V, -1, 3, 3)
        s64, inl64 = R.scores(hyp64, x, y, u, v, w, THRESHOLD)
        s32, _ = R.scores(hyp32, *(t.float() for t in (x, y, u, v, w)), THRESHOLD)
        best = s64.argmax(dim=1)
        assert torch.equal(best, s32.argmax(dim=1)) and torch.equal(best, o64["best"]), (best, s32.argmax(dim=1), o64["best"])
        top = s64.sort(dim=1, descending=True).values
        assert bool(((top[:, 0] - top[:, 1]) >= 0.01 * top[:, 0]).all())
        err = R.reprojection_error(hyp64[torch.arange(V), best][:, None], x, y, u, v)[:, 0]
        assert float((err - THRESHOLD).abs().min()) >= 1e-3
        n_inl = inl64[torch.arange(V), best].sum(dim=1)
        assert torch.equal(n_inl, o64["n_inliers"])
        n_used = torch.tensor(rec["refit_n"])
        assert torch.equal(n_used, n_inl.clamp(max=R.MAX_INLIERS)), (n_used, n_inl)
        assert torch.equal(c_after.flatten(0, 1).flatten(1), wm), "the reference zeroes the masked confidences in place"
        if name == "c":
            assert int((wm == 0).sum()) >= 8 * V
        if name == "d":
            assert float(torch.linalg.det(ref["H"][0])) < 0 and float(torch.linalg.det(H64[0])) < 0, "the reference must take the det < 0 branch"
        case = dict(ray=ray, conf=conf, sample_idx=table.to(torch.int32), best=best.to(torch.int32), n_inliers=n_inl.to(torch.int32),
                    n_used=n_used.to(torch.int32), H64=H64, **{f"{k}32": t for k, t in ref.items()})
        if name == "e":
            assert int(n_inl.min()) > R.MAX_INLIERS, "case e needs more than 8000 inliers on the winner"
            runs32 = [ref] + [run_reference(ru, geometry, ray, conf, table, seed=s)[0] for s in range(1, E_SEEDS)]
            runs64 = [H64] + [reference_h64(ru, ray, conf, table, seed=s)[0] for s in range(1, E_SEEDS)]
            for k in runs32[0]:
                stack = torch.stack([r[k] for r in runs32]).double()
                case[f"{k}32"] = stack.mean(0).float()
                case[f"{k}32_dev"] = float((stack - stack.mean(0)).abs().max())
            stack = torch.stack(runs64)
            case["H64"], case["H64_dev"] = stack.mean(0), float((stack - stack.mean(0)).abs().max())
            assert case["H32_dev"] > 0, "the seeds must draw different subsets"
        fixture[name] = case
        print(f"case {name}: seed {seed}, best {best.tolist()}, inliers {n_inl.tolist()} of {N}, used {n_used.tolist()}, "
              f"lead {((top[:, 0] - top[:, 1]) / top[:, 0]).tolist()}")
    print(f"{discarded} seeds discarded")
    path = os.path.join(HERE, "da3_raypose.pt")
    torch.save(fixture, path)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20), "fixtures stay below 1 MiB"


if __name__ == "__main__":
    main(sys.argv[1])
