"""Depth Anything 3's ray-based cameras without a GPU: the restatement of tests/da3_raypose_ref.py against the reference's results in
tests/golden/da3_raypose.pt (make_golden_raypose.py: get_extrinsic_from_camray and ransac_find_homography_weighted_fast_batch on the CPU), the
fixture's own premises, the sample table, and what the package refuses without a device.

Bounds.  (1) fp64 against fp64: the restated homography is the eigenvector of the normal matrix where the reference takes the singular vector of the
DLT matrix itself; both are float64, so they differ by about eps64 * cond^2 = 2e-16 * 1e6: 1e-8 of the largest entry.  (2) The reference's fp32
results against the fp64 oracle: its SVD leaves eps32 * cond = 1.2e-7 * 1e3 = 1.2e-4 of the largest entry in the singular vector at the most; a
flipped inlier moves a result by about 1e-3.  The bound is 2.5e-4 of the output's largest magnitude, which separates the two; this distance is the
d_ref of tests/test_gpu_da3_raypose.py and is printed per case and output."""
import pytest
import torch

import da3_raypose_ref as R

CASES = {"a": (3, 16, 24), "b": (2, 15, 21), "c": (3, 16, 24), "d": (1, 16, 24), "e": (1, 96, 128)}
SVD_FP32 = 2.5e-4


def test_fixture_is_what_the_tests_assume():
    fx = R.fixture()
    assert fx["threshold"] == 0.2 and set(CASES) <= set(fx)
    for name, (V, ph, pw) in CASES.items():
        c = fx[name]
        assert c["ray"].shape == (1, V, ph, pw, 6) and c["conf"].shape == (1, V, ph, pw) and c["ray"].dtype == c["conf"].dtype == torch.float32
        assert c["sample_idx"].shape == (100, 8) and int(c["sample_idx"].max()) < max(8, int(ph * pw * 0.3)) and int(c["sample_idx"].min()) >= 0
        assert all(len(set(row)) == 8 for row in c["sample_idx"].tolist())
        assert all(c["conf"][0, v].unique().numel() == ph * pw for v in range(V)), "ties would make the candidate order a convention"
    assert (15 * 21) % 64 != 0
    z = fx["c"]["ray"][0, :, :, :, 2].flatten()
    thr = torch.tensor(1e-4, dtype=torch.float32)
    for want in (0.0, thr, -thr, 0.9e-4, -0.9e-4):
        assert bool((z == want).any()), want
    assert float(torch.linalg.det(fx["d"]["H32"][0].double())) < 0 and float(torch.linalg.det(fx["d"]["H64"][0])) < 0
    assert int(fx["e"]["n_inliers"][0]) > R.MAX_INLIERS and int(fx["e"]["n_used"][0]) == R.MAX_INLIERS and fx["e"]["H32_dev"] > 0


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_the_reference(name):
    fx = R.fixture()
    c, o = fx[name], R.oracle(name)
    assert torch.equal(o["best"].int(), c["best"]) and torch.equal(o["n_inliers"].int(), c["n_inliers"]) and torch.equal(o["n_used"].int(), c["n_used"])
    top = o["score"].sort(dim=1, descending=True).values
    assert bool(((top[:, 0] - top[:, 1]) >= 0.01 * top[:, 0]).all()) and float(o["margin"].min()) >= 1e-3        # the generator's screening, seen from here
    scale = float(c["H64"].abs().max())
    d64 = R.distance(o["H"], c["H64"])
    room = 3 * c["H64_dev"] if name == "e" else 0.0            # case e: one more draw of the 8000 on each side
    print(f"case {name}: |H - H64| {d64:.3e} of {scale:.3g}")
    assert d64 <= 1e-8 * scale + room
    for k, (b, d_ref) in R.bounds(name).items():
        mag = float(o[k].abs().max())
        print(f"case {name} {k}: d_ref {d_ref:.3e} of {mag:.3g} (bound for the device {b:.3e})")
        assert d_ref <= SVD_FP32 * max(mag, 1.0) + (3 * c[f"{k}32_dev"] if name == "e" else 0.0), (name, k, d_ref)


def test_masked_confidences_reach_the_translation_and_the_inputs_stay():
    """case c: its most confident rays sit on the z threshold and lose their confidence; with them T is somewhere else"""
    fx = R.fixture()
    c, o = fx["c"], R.oracle("c")
    ray, conf = c["ray"].clone(), c["conf"].clone()
    R.ray_pose(ray, conf, fx["image_hw"], c["sample_idx"], fx["threshold"])
    assert torch.equal(ray, c["ray"]) and torch.equal(conf, c["conf"])
    w = c["conf"].flatten(0, 1).flatten(1).double()
    unmasked = (c["ray"].flatten(0, 1).flatten(1, 2)[..., 3:].double() * w[..., None]).sum(1) / w.sum(1, keepdim=True)
    assert R.distance(o["T"], c["T32"]) < 1e-5 < 1e-3 < R.distance(unmasked, c["T32"])


def test_sample_table():
    from videogpa_amd import ops
    g = torch.Generator().manual_seed(5)
    t = ops.da3_ray_sample_table(115, g, "cpu")
    assert t.shape == (100, 8) and t.dtype == torch.int32 and int(t.min()) >= 0 and int(t.max()) < 115
    assert all(len(set(row)) == 8 for row in t.tolist())
    assert torch.equal(t, ops.da3_ray_sample_table(115, torch.Generator().manual_seed(5), "cpu"))
    assert not torch.equal(t, ops.da3_ray_sample_table(115, torch.Generator().manual_seed(6), "cpu"))
    assert len(set(ops.da3_ray_sample_table(8, g, "cpu")[0].tolist())) == 8
    with pytest.raises(ValueError, match="n_sample >= 8"):
        ops.da3_ray_sample_table(7, g, "cpu")
    gx, gy = ops.da3_ray_grid(15, 21)
    rx, ry = R.plane_grid(15, 21)
    assert torch.equal(gx, rx) and torch.equal(gy, ry) and gx.shape == (21,) and float(gx.abs().max()) < 1 and abs(float(gx[0]) + 1 - 1 / 21) < 1e-6


def test_no_cpu_fallback():
    from test_dualdpt_host import small_net
    from videogpa_amd import ops
    from videogpa_amd.da3 import DepthAnything3
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.da3_ray_pose(torch.zeros(1, 2, 4, 4, 6), torch.ones(1, 2, 4, 4), (28, 28))
    api = DepthAnything3(model=small_net(), use_ray_pose=True)          # the instance's default reaches a bare inference(frames)
    assert api.use_ray_pose and api.ray_pose_generator is None and not DepthAnything3(model=small_net()).use_ray_pose
    frames = [torch.zeros(40, 60, 3, dtype=torch.uint8).numpy()] * 2
    with pytest.raises(NotImplementedError, match="use_ray_pose.*no CPU fallback"):
        api.inference(frames)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="use_ray_pose.*no CPU fallback"):
        api.model(torch.zeros(1, 2, 3, 42, 56), use_ray_pose=True)
