"""Depth Anything 3's ray-based cameras on the device (ops.da3_ray_pose on csrc/da3_ray_pose.hip, `use_ray_pose=True`).  -m gpu only.

The inputs and the reference's results are tests/golden/da3_raypose.pt (make_golden_raypose.py); the fp64 oracle is tests/da3_raypose_ref.py on the
CPU, computed once per case and shared with tests/test_da3_raypose_host.py.

Bound.  For each output kind (H, R, T, focal, pp, extrinsics, intrinsics) d_ref is the largest distance over the case's views between the
reference's stored fp32 result and the fp64 oracle; the device must be within 2 x d_ref of the oracle, and the bound is never below 4 fp32 ulps of
the output's largest magnitude.  The device reads the same fp32 inputs and orders its sums differently: that is the factor 2.  A flipped inlier moves
a result by about 1e-3 and fails.  The winner and the inlier counts are exact.  Case e (more than 8000 inliers: a random 8000 are refitted) adds 3 x
the reference's stored seed-to-seed deviation from its own mean over 8 seeds, and is measured against the oracle's mean over 8 seeds.  Every figure is
printed before it is asserted and written to da3_ray_pose_parity.json in $VGPA_REPORT_DIR (or the test's temporary directory);
profiles/da3_ray_pose_parity.json is a copy of one run on an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

import da3_raypose_ref as R

pytestmark = pytest.mark.gpu
_REPORT = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops
    return ops


@pytest.fixture(scope="module")
def report_dir(tmp_path_factory):
    return os.environ.get("VGPA_REPORT_DIR") or str(tmp_path_factory.mktemp("da3_ray_pose"))


def run_case(ops, name, generator=None, threshold=None):
    fx = R.fixture()
    c = fx[name]
    ray, conf = c["ray"].cuda(), c["conf"].cuda()
    ext, intr, info = ops.da3_ray_pose(ray, conf, fx["image_hw"], sample_idx=c["sample_idx"], generator=generator,
                                       reproj_threshold=fx["threshold"] if threshold is None else threshold)
    assert torch.equal(ray.cpu(), c["ray"]) and torch.equal(conf.cpu(), c["conf"]), "the inputs must not be written"
    V = c["ray"].shape[1]
    assert ext.shape == (1, V, 3, 4) and intr.shape == (1, V, 3, 3) and ext.dtype == intr.dtype == torch.float32
    return dict(info, extrinsics=ext, intrinsics=intr)


def check_outputs(name, got, report_dir):
    """every output of a case against the oracle: prints and records distance, d_ref and bound, then asserts"""
    o, rows = R.oracle(name), {}
    for k, (bound, d_ref) in R.bounds(name).items():
        d = R.distance(got[k][0], o[k])
        rows[k] = {"device": d, "d_ref": d_ref, "bound": bound}
        print(f"case {name} {k}: device {d:.3e} d_ref {d_ref:.3e} bound {bound:.3e}")
    _REPORT[name] = rows
    with open(os.path.join(report_dir, "da3_ray_pose_parity.json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "distance": "largest absolute difference from the fp64 oracle over the case's views",
                   "cases": _REPORT}, f, indent=1, sort_keys=True)
    for k, r in rows.items():
        assert np.isfinite(r["device"]) and r["device"] <= r["bound"], (name, k, r)


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_fixture_cases(ops, report_dir, name):
    c, got = R.fixture()[name], run_case(ops, name)
    for k in ("best", "n_inliers", "n_used"):
        print(f"case {name} {k}: device {got[k][0].tolist()} reference {c[k].tolist()}")
        assert torch.equal(got[k][0].cpu(), c[k]), k
    check_outputs(name, got, report_dir)


def test_more_than_8000_inliers(ops, report_dir):
    c = R.fixture()["e"]
    gen = lambda seed: torch.Generator(device="cuda").manual_seed(seed)
    got = run_case(ops, "e", generator=gen(1))
    assert torch.equal(got["best"][0].cpu(), c["best"]) and torch.equal(got["n_inliers"][0].cpu(), c["n_inliers"])
    assert got["n_used"].tolist() == [[R.MAX_INLIERS]]
    check_outputs("e", got, report_dir)
    again, other = run_case(ops, "e", generator=gen(1)), run_case(ops, "e", generator=gen(2))
    for k in R.OUTPUTS:
        assert torch.equal(got[k], again[k]), k
    assert not torch.equal(got["H"], other["H"]) and other["n_used"].tolist() == [[R.MAX_INLIERS]]
    host = run_case(ops, "e", generator=torch.Generator().manual_seed(1))       # a host generator draws on the host
    assert host["n_used"].tolist() == [[R.MAX_INLIERS]] and R.distance(host["H"], got["H"]) <= 2 * (3 * c["H32_dev"])


def test_two_runs_are_bit_identical(ops):
    one, two = run_case(ops, "a"), run_case(ops, "a")
    for k in R.OUTPUTS + ("best", "n_inliers", "n_used"):
        assert torch.equal(one[k], two[k]), k


def test_too_few_inliers_raise(ops):
    with pytest.raises(ValueError, match="At least 4 points"):
        run_case(ops, "a", threshold=1e-12)


def test_drawn_sample_table(ops):
    c = R.fixture()["b"]
    ray, conf, hw = c["ray"].cuda(), c["conf"].cuda(), R.fixture()["image_hw"]
    n_sample = max(8, int(15 * 21 * 0.3))
    draw = lambda seed: ops.da3_ray_pose(ray, conf, hw, generator=torch.Generator(device="cuda").manual_seed(seed))[2]["sample_idx"]
    t = draw(3)
    assert t.shape == (100, 8) and t.dtype == torch.int32 and t.is_cuda and int(t.min()) >= 0 and int(t.max()) < n_sample
    assert all(len(set(row)) == 8 for row in t.tolist())
    assert torch.equal(t, draw(3)) and not torch.equal(t, draw(4))
    assert torch.equal(t, ops.da3_ray_sample_table(n_sample, torch.Generator(device="cuda").manual_seed(3), ray.device))


def test_refusals(ops):
    c = R.fixture()["a"]
    ray, conf, hw = c["ray"].cuda(), c["conf"].cuda(), R.fixture()["image_hw"]
    for bad in (dict(ray=ray[..., :5].contiguous()), dict(conf=conf[:, :2].contiguous()), dict(ray=ray.double()), dict(sample_idx=c["sample_idx"][:, :7]),
                dict(sample_idx=c["sample_idx"].float()), dict(sample_idx=c["sample_idx"].repeat(2, 1))):
        kw = dict(dict(ray=ray, conf=conf, sample_idx=c["sample_idx"]), **bad)
        with pytest.raises(RuntimeError):
            ops.da3_ray_pose(kw["ray"], kw["conf"], hw, sample_idx=kw["sample_idx"])
    bad = c["sample_idx"].clone()
    bad[:, 0] = 10 ** 6                                         # a position outside the candidates: no hypothesis fits, nothing is read out of bounds
    with pytest.raises(ValueError, match="At least 4 points"):
        ops.da3_ray_pose(ray, conf, hw, sample_idx=bad)


def test_network_and_api_wiring(ops):
    import da3_ref as D
    from test_gpu_dualdpt import small_net
    from videogpa_amd.da3 import DepthAnything3
    net = small_net()
    gen = lambda: torch.Generator(device="cuda").manual_seed(7)
    x = None
    for seed in (100, 101, 102, 103, 104, 105):                # random weights: the first clip whose every view keeps 4 inliers
        cand = D.images(seed, 1, 4, (42, 56)).cuda()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            full = net(cand, aux=True)
        try:
            want = ops.da3_ray_pose(full.ray, full.ray_conf, (42, 56), generator=gen())
        except ValueError:
            continue
        x = cand
        break
    assert x is not None and int(want[2]["n_inliers"].min()) >= 4, "no seed leaves every view 4 inliers"
    print(f"wiring: images seed {seed}, inliers {want[2]['n_inliers'].tolist()} of {24 * 32}")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = net(x, use_ray_pose=True, aux=False, ray_pose_generator=gen())       # the auxiliary branch runs whatever `aux` says
    assert torch.equal(out.extrinsics, want[0]) and torch.equal(out.intrinsics, want[1]) and out.extrinsics.shape == (1, 4, 3, 4)
    assert torch.equal(out.ray, full.ray) and torch.equal(out.ray_conf, full.ray_conf) and torch.equal(out.depth, full.depth)
    assert not torch.equal(out.extrinsics, full.extrinsics) and not torch.equal(out.intrinsics, full.intrinsics)      # `full` holds cam_dec's cameras

    frames = (torch.rand(4, 40, 60, 3, generator=torch.Generator().manual_seed(11)) * 255).to(torch.uint8)
    plain = DepthAnything3(model=net, process_res=42)
    bare, off = plain.inference(frames), plain.inference(frames, use_ray_pose=False)
    for k in ("depth", "conf", "extrinsics", "intrinsics", "processed_images"):
        assert torch.equal(getattr(bare, k), getattr(off, k)), k
    try:
        api = DepthAnything3(model=net, process_res=42, use_ray_pose=True, ray_pose_generator=gen())
        pred = api.inference(frames)                           # the instance's default reaches a bare call, as VideoProcessor makes it
    except ValueError:
        pytest.fail("the API clip leaves a view fewer than 4 inliers: pick other frames")
    x_api = plain.input_processor(plain._get_model_device()).process(frames, None, None, 42, "upper_bound_resize")[0]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        aux = net(x_api, aux=True)
    ext, intr, _ = ops.da3_ray_pose(aux.ray, aux.ray_conf, x_api.shape[-2:], generator=gen())
    assert torch.equal(pred.extrinsics, ext[0]) and torch.equal(pred.intrinsics, intr[0]) and pred.extrinsics.shape == (4, 3, 4)
    assert torch.equal(pred.depth, bare.depth) and torch.equal(pred.conf, bare.conf) and not torch.equal(pred.extrinsics, bare.extrinsics)
    torch.cuda.manual_seed(7)
    named = plain.inference(frames, use_ray_pose=True)          # the argument overrides the instance's default, here with the default generator
    assert named.extrinsics.shape == (4, 3, 4) and bool(torch.isfinite(named.intrinsics).all())
