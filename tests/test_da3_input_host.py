"""Depth Anything 3's input processing without a GPU (videogpa_amd/da3_input.py): `plan` and the intrinsics transforms against what the reference's own
InputProcessor does (tests/golden/da3_input_plan.json, written by tests/golden/make_golden_da3_input.py from the reference with cv2 stubbed), the
`processed_images` table against api.py's numpy expression, the area oracle's weight sums, and what is refused."""
import json
import os

import numpy as np
import pytest
import torch

import da3_input_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "da3_input_plan.json")))
SIZES = [(480, 720), (768, 1360), (704, 1280), (720, 480), (518, 518), (504, 376), (200, 300)]
METHODS = ["upper_bound_resize", "upper_bound_crop", "lower_bound_resize", "lower_bound_crop"]


def test_fixture_covers_every_size_method_and_intrinsics_choice():
    seen = {(r["H"], r["W"], r["method"], r["K_in"] is not None) for r in GOLDEN["rows"]}
    assert seen == {(h, w, m, k) for h, w in SIZES for m in METHODS for k in (False, True)} and len(GOLDEN["rows"]) == 56


@pytest.mark.parametrize("row", GOLDEN["rows"], ids=lambda r: f"{r['H']}x{r['W']}-{r['method']}-{'K' if r['K_in'] else 'noK'}")
def test_plan_and_intrinsics_are_the_reference_s(row):
    from videogpa_amd import da3_input as di
    stages, size = di.plan(row["H"], row["W"], row["process_res"], row["method"])
    assert [list(s) for s in stages] == row["stages"] and list(size) == row["size"]
    ops, rsize, _ = R.process_one(row["H"], row["W"], None, row["process_res"], row["method"])          # the tests' own restatement, pinned the same way
    assert [list(s) for s in ops] == row["stages"] and list(rsize) == row["size"]
    if row["K_in"] is not None:
        K = np.array(row["K_in"], np.float32)
        got = di.plan_ixt(K, row["H"], row["W"], stages)
        want = np.array(row["K_out"], np.float32)
        assert got.dtype == np.float32 and np.array_equal(got, want), (got, want)
        assert np.array_equal(R.process_one(row["H"], row["W"], K, row["process_res"], row["method"])[2], want)
        assert np.array_equal(K, np.array(row["K_in"], np.float32))                                        # the caller's array is left alone


def test_expected_plan_rows():
    from videogpa_amd import da3_input as di
    assert di.plan(480, 720) == ([("area", 336, 504)], (336, 504))
    assert di.plan(704, 1280, 504, "upper_bound_resize") == ([("area", 277, 504), ("cubic", 280, 504)], (280, 504))
    assert di.plan(768, 1360) == ([("area", 285, 504), ("area", 280, 504)], (280, 504))
    assert di.plan(504, 376, 504, "upper_bound_crop") == ([("crop", 0, 6, 504, 364)], (504, 364))
    assert di.plan(336, 504) == ([], (336, 504))                                       # nothing to do: the last stage alone
    for stages, (h, w) in (di.plan(H, W, 504, m) for H, W in SIZES for m in METHODS):
        assert h % 14 == 0 and w % 14 == 0
        for s in stages:                                                               # area is only ever planned when neither axis grows
            assert s[0] in ("area", "cubic", "crop")
    with pytest.raises(ValueError, match="Unsupported process_res_method"):
        di.plan(480, 720, 504, "resize")
    with pytest.raises(ValueError, match="smaller than one"):
        di.plan(480, 720, 13, "upper_bound_crop")


def test_area_is_never_planned_for_a_growing_axis():
    from videogpa_amd import da3_input as di
    for H in range(20, 900, 61):
        for W in range(24, 1500, 97):
            for m in METHODS:
                for res in (56, 504):
                    h, w = H, W
                    if m.endswith("crop") and min(H, W) * res < 14 * (max(H, W) if m.startswith("upper") else min(H, W)):
                        continue                                           # thinner than one patch after the boundary resize: refused, see above
                    for s in di.plan(H, W, res, m)[0]:
                        if s[0] == "area":
                            assert s[1] <= h and s[2] <= w, (H, W, m, res, s)
                        h, w = (s[1], s[2]) if s[0] != "crop" else (s[3], s[4])


@pytest.mark.parametrize("b", GOLDEN["batches"], ids=lambda b: f"{len(b['sizes'])}-{b['sizes'][0][0]}-{b['method']}")
def test_unified_batches_are_the_reference_s(b):
    """mixed sizes: `_unify_batch_shapes` centre-crops to the smallest and moves the principal points; InputProcessor's host side alone (no device:
    the launches are replaced by shape-only stand-ins)"""
    from videogpa_amd import da3_input as di
    Ks = np.array(b["K_in"], np.float32)
    plans = [di.plan(h, w, b["process_res"], b["method"]) for h, w in b["sizes"]]
    mh, mw = min(p[1][0] for p in plans), min(p[1][1] for p in plans)
    assert [mh, mw] == b["size"]
    got = []
    for (H, W), (stages, (h, w)), K in zip(b["sizes"], plans, Ks):
        if (h, w) != (mh, mw):
            stages = stages + [("crop", (h - mh) // 2, (w - mw) // 2, mh, mw)]
        got.append(di.plan_ixt(K, H, W, stages))
    assert np.array_equal(np.asarray(got), np.array(b["K_out"], np.float32))
    sizes, ks = zip(*[R.process_one(h, w, K, b["process_res"], b["method"])[1:] for (h, w), K in zip(b["sizes"], Ks)])
    _, rsize, rk = R.unify(list(sizes), list(ks))
    assert list(rsize) == b["size"] and np.array_equal(np.asarray(rk), np.array(b["K_out"], np.float32))


def test_processed_images_table_is_the_numpy_expression():
    from videogpa_amd import da3_input as di
    table = di.processed_table()
    assert table.shape == (3, 256) and table.dtype == np.uint8
    u = np.arange(256, dtype=np.uint8)
    img = np.stack([u, u, u], axis=-1)[None, None]                       # [1,1,256,3]: every byte in every channel
    want = R.processed_images(R.normalize(img))[0, 0]                    # [256,3]
    assert np.array_equal(table, want.T)
    off = int((table != u[None, :]).sum())
    print(f"processed_images table: {off} of 768 entries differ from the byte they came from")
    assert off > 0 and int(np.abs(table.astype(int) - u[None, :].astype(int)).max()) == 1     # "not always u": truncation of 254.99999...


SHAPES = [((40, 60), (28, 42)), ((37, 53), (28, 42)), ((56, 90), (28, 42)), ((30, 42), (28, 42)), ((56, 84), (28, 42)), ((84, 126), (28, 42)),
          ((480, 720), (336, 504)), ((704, 1280), (277, 504))]


@pytest.mark.parametrize("src,dst", SHAPES)
def test_area_oracle_weights_sum_to_one(src, dst):
    for n_in, n_out in zip(src, dst):
        M = R.area_matrix(n_in, n_out)
        assert float(np.abs(M.sum(axis=1) - 1.0).max()) < 1e-12 and (M >= 0).all()


def test_cubic_oracles_agree_on_the_identity_and_partition_unity():
    img = R.frames(2, 9, 11, seed=3)
    assert np.array_equal(R.cubic_fixed(img, 9, 11), img) and np.allclose(R.cubic_exact(img, 9, 11), img, atol=1e-9)
    for n_in, n_out in ((27, 28), (50, 50), (20, 28), (31, 42)):
        assert float(np.abs(R.cubic_matrix(n_in, n_out).sum(axis=1) - 1.0).max()) < 1e-12
        _, w = R.cubic_fixed_table(n_in, n_out)
        assert int(np.abs(w.sum(axis=1) - 2048).max()) <= 2              # not re-normalised: four roundings


def test_input_processor_refuses_paths_and_wrong_frames_and_needs_a_device():
    from videogpa_amd import da3_input as di
    from videogpa_amd.da3 import DepthAnything3
    from test_dualdpt_host import small_net
    proc = di.InputProcessor(device="cpu")
    with pytest.raises(TypeError, match="decoded frames"):
        proc(["clip/frame0.png"])
    with pytest.raises(TypeError, match="decoded frames"):
        proc("clip.mp4")
    with pytest.raises(ValueError, match="uint8 frames"):
        proc([np.zeros((40, 60, 3), np.float32)])
    with pytest.raises(ValueError, match="Length of intrinsics"):
        proc(np.zeros((2, 40, 60, 3), np.uint8), intrinsics=np.zeros((3, 3, 3)))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            proc(np.zeros((2, 40, 60, 3), np.uint8), process_res=42)
    api = DepthAnything3(model=small_net())
    frames = [np.zeros((40, 60, 3), np.uint8)] * 2
    for kw, msg in ((dict(extrinsics=np.zeros((2, 4, 4))), "cam_enc"), (dict(intrinsics=np.zeros((2, 3, 3))), "cam_enc"), (dict(infer_gs=True), "infer_gs"),
                    (dict(use_ray_pose=True), "use_ray_pose"), (dict(export_dir="out"), "export"), (dict(export_feat_layers=[1]), "export_feat_layers")):
        with pytest.raises(NotImplementedError, match=msg):
            api.inference(frames, **kw)
    with pytest.raises(ValueError, match="unknown preset"):
        DepthAnything3("da3-giant")


def test_video_processor_dispatches_on_inference_and_points_at_the_api_class():
    from videogpa_amd.process_video import VideoProcessor
    seen = []

    class Api:
        def inference(self, frames):
            seen.append(frames)
            return "prediction"
    vp = VideoProcessor({}, backbone="da3", da3_model=Api(), device="cpu")
    clip = np.zeros((3, 40, 60, 3), np.uint8)
    assert vp.backbone_fn(clip) == "prediction" and isinstance(seen[0], list) and len(seen[0]) == 3 and seen[0][0].shape == (40, 60, 3)
    bare = VideoProcessor({}, backbone="da3", da3_model=lambda x, aux: None, device="cpu")
    with pytest.raises(ValueError, match="multiples of 14.*DepthAnything3"):
        bare._run_da3(None, torch.zeros(3, 40, 60, 3, dtype=torch.uint8))
