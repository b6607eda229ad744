"""SuperPoint, the part that needs no GPU: the oracle's own consistency, the size arithmetic, names and weight files, the gray table, the loud errors."""
import os

import numpy as np
import pytest
import torch

import superpoint_ref as R


@pytest.mark.parametrize("radius", [2, 4])
def test_oracle_nms_against_brute_force(radius):
    """the torch simple_nms of the oracle against explicit window loops, on a map with plateaus and ties (values on a grid of 8 levels)"""
    g = torch.Generator().manual_seed(radius)
    s = (torch.rand(23, 31, generator=g) * 8).floor() / 8 + 0.125
    s[5:9, 5:20] = 1.0                                                   # a plateau wider than the window
    for dt in (torch.float32, torch.float64):
        got = R.simple_nms(s.to(dt)[None], radius)[0].numpy()
        assert np.array_equal(got, R.nms_brute(s.to(dt).numpy(), radius))
    assert (got > 0).sum() > 10


def test_oracle_cut_is_stable_and_row_major_otherwise():
    img = torch.zeros(6, 8)
    img[1, 2] = img[4, 1] = img[2, 5] = 0.5
    img[3, 3] = 0.9
    kp, sc = R.select(img, 0.1, None)
    assert kp.tolist() == [[2, 1], [5, 2], [3, 3], [1, 4]]
    kp, sc = R.select(img, 0.1, 3)
    assert kp.tolist() == [[3, 3], [2, 1], [5, 2]] and sc.tolist() == [pytest.approx(0.9), 0.5, 0.5]
    assert R.select(img, 0.1, 4)[0].tolist() == R.select(img, 0.1, None)[0].tolist() == R.select(img, 0.1, 9)[0].tolist()


def test_side_to_image_size():
    from videogpa_amd.superpoint import side_to_image_size
    assert side_to_image_size((480, 720), 1024) == (682, 1024)
    assert side_to_image_size((720, 480), 1024) == (1024, 682)
    assert side_to_image_size((48, 72), 96) == (64, 96)
    assert side_to_image_size((48, 72), 60) == (40, 60)
    assert side_to_image_size((100, 100), 64) == (64, 64)
    assert side_to_image_size((480, 720), 512, "short") == (512, 768)
    assert side_to_image_size((480, 720), 512, "vert") == (512, 768) and side_to_image_size((480, 720), 512, "horz") == (341, 512)
    for h in range(17, 400, 29):
        for w in range(19, 500, 31):
            assert side_to_image_size((h, w), 320) == R.side_to_image_size(h, w, 320)


def test_state_dict_names_and_from_pretrained_round_trip(tmp_path):
    from videogpa_amd.superpoint import SuperPoint, WEIGHT_FILES
    net = SuperPoint(pretrained=False)
    assert list(net.state_dict()) == R.NAMES
    sd = R.state(3)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    torch.save(sd, tmp_path / WEIGHT_FILES[0])
    for src in (tmp_path, tmp_path / WEIGHT_FILES[0]):
        got = SuperPoint.from_pretrained(src, max_num_keypoints=2048)
        assert all(torch.equal(got.state_dict()[k], sd[k]) for k in sd) and got.conf["max_num_keypoints"] == 2048
        assert not any(p.requires_grad for p in got.parameters()) and not got.training
    os.remove(tmp_path / WEIGHT_FILES[0])
    with pytest.raises(FileNotFoundError, match="local files only"):
        SuperPoint.from_pretrained(tmp_path)
    from safetensors.torch import save_file
    save_file(sd, str(tmp_path / WEIGHT_FILES[1]))
    got = SuperPoint.from_pretrained(tmp_path)
    assert all(torch.equal(got.state_dict()[k], sd[k]) for k in sd)
    a, b = SuperPoint(pretrained=False), SuperPoint(pretrained=False)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))          # the seeded init


def test_gray_table_and_constants():
    from videogpa_amd import ops
    want = torch.from_numpy(np.arange(256, dtype=np.uint8) / 255.0).float()
    assert torch.equal(ops.sp_gray_table(), want)
    r, g, b, sh = R.GRAY
    assert r + g + b == 1 << sh
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.gray_bytes(np.stack([v, v, v], -1)[None]), v[None])                              # (g, g, g) -> g
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "videogpa_amd", "csrc", "superpoint.hip")).read()
    for name, val in zip(("SP_GRAY_R", "SP_GRAY_G", "SP_GRAY_B", "SP_GRAY_SHIFT"), R.GRAY):
        assert f"#define {name} {val}\n" in src


def test_loud_errors():
    from videogpa_amd.scorer import LightGlueMatcher
    from videogpa_amd.superpoint import SuperPoint
    with pytest.raises(RuntimeError, match="never downloads"):
        SuperPoint()
    with pytest.raises(RuntimeError, match="never downloads"):
        LightGlueMatcher(matcher=lambda d: d)                                     # the default extractor needs weights
    with pytest.raises(RuntimeError, match="LightGlue transformer is not implemented on the device yet"):
        LightGlueMatcher(extractor=SuperPoint(pretrained=False))
    with pytest.raises(TypeError):
        SuperPoint(pretrained=False, nms_radios=4)
    with pytest.raises(NotImplementedError):
        SuperPoint(pretrained=False, nms_radius=5)
    net = SuperPoint(pretrained=False)
    with pytest.raises(NotImplementedError, match="48 x 72 to 40 x 60"):
        net._target(48, 72, 60)
    assert net._target(48, 72, 96) == ((64, 96), (96 / 72, 64 / 48)) and net._target(48, 72, None) == ((48, 72), (1.0, 1.0))
    with pytest.raises(ValueError, match="fp32"):
        net({"image": torch.zeros(1, 1, 16, 16, dtype=torch.float64)})
    with torch.enable_grad(), pytest.raises(RuntimeError, match="forward only"):
        net({"image": torch.zeros(1, 1, 16, 16, requires_grad=True)})


def test_no_gpu_is_an_error():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from videogpa_amd.superpoint import SuperPoint
    net = SuperPoint(pretrained=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net({"image": torch.zeros(1, 1, 16, 16)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.extract(torch.zeros(1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.extract_clip(np.zeros((2, 16, 16, 3), np.uint8))


def test_header_exports_and_ctypes_table_agree_on_the_new_entry_points():
    import test_cabi
    from videogpa_amd import _lib, build
    build.build(verbose=False)
    declared = test_cabi._header_signatures(variants=False)
    new = ["vgpa_conv1x1_relu_f32", "vgpa_sp_input_conv1a", "vgpa_sp_head_f32", "vgpa_sp_nms_f32", "vgpa_sp_select_workspace_bytes", "vgpa_sp_select",
           "vgpa_sp_sample_desc_f32"]
    for name in new:
        assert declared[name] == _lib.SIGNATURES[name], name
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in new)
    assert _lib.query("vgpa_sp_select_workspace_bytes", 0, 8, 8) == 0
    assert _lib.query("vgpa_sp_select_workspace_bytes", 2, 48, 72) >= 2 * 48 * 72 * 8
