"""Writes tests/golden/da3_input_plan.json: what Depth Anything 3's own `InputProcessor` (depth_anything_3/utils/io/input_processor.py) does to frames of
given sizes -- the cv2.resize calls it makes (interpolation and size, in order), the crop box, the final size and the transformed intrinsics -- by
importing it from the reference and running it.

    python tests/golden/make_golden_da3_input.py /path/to/reference

`cv2` and `torchvision.transforms` are stubbed (neither is needed for sizes and intrinsics, which do not depend on pixel values): the stub `cv2.resize`
returns zeros of the requested size and logs the call, `PIL.Image.Image.crop` is wrapped to log its box.  imageio / tqdm, which the reference's
parallel_utils imports, are stubbed when absent.  The fixture holds numbers and names only."""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(480, 720), (768, 1360), (704, 1280), (720, 480), (518, 518), (504, 376), (200, 300)]          # (H, W)
BATCHES = [[(480, 720), (720, 480)], [(518, 518), (504, 376)], [(704, 1280), (480, 720), (704, 1280)]]
METHODS = ["upper_bound_resize", "upper_bound_crop", "lower_bound_resize", "lower_bound_crop"]
PROCESS_RES = 504
LOG = []


def stub_modules():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_AREA, cv2.INTER_CUBIC = "area", "cubic"

    def resize(arr, size, interpolation=None):
        w, h = size
        LOG.append([interpolation, int(h), int(w)])
        return np.zeros((h, w, 3), np.uint8)
    cv2.resize = resize
    sys.modules["cv2"] = cv2

    tv, T = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    class Normalize:                                   # a class: InputProcessor.NORMALIZE is a class attribute, a function there would bind as a method
        def __init__(self, mean, std):
            pass

        def __call__(self, t):
            return t
    T.Normalize = Normalize
    T.ToTensor = lambda: (lambda img: torch.from_numpy(np.asarray(img)).permute(2, 0, 1).float())

    def center_crop(size):
        h, w = size
        return lambda t: t[..., (t.shape[-2] - h) // 2:(t.shape[-2] - h) // 2 + h, (t.shape[-1] - w) // 2:(t.shape[-1] - w) // 2 + w]
    T.CenterCrop = center_crop
    tv.transforms = T
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, T
    for name in ("imageio", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            m.tqdm = lambda it, *a, **k: it
            sys.modules[name] = m

    crop = Image.Image.crop

    def logged_crop(self, box=None):
        left, top, right, bottom = box
        LOG.append(["crop", int(top), int(left), int(bottom - top), int(right - left)])
        return crop(self, box)
    Image.Image.crop = logged_crop


def import_reference(ref_root):
    sys.path.insert(0, ref_root)
    for pkg in ("depth_anything_3", "depth_anything_3.utils", "depth_anything_3.utils.io"):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = [os.path.join(ref_root, *pkg.split("."))]
            sys.modules[pkg] = m
    from depth_anything_3.utils.io import input_processor
    return input_processor.InputProcessor


def make_k(h, w):
    return np.array([[1200.0, 0, w / 2.0], [0, 1100.0, h / 2.0], [0, 0, 1]], dtype=np.float32)


def main(ref_root):
    stub_modules()
    proc = import_reference(ref_root)()
    rows, batches = [], []
    for H, W in SIZES:
        for method in METHODS:
            for with_k in (False, True):
                LOG.clear()
                K = make_k(H, W)[None] if with_k else None
                x, _, k_out = proc([np.zeros((H, W, 3), np.uint8)], None, K, PROCESS_RES, method, num_workers=1, sequential=True)
                rows.append(dict(H=H, W=W, process_res=PROCESS_RES, method=method, stages=[list(s) for s in LOG], size=list(x.shape[-2:]),
                                 K_in=None if K is None else K[0].tolist(), K_out=None if k_out is None else k_out[0].tolist()))
    for sizes in BATCHES:
        for method in METHODS:
            K = np.stack([make_k(h, w) for h, w in sizes])
            x, _, k_out = proc([np.zeros((h, w, 3), np.uint8) for h, w in sizes], None, K, PROCESS_RES, method, num_workers=1, sequential=True)
            batches.append(dict(sizes=[list(s) for s in sizes], process_res=PROCESS_RES, method=method, size=list(x.shape[-2:]), K_in=K.tolist(),
                                K_out=k_out.tolist()))
    path = os.path.join(HERE, "da3_input_plan.json")
    with open(path, "w") as f:
        json.dump(dict(rows=rows, batches=batches), f, indent=0)
    print(path, os.path.getsize(path), len(rows), len(batches))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(sys.argv[1])
