"""Writes tests/golden/dualdpt.pt, dualdpt_{A,B}.pt and dualdpt_names.json: Depth Anything 3's DualDPT head (depth_anything_3/model/dualdpt.py)
imported from the reference and evaluated on the CPU in fp32 and in float64.

    python tests/golden/make_golden_dualdpt.py /path/to/reference

Tensors, numbers and names only, every file below 1 MiB.  The reduced configuration, the cases and the seeded recipe are tests/dualdpt_ref.py's:
  dualdpt.pt          cfg, seed, shapes and per-tensor float64 sums of the state (434 350 parameters, 1.7 MB: the tests regenerate it from the recipe and check
                      the sums)
  dualdpt_CASE.pt     per case: the four feature tensors, the four outputs in fp32 (unchunked) and float64, d32 per output (max-abs difference over
                      max-abs of the float64 answer), and the range of every logit
  dualdpt_names.json  names and shapes of DualDPT(2048) at the defaults, built on the meta device
Of the reference's chunked evaluation (chunk_size below S) only its distance from float64 is stored (d32_chunked)."""
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dualdpt_ref as R  # noqa: E402


class AttrDict(dict):
    """stands in for addict.Dict, which dualdpt.py imports for its return value: a dict whose keys read as attributes"""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def save(name, obj):
    path = os.path.join(HERE, name)
    torch.save(obj, path)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20), "fixtures stay below 1 MiB each"


def import_reference(ref_root):
    """the package __init__ chain needs omegaconf and cv2: the parent packages are registered as plain namespaces, and `addict` as the stand-in above"""
    sys.path.insert(0, ref_root)
    for pkg in ("depth_anything_3", "depth_anything_3.model", "depth_anything_3.model.utils"):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = [os.path.join(ref_root, *pkg.split("."))]
            sys.modules[pkg] = m
    if "addict" not in sys.modules:
        stub = types.ModuleType("addict")
        stub.Dict = AttrDict
        sys.modules["addict"] = stub
    from depth_anything_3.model import dualdpt
    return dualdpt


def main(ref_root):
    dualdpt = import_reference(ref_root)
    head = dualdpt.DualDPT(**R.CFG).eval()
    shapes = {k: list(v.shape) for k, v in head.state_dict().items()}
    state = R.seeded_state(shapes, R.SEED)
    head.load_state_dict(state, strict=True)
    head64 = dualdpt.DualDPT(**R.CFG).eval().double()
    head64.load_state_dict({k: v.double() for k, v in state.items()}, strict=True)
    print("parameters", sum(v.numel() for v in state.values()), "tensors", len(state))
    save("dualdpt.pt", {"cfg": dict(R.CFG), "seed": R.SEED, "shapes": shapes, "sums": R.state_sums(state)})
    for name, (B, S, (H, W)) in R.CASES.items():
        feats = R.features(name)
        with torch.no_grad():
            out32 = head([(f, None) for f in feats], H, W, patch_start_idx=0, chunk_size=8)
            chunked = head([(f, None) for f in feats], H, W, patch_start_idx=0, chunk_size=2 if S > 2 else 1)
            out64 = head64([(f.double(), None) for f in feats], H, W, patch_start_idx=0, chunk_size=8)
        assert tuple(out32) == R.OUTPUTS, tuple(out32)
        c = {"feats": feats, "hw": (H, W), "out32": {k: v.clone() for k, v in out32.items()}, "out64": {k: v.clone() for k, v in out64.items()},
             "d32": {k: R.rel(out32[k], out64[k]) for k in R.OUTPUTS}}
        c["d32_chunked"] = {k: R.rel(chunked[k], out64[k]) for k in R.OUTPUTS}       # the reference's own chunked evaluation: the same class
        logits = {"depth": out64["depth"].log(), "depth_conf": (out64["depth_conf"] - 1).log(), "ray": out64["ray"], "ray_conf": (out64["ray_conf"] - 1).log()}
        c["logit_range"] = {k: (float(v.min()), float(v.max())) for k, v in logits.items()}
        print(name, {k: tuple(v.shape) for k, v in out64.items()})
        print(name, "d32", {k: float(f"{v:.2e}") for k, v in c["d32"].items()}, "logits", {k: (round(a, 2), round(b, 2)) for k, (a, b) in c["logit_range"].items()})
        save(f"dualdpt_{name}.pt", c)
    with torch.device("meta"):
        full = dualdpt.DualDPT(2048)
    names = {k: list(v.shape) for k, v in full.state_dict().items()}
    path = os.path.join(HERE, "dualdpt_names.json")
    with open(path, "w") as f:
        json.dump(names, f, indent=0, sort_keys=True)
    print(path, len(names), os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
