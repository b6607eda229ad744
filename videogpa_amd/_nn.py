"""What the forward-only modules of vggt.py, dpt.py, da3.py and lpips.py share and no kernel is behind: the gradient refusal, the cache of
kernel-layout parameter copies, and the reader of local checkpoints."""
import os

import torch


def _forward_only(module, *tensors):
    if torch.is_grad_enabled() and (any(p.requires_grad for p in module.parameters()) or any(t.requires_grad for t in tensors)):
        raise RuntimeError(f"{type(module).__name__} is forward only (no backward kernels): call it under torch.no_grad()")


class _PackedCache:
    """fp32 kernel-layout copies of parameters, rebuilt when a parameter's `_version`, storage or device changes"""

    def __init__(self):
        self._c = {}

    def get(self, key, params, make):
        tag = tuple((p._version, p.data_ptr(), str(p.device), p.dtype) for p in params)
        hit = self._c.get(key)
        if hit is None or hit[0] != tag:
            with torch.no_grad():
                hit = (tag, make())
            self._c[key] = hit
        return hit[1]


def read_state_file(path):
    """the state dict in one .safetensors file, or in anything else through torch.load(weights_only=True)"""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    return torch.load(path, map_location="cpu", weights_only=True)


def read_checkpoint(path):
    """A state dict from the LOCAL file system (never the network): `path` is a directory holding model.safetensors or model.pt, or such a file."""
    path = os.fspath(path)
    if os.path.isdir(path):
        found = [f for f in ("model.safetensors", "model.pt") if os.path.isfile(os.path.join(path, f))]
        if not found:
            raise FileNotFoundError(f"{path}: neither model.safetensors nor model.pt (from_pretrained reads local checkpoints only)")
        path = os.path.join(path, found[0])
    elif not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such checkpoint file or directory (from_pretrained reads local checkpoints only)")
    return read_state_file(path)
