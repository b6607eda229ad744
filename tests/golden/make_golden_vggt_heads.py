"""Writes tests/golden/vggt_heads.pt: the reference's CameraHead and DPTHead (vggt/heads) evaluated on the CPU in fp32 and in float64.

    python tests/golden/make_golden_vggt_heads.py /path/to/reference

Tensors only, three files below 1 MiB each (vggt_heads.pt: inputs + the depth head; vggt_heads_point.pt; vggt_heads_camera.pt).  Cases: a
depth head (exp, output_dim 2) and a point head (inv_log, output_dim 4) at 3 frames of 42 x 56 (a non-square 3 x 4 patch grid), each
unchunked and with frames_chunk_size=2, and a camera head with 2 trunk blocks.  The default initialisation leaves the depth output within
0.86-0.90, so the random weights are scaled up until the pre-activation values span several units and both signs."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def scaled_init(module, gen, gain):
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.ndim >= 2:
                fan_in = p[0].numel() if not name.startswith("resize_layers.0") and not name.startswith("resize_layers.1") else p.shape[0]
                p.copy_(torch.randn(p.shape, generator=gen) * gain / fan_in ** 0.5)
            elif name.endswith("gamma"):
                p.copy_(0.5 + 0.5 * torch.rand(p.shape, generator=gen))
            elif name.endswith("norm.weight") or ".norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=gen))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))


CFG = dict(dim_in=32, features=32, out_channels=[16, 16, 32, 32], intermediate_layer_idx=[0, 1, 2, 3])
GAIN = float(os.environ.get("VGPA_GOLDEN_GAIN", "1.15"))


def save(name, obj):
    path = os.path.join(HERE, name)
    torch.save(obj, path)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20), "fixtures stay below 1 MiB each"


def main(ref_root):
    sys.path.insert(0, ref_root)
    from vggt.heads.camera_head import CameraHead
    from vggt.heads.dpt_head import DPTHead
    g = torch.Generator().manual_seed(1234)
    B, S, H, W, patch, psi, dim = 1, 3, 42, 56, 14, 5, CFG["dim_in"]
    P = psi + (H // patch) * (W // patch)
    tokens = [torch.randn(B, S, P, dim, generator=g) for _ in range(4)]
    images = torch.rand(B, S, 3, H, W, generator=g)
    depth = DPTHead(patch_size=patch, output_dim=2, activation="exp", **CFG).eval()
    scaled_init(depth, g, gain=GAIN)
    point = DPTHead(patch_size=patch, output_dim=4, activation="inv_log", **CFG).eval()
    point.load_state_dict({k: v for k, v in depth.state_dict().items() if not k.startswith("scratch.output_conv2")}, strict=False)
    scaled_init(point.scratch.output_conv2, g, gain=GAIN)
    files = {"depth": {"tokens": tokens, "image_hw": torch.tensor([H, W]), "patch_start_idx": torch.tensor(psi),
                       "state": {k: v.clone() for k, v in depth.state_dict().items()}},
             # the point head shares every layer below scratch.output_conv2 with the depth head: only the difference is stored
             "point": {"state_delta": {k: v.clone() for k, v in point.state_dict().items() if k.startswith("scratch.output_conv2")}}}
    for tag, head in (("depth", depth), ("point", point)):
        out = files[tag]
        with torch.no_grad():
            for chunk_tag, chunk in (("", 8), ("chunk2.", 2)):
                p32, c32 = head(tokens, images, psi, frames_chunk_size=chunk)
                out[f"{chunk_tag}preds32"], out[f"{chunk_tag}conf32"] = p32.clone(), c32.clone()
            p64, c64 = head.double()([t.double() for t in tokens], images.double(), psi, frames_chunk_size=8)
            out["preds64"], out["conf64"] = p64.clone(), c64.clone()
        pre = torch.log(p64) if tag == "depth" else torch.sign(p64) * torch.log1p(p64.abs())
        print(tag, "pre-activation values", float(pre.min()), float(pre.max()), "confidence logits", float(torch.log(c64 - 1).min()),
              float(torch.log(c64 - 1).max()))
    cam = CameraHead(dim_in=64, trunk_depth=2, num_heads=2).eval()
    scaled_init(cam, g, gain=1.0)
    cam_tokens = [torch.randn(B, S, 1, 64, generator=g)]              # only the camera token (index 0) is read
    camera = {"tokens": cam_tokens[0], "state": {k: v.clone() for k, v in cam.state_dict().items()}}
    with torch.no_grad():
        camera["pose32"] = torch.stack(cam(cam_tokens, num_iterations=4))
        camera["pose64"] = torch.stack(cam.double()([t.double() for t in cam_tokens], num_iterations=4))
    print("camera pose range", float(camera["pose64"].min()), float(camera["pose64"].max()))
    save("vggt_heads.pt", files["depth"])
    save("vggt_heads_point.pt", files["point"])
    save("vggt_heads_camera.pt", camera)


if __name__ == "__main__":
    main(sys.argv[1])
