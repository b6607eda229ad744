"""SuperPoint on the device (videogpa_amd/superpoint.py, csrc/superpoint.hip) at the epipolar metric's scale: ten frames of 480 x 720 (what
generate.image_to_video produces) resized to 682 x 1024 as `Extractor.extract` does, max_num_keypoints = 2048, seeded random weights.

Reported, from HIP events around each of the warm repetitions: the whole `extract_clip` (host planning, allocation and the one read of the counts
included) and each stage on its own, alternating with a plain-torch fp32 restatement (tests/superpoint_ref.py on the same device, TF32 off) of the same
frames in the same process; next to the times, the bytes every stage has to move and its FLOPs, both from the shapes.  On random weights nearly every
8 x 8 cell holds a keypoint candidate, so the selection runs with an active cut in every frame.  Needs the GPU.

    python tools/superpoint_bench.py [--json profiles/superpoint_extract.json] [--reps 10]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    return (a, b), out


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "repetitions": len(ms)}


def shapes(T, H, W, Ho, Wo, K):
    """bytes that must move and FLOPs of every stage, from the shapes alone (fp32 maps, each read once and written once)"""
    from videogpa_amd.superpoint import LAYERS
    out, h, w = {}, Ho, Wo
    out["input_conv1a"] = {"bytes": T * (H * W * 3 + Ho * Wo * 64 * 4), "flops": 2 * T * Ho * Wo * 9 * 64}
    stack_b = stack_f = 0
    for name, cin, cout, ks in LAYERS[1:8]:
        stack_b += T * h * w * (cin + cout) * 4
        stack_f += 2 * T * h * w * ks * ks * cin * cout
        if name in ("conv1b", "conv2b", "conv3b"):
            stack_b += T * h * w * cout * 4 + T * (h // 2) * (w // 2) * cout * 4
            h, w = h // 2, w // 2
    out["conv1b_to_conv4b_with_pools"] = {"bytes": stack_b, "flops": stack_f}
    cells = T * h * w
    out["convPa_and_detector_head"] = {"bytes": cells * (128 + 256 + 256 + 64) * 4, "flops": 2 * cells * (9 * 128 * 256 + 256 * 65)}
    out["convDa_and_convDb"] = {"bytes": cells * (128 + 256 + 256 + 256) * 4, "flops": 2 * cells * (9 * 128 * 256 + 256 * 256)}
    out["nms_and_borders"] = {"bytes": 2 * cells * 64 * 4, "flops": 0}
    out["threshold_compaction_selection"] = {"bytes": cells * 64 * 4 * 2 + T * K * 12, "flops": 0}
    out["descriptor_sampling"] = {"bytes": T * K * 5 * 256 * 4, "flops": 0}
    out["whole"] = {"bytes": sum(v["bytes"] for v in out.values()), "flops": sum(v["flops"] for v in out.values())}
    return out, (h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("superpoint_bench needs the GPU: nothing here is a measurement without it")
    import superpoint_ref as R
    from videogpa_amd import ops
    from videogpa_amd.superpoint import SuperPoint, side_to_image_size
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda")
    T, H, W, K = 10, 480, 720, 2048
    Ho, Wo = side_to_image_size((H, W), 1024)
    frames = R.smooth_frames(T, H, W, seed=0).to(dev)
    net = SuperPoint(pretrained=False, max_num_keypoints=K, frames_chunk=T).to(dev)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    p = net.packed()
    work, (h, w) = shapes(T, H, W, Ho, Wo, K)

    def stack(x):
        for name in ("conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b"):
            x = ops.conv3x3_f32(x, *p[name], relu_in=name not in ("conv2a", "conv3a", "conv4a"))
            if name in ("conv1b", "conv2b", "conv3b"):
                x = ops.maxpool2x2_f32(x, relu=True)
        return x

    def torch_whole():
        img = R.resize(torch.from_numpy(R.gray_bytes(frames.cpu().numpy()) / 255.0).float()[:, None].to(dev), (Ho, Wo))
        return R.detect(sd, img, k=K)

    def torch_device_part(img):
        return R.detect(sd, img, k=K)

    gray_small = R.frame2tensor(frames.cpu()).to(dev)
    stages = {"input_conv1a": [], "conv1b_to_conv4b_with_pools": [], "convPa_and_detector_head": [], "convDa_and_convDb": [], "nms_and_borders": [],
              "threshold_compaction_selection": [], "descriptor_sampling": [], "whole": [], "torch_restatement_on_device": [],
              "torch_restatement_with_host_gray": []}
    with torch.no_grad():
        for rep in range(args.reps + 2):
            ev = {}
            ev["whole"], feats = event_ms(lambda: net.extract_clip(frames))
            ev["input_conv1a"], c1 = event_ms(lambda: ops.sp_input_conv1a(frames, *p["conv1a"], size=(Ho, Wo), table=p["table"]))
            ev["conv1b_to_conv4b_with_pools"], x = event_ms(lambda: stack(c1))
            del c1
            ev["convPa_and_detector_head"], score = event_ms(lambda: ops.sp_head_f32(ops.conv3x3_f32(x, *p["convPa"], relu_in=True), *p["convPb"]))
            ev["convDa_and_convDb"], dmap = event_ms(lambda: ops.conv1x1_relu_f32(ops.conv3x3_f32(x, *p["convDa"], relu_in=True), *p["convDb"]))
            ev["nms_and_borders"], nms = event_ms(lambda: ops.sp_nms_f32(score, 4, 4))
            ev["threshold_compaction_selection"], (kp, sc, counts) = event_ms(lambda: ops.sp_select(nms, 0.0005, K))
            ev["descriptor_sampling"], desc = event_ms(lambda: ops.sp_sample_desc_f32(dmap, kp, counts))
            ev["torch_restatement_on_device"], ref = event_ms(lambda: torch_device_part(R.resize(gray_small, (Ho, Wo))))
            if rep == 2:
                ev["torch_restatement_with_host_gray"], _ = event_ms(torch_whole)
            torch.cuda.synchronize()
            if rep >= 2:
                for k, (a, b) in ev.items():
                    stages[k].append(a.elapsed_time(b))
    res = {"device": torch.cuda.get_device_name(0),
           "workload": f"{T} frames of {H} x {W} -> {Ho} x {Wo}, max_num_keypoints {K}, seeded random weights, smooth frames, one chunk of {T}",
           "keypoints_per_frame": [int(f["keypoints"].shape[1]) for f in feats], "cells": [h, w], "stages": {}}
    for k, ms in stages.items():
        if not ms:
            continue
        entry = stats(ms)
        if k in work:
            entry.update(work[k])
            s = entry["ms_median"] * 1e-3
            entry["bytes_per_second"] = work[k]["bytes"] / s
            entry["flops_per_second"] = work[k]["flops"] / s
        res["stages"][k] = entry
        print(f"{k:36s} {entry['ms_median']:9.3f} ms (min {entry['ms_min']:.3f}, max {entry['ms_max']:.3f})"
              + (f"  {entry['bytes'] / 1e6:8.1f} MB {entry['bytes_per_second'] / 1e12:5.2f} TB/s  {entry['flops'] / 1e9:8.1f} GFLOP "
                 f"{entry['flops_per_second'] / 1e12:6.1f} TFLOP/s" if k in work else ""), flush=True)
    res["stages"]["whole"]["note"] = "SuperPoint.extract_clip on device frames: host planning, allocation, the read of the counts and the per-frame slicing included"
    res["stages"]["torch_restatement_on_device"]["note"] = ("tests/superpoint_ref.py in fp32 on the same device from the gray image on: resize, backbone, NMS, "
                                                             "torch.where per frame, stable sort, grid_sample; the gray conversion is left out of it")
    res["note"] = "bytes and FLOPs are computed from the shapes, not measured"
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
