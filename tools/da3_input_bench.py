"""Depth Anything 3's input processing (videogpa_amd/da3_input.py, csrc/da3_input.hip) at the scorer's scale: 10 frames of 480 x 720 (what
generate.image_to_video produces) -> 336 x 504 under the default `upper_bound_resize` at process_res 504, i.e. one INTER_AREA stage whose epilogue
writes the network's input `x` and `processed_images`.

Reported, from HIP events around each of 20 warm repetitions: the launches of one call, the bytes it has to move (one read of the source, one write of
`x`, one write of `processed_images`), microseconds (median / min / max), the achieved bytes per second and its fraction of the HBM streaming rate
(6.3 TB/s, the rate the project's streaming kernels reach, tools/t5_bench.py; the 8 TB/s peak next to it).  The working set (36 MB) fits the last-level
cache, so a fraction above what HBM alone allows is possible and says so.  For comparison, in the same process: the same work restated in plain torch
(F.interpolate(mode="area") on an fp32 copy, round, normalise, the uint8 image: the same traffic pattern, not the same pixels, since torch's "area" is
adaptive average pooling with unweighted whole-pixel windows), and the two-stage 704 x 1280 plan (area then cubic).  Needs the GPU.

    python tools/da3_input_bench.py [--json PATH] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_STREAM = 6.3e12      # bytes / s the project's streaming kernels reach
HBM_PEAK = 8.0e12


def timed(fn, reps, warm=3):
    """-> microseconds of each of `reps` calls, one event pair per call, after `warm` untimed calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in pairs]


def summary(us, nbytes=None):
    out = {"us_median": statistics.median(us), "us_min": min(us), "us_max": max(us), "repetitions": len(us)}
    if nbytes is not None:
        rate = nbytes / (out["us_median"] * 1e-6)
        out.update(bytes=nbytes, bytes_per_second=rate, fraction_of_hbm_streaming_rate=rate / HBM_STREAM, fraction_of_hbm_peak=rate / HBM_PEAK)
    return out


def torch_restatement(frames, h, w):
    """the same outputs from torch ops: an fp32 NCHW copy, adaptive average pooling, round, normalise, and the uint8 image"""
    mean = torch.tensor([0.485, 0.456, 0.406], device=frames.device).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=frames.device).view(1, 3, 1, 1)
    u = F.interpolate(frames.permute(0, 3, 1, 2).float(), size=(h, w), mode="area").round_().clamp_(0, 255)
    x = ((u / 255.0 - mean) / std).unsqueeze(0)
    return x, u.permute(0, 2, 3, 1).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("da3_input_bench needs the GPU: nothing here is a measurement without it")
    from videogpa_amd import da3_input, ops
    dev = torch.device("cuda")
    T, H, W = 10, 480, 720
    frames = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    stages, (h, w) = da3_input.plan(H, W, 504, "upper_bound_resize")
    assert stages == [("area", 336, 504)], stages
    table = torch.from_numpy(da3_input.processed_table()).to(dev)
    nbytes = T * H * W * 3 + T * 3 * h * w * 4 + T * h * w * 3
    res = {"device": torch.cuda.get_device_name(0), "workload": f"{T} frames of {H} x {W} -> {h} x {w}, upper_bound_resize at process_res 504",
           "plan": [list(s) for s in stages], "hbm_streaming_rate_bytes_per_second": HBM_STREAM, "hbm_peak_bytes_per_second": HBM_PEAK}

    res["fused"] = dict(summary(timed(lambda: ops.da3_resize(frames, h, w, "area", table=table), args.reps), nbytes),
                        launches=3, launches_note="two tap-table kernels (out_w and out_h threads) and the area kernel with the last stage as its epilogue",
                        bytes_note="one read of the source, one write of x (fp32), one write of processed_images (uint8)")
    # the same pixels without the epilogue: the resized uint8 image written, then read again by the last stage
    unfused_bytes = nbytes + 2 * T * h * w * 3
    res["resize_then_last_stage"] = dict(summary(timed(lambda: ops.da3_normalize(ops.da3_resize(frames, h, w, "area"), table), args.reps), unfused_bytes), launches=4)
    res["torch_restatement"] = dict(summary(timed(lambda: torch_restatement(frames, h, w), args.reps)),
                                    note="F.interpolate(mode='area') on an fp32 NCHW copy + round + normalise + uint8 image; time only, it moves several fp32 images")
    proc = da3_input.InputProcessor(dev)
    res["input_processor_call"] = dict(summary(timed(lambda: proc.process(frames), args.reps)), note="InputProcessor.process on a device tensor: host planning and allocation included")

    x, p = ops.da3_resize(frames, h, w, "area", table=table)
    xt, ut = torch_restatement(frames, h, w)
    u = ops.da3_resize(frames, h, w, "area")
    res["against_torch_restatement"] = {"uint8_samples_differing": int((u != ut).sum()), "of": u.numel(), "max_grey_level_difference": int((u.int() - ut.int()).abs().max()),
                                        "max_abs_difference_of_x": float((x - xt).abs().max()),
                                        "note": "not an accuracy figure: F.interpolate(mode='area') is adaptive average pooling, whole source pixels with equal weights, "
                                                "where INTER_AREA weights the border pixels by their covered fraction, so on random bytes most samples differ; the "
                                                "restatement is here for its time.  tests/test_gpu_da3_input.py holds the accuracy checks"}

    T2, H2, W2 = 10, 704, 1280
    frames2 = torch.randint(0, 256, (T2, H2, W2, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    st2, (h2, w2) = da3_input.plan(H2, W2, 504, "upper_bound_resize")
    mid = st2[0]
    bytes2 = T2 * H2 * W2 * 3 + 2 * T2 * mid[1] * mid[2] * 3 + T2 * 3 * h2 * w2 * 4 + T2 * h2 * w2 * 3
    res["two_stage_704x1280"] = dict(summary(timed(lambda: proc.process(frames2), args.reps), bytes2), plan=[list(s) for s in st2], launches=6,
                                     note="host-inclusive InputProcessor.process; the uint8 image between the stages is written once and read once")
    for k, v in res.items():
        if isinstance(v, dict) and "us_median" in v:
            frac = f"  {v['bytes'] / 1e6:6.1f} MB  {v['bytes_per_second'] / 1e12:5.2f} TB/s = {v['fraction_of_hbm_streaming_rate']:.2f} of the streaming rate" if "bytes" in v else ""
            print(f"{k:26s} {v['us_median']:9.1f} us (min {v['us_min']:.1f}, max {v['us_max']:.1f}){frac}", flush=True)
    print("against the torch restatement:", res["against_torch_restatement"])
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
