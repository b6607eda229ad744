"""LightGlue on the device (videogpa_amd/lightglue.py, csrc/lightglue.hip) at the epipolar metric's scale: the consecutive pairs of 2 and of 10 frames
with 2048 keypoints per frame, seeded random weights, as one padded batch (`match_batch`).

Two runs per clip length: (a) pruning and early stopping OFF (depth_confidence = width_confidence = -1): with random weights neither would trigger in
any useful way, so all nine layers run at full length; (b) stopping off, the pruning threshold lowered to 1024 and the pruning weights of
tests/lightglue_ref.py (`prune_state`, matchability gain 100: about a quarter of a side goes per layer) so that the variable-length path (the confidence
and prune kernels, shrinking counts) is timed.  HIP events around each of the warm repetitions, one process.  The device path alternates with a
plain-torch restatement on the same device: fp32 linears, fp16 `F.scaled_dot_product_attention`, the same shapes, no pruning.  The totals are timed with
no event inside the call; the stages in repetitions of their own: attention (ops.KernelTimer around the kernel / events around sdpa), the GEMM kernel
(the torch restatement's linears by difference), the row kernels, the assignment.  Needs the GPU.

    python tools/lightglue_bench.py [--json profiles/lightglue_match.json] [--reps 10]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP16_PEAK_TFLOPS = 2516.6        # MI355X dense fp16 matrix peak (vendor figure)


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "repetitions": len(ms)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def frames_feats(T, K, seed):
    g = torch.Generator().manual_seed(seed)
    size = torch.tensor([[1024.0, 682.0]], device="cuda")
    return [{"keypoints": (torch.rand(1, K, 2, generator=g) * torch.tensor([1024.0, 682.0])).cuda(),
             "descriptors": F.normalize(torch.randn(1, K, 256, generator=g), dim=-1).cuda(), "image_size": size} for _ in range(T)]


def torch_restatement(net, feats, acc):
    """the same nine layers and the assignment in plain torch on the device: fp32 linears, fp16 sdpa; acc (a dict, or None for an undisturbed run)
    collects the per-stage event times"""
    B = len(feats) - 1
    x = torch.cat([torch.cat([f["descriptors"] for f in feats[:-1]]), torch.cat([f["descriptors"] for f in feats[1:]])], 0)       # [2B,K,256]
    kp = torch.cat([torch.cat([f["keypoints"] for f in feats[:-1]]), torch.cat([f["keypoints"] for f in feats[1:]])], 0)
    size = feats[0]["image_size"]
    kp = (kp - size / 2) / (size.max() / 2)
    p = kp @ net.posenc.Wr.weight.t()
    cs, sn = p.cos().repeat_interleave(2, -1)[:, None], p.sin().repeat_interleave(2, -1)[:, None]

    def rot(t):
        a, b = t.unflatten(-1, (-1, 2)).unbind(-1)
        return torch.stack((-b, a), -1).flatten(-2)

    def stage(name, fn):
        if acc is None:
            return fn()
        ms, out = timed(fn)
        acc[name] = acc.get(name, 0.0) + ms
        return out

    def sdpa(q, k, v):
        return stage("attention", lambda: F.scaled_dot_product_attention(q.half(), k.half(), v.half()).float())
    for t in net.transformers:
        s, c = t.self_attn, t.cross_attn
        qkv = s.Wqkv(x).unflatten(-1, (4, 64, 3)).transpose(1, 2)
        q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
        ctx = sdpa(q * cs + rot(q) * sn, k * cs + rot(k) * sn, v)
        x = x + s.ffn(torch.cat([x, s.out_proj(ctx.transpose(1, 2).flatten(2))], -1))
        heads = lambda y: y.unflatten(-1, (4, 64)).transpose(1, 2)
        qk, v = heads(c.to_qk(x)) * 64 ** -0.25, heads(c.to_v(x))
        other = lambda y: torch.cat([y[B:], y[:B]])
        msg = c.to_out(sdpa(qk, other(qk), other(v)).transpose(1, 2).flatten(2))
        x = x + c.ffn(torch.cat([x, msg], -1))

    def assign():
        a = net.log_assignment[-1]
        md = a.final_proj(x) / 4
        sim = md[:B] @ md[B:].transpose(1, 2)
        z = a.matchability(x)
        sc = F.log_softmax(sim, 2) + F.log_softmax(sim, 1) + F.logsigmoid(z[:B]) + F.logsigmoid(z[B:]).transpose(1, 2)
        m0, m1 = sc.max(2), sc.max(1)
        mutual = torch.arange(sc.shape[1], device=sc.device)[None] == m1.indices.gather(1, m0.indices)
        return torch.where(mutual & (m0.values.exp() > 0.1), m0.indices, -1)
    return stage("assignment", assign)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--keypoints", type=int, default=2048)
    args = ap.parse_args()
    import lightglue_ref as R
    from videogpa_amd import ops
    from videogpa_amd.lightglue import LightGlue
    torch.backends.cuda.matmul.allow_tf32 = False
    K = args.keypoints
    result = {"device": torch.cuda.get_device_name(0), "keypoints_per_frame": K,
              "weights": "run (a): seeded random (LightGlue(pretrained=False, seed=0)); run (b): tests/lightglue_ref.py prune_state(0, match_gain=100)",
              "note": "run (a) 'full': pruning and early stopping off, since with plain random weights neither would trigger (no point is ever removed); "
                      "run (b) 'pruning_1024': stopping off, pruning threshold 1024 and the oracle's pruning weights, whose matchability removes about a "
                      "quarter of a side per layer until it is at or below 1024: the shrinking variable-length path.  Totals ('device', "
                      "'torch_restatement') come from repetitions with no event inside the call; the per-stage times from separate repetitions with an "
                      "event pair around every launch (device) or around sdpa and the assignment (torch), which cost time themselves, so the stages are "
                      "not expected to add up to the total.", "runs": {}}
    full = LightGlue(depth_confidence=-1, width_confidence=-1).cuda()
    pruned = LightGlue(depth_confidence=-1)
    pruned.load_state_dict(R.prune_state(0, match_gain=100.0))
    pruned.pruning_keypoint_thresholds = {**LightGlue.pruning_keypoint_thresholds, "flash": 1024}
    pruned = pruned.cuda()
    for T in (2, 10):
        feats = frames_feats(T, K, seed=T)
        B = T - 1
        attn_flops = 9 * 2 * 2 * B * 4.0 * 4 * K * K * 64          # layers x blocks x sides: 4 H Tq Tk 64 each
        for name, net in (("full", full), ("pruning_1024", pruned)):
            out = net.match_batch(feats)                           # warm: allocator, kernel-layout copies
            torch_restatement(net, feats, None)
            dev_ms, ref_ms, stages, staged_ms, ref_stages = [], [], [], [], []
            for _ in range(args.reps):
                dev_ms.append(timed(lambda: net.match_batch(feats))[0])
                if name == "full":
                    ref_ms.append(timed(lambda: torch_restatement(net, feats, None))[0])
                ops.TIMER = ops.KernelTimer()
                ms, _ = timed(lambda: net.match_batch(feats))
                summ, ops.TIMER = ops.TIMER.summary(), None
                staged_ms.append(ms)
                tot = lambda names: sum(summ[n]["total_ms"] for n in names if n in summ)
                stages.append({"attention": tot(["lg_attn_fwd"]), "row_kernels": tot(["lg_posenc", "lg_ln_gelu", "lg_confidence", "lg_prune"]),
                               "assignment": tot(["lg_assign"]), "gemms": tot(["lg_gemm"])})
                if name == "full":
                    acc = {}
                    timed(lambda: torch_restatement(net, feats, acc))
                    ref_stages.append(acc)
            med = lambda rows: {k: statistics.median(r[k] for r in rows) for k in rows[0]}
            run = {"pairs": B, "device": stats(dev_ms), "device_stages_ms_median": med(stages), "device_ms_median_with_stage_events": statistics.median(staged_ms)}
            run["device_stages_ms_median"]["rest_by_difference"] = run["device"]["ms_median"] - sum(run["device_stages_ms_median"].values())
            if name != "full":                                     # a point still alive at the end was counted at every pruning of its side
                alive = [[int((o[k][0] == o[k][0].max()).sum()) for o in out] for k in ("prune0", "prune1")]
                run.update(prunings_per_side_max=int(max(int(o["prune0"].max()) for o in out)) - 1,
                           kept_points_mean=(sum(alive[0]) + sum(alive[1])) / (2.0 * B))
            else:
                att = run["device_stages_ms_median"]["attention"]
                tst = med(ref_stages)
                tst["linears_and_rest_by_difference"] = statistics.median(ref_ms) - sum(tst.values())
                run.update(kept_points_mean=float(K), attention_flops=attn_flops, attention_tflops=attn_flops / att / 1e9,
                           attention_fraction_of_fp16_matrix_peak=attn_flops / att / 1e9 / FP16_PEAK_TFLOPS,
                           torch_restatement=stats(ref_ms), torch_stages_ms_median=tst)
            result["runs"][f"{T}_frames_{name}"] = run
            print(f"{T} frames {name}: device {run['device']['ms_median']:.2f} ms, stages {run['device_stages_ms_median']}, kept {run['kept_points_mean']:.0f}"
                  + (f", torch {run['torch_restatement']['ms_median']:.2f} ms, stages {run['torch_stages_ms_median']}" if name == "full" else ""))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
