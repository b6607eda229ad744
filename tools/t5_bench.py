"""Time the T5 text encoder at the real configuration (T5-v1.1-XXL: 24 layers, d_model 4096, 64 heads, d_ff 10240; about 9.5 GB of bf16 weights)
on seeded random weights -- no checkpoint needed -- at B = 1 and B = 2 prompts of 226 tokens, and write profiles/t5_encode.json:

    python tools/t5_bench.py [--out profiles/t5_encode.json] [--layers 24] [--iters 100] [--warmup 5]

A  videogpa_amd.t5.T5EncoderModel (the device module)
B  tests/t5_ref.py in mode "bf16" moved to the same device: plain torch issuing the operation sequence the reference's bf16 module issues
Both read the same weights, in one session, alternating, timed with device events after a warm-up of every shape.  Condition: A is no slower than B
at both batch sizes.  Also reported: A's fraction of the weight-streaming floor = (bf16 bytes of the linear weights) / 6.3 TB/s, the achievable HBM
rate; at 226 or 452 rows per GEMM the encoder cannot run faster than its weights stream.  The module's own kernels (everything but the GEMMs) are
timed per launch in a separate pass under ops.KernelTimer.  Needs a GPU: there is no CPU timing."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_ACHIEVABLE = 6.3e12          # bytes / s


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_encode.json"))
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--tokens", type=int, default=226)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/t5_bench.py measures on the GPU; there is none here")
    import t5_ref
    from videogpa_amd import ops, t5
    cfg = t5_ref.make_cfg(vocab_size=32128, d_model=4096, d_ff=10240, num_layers=args.layers, num_heads=64)
    sd = t5_ref.seeded_state_dict(cfg, seed=0, device="cuda")
    linear_bytes = sum(v.numel() * v.element_size() for k, v in sd.items() if ".SelfAttention." in k and "relative" not in k or ".DenseReluDense." in k)
    with torch.device("meta"):
        model = t5.T5EncoderModel(cfg)
    model.load_state_dict(dict(sd), strict=True, assign=True)
    model.encoder.embed_tokens.weight = model.shared.weight
    ref_sd = sd          # B reads the tensors as drawn; A's q / k / v and wi_0 / wi_1 parameters become views of fused copies on its first forward
    floor_ms = linear_bytes / HBM_ACHIEVABLE * 1e3
    result = {"config": {k: cfg[k] for k in t5_ref.CFG_KEYS}, "tokens": args.tokens, "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "linear_weight_bytes": linear_bytes, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
              "weight_streaming_floor_ms": floor_ms, "batches": {}}
    ok = True
    for B in (1, 2):
        ids = torch.randint(0, cfg["vocab_size"], (B, args.tokens), generator=torch.Generator().manual_seed(B)).cuda()
        run_a = lambda: model(ids)[0]
        run_b = lambda: t5_ref.forward(ref_sd, cfg, ids, None, "bf16", prepared=True)
        with torch.no_grad():
            for _ in range(args.warmup):
                oa, ob = run_a(), run_b()
            torch.cuda.synchronize()
            diff = float((oa.float() - ob.float()).norm() / ob.float().norm())
            ta, tb = [], []
            for _ in range(args.rounds):                    # alternate: other work shares the machine
                ta.append(_time(run_a, args.iters))
                tb.append(_time(run_b, args.iters))
            ops.TIMER = ops.KernelTimer()                   # a run of its own: the event pairs keep launches from overlapping
            for _ in range(args.warmup):
                run_a()
            torch.cuda.synchronize()
            kernels = {k: {"launches_per_forward": v["launches"] / args.warmup, "avg_ms": v["avg_ms"], "ms_per_forward": v["total_ms"] / args.warmup,
                           "work_per_launch": v["work_per_launch"], "unit": v["unit"]} for k, v in ops.TIMER.summary().items()}
            ops.TIMER = None
        a_ms, b_ms = min(ta), min(tb)
        result["batches"][str(B)] = {"device_module_ms": a_ms, "torch_bf16_restatement_ms": b_ms, "device_module_ms_rounds": ta,
                                     "torch_bf16_restatement_ms_rounds": tb, "speedup": b_ms / a_ms, "fraction_of_weight_streaming_floor": floor_ms / a_ms,
                                     "rel_l2_A_vs_B": diff, "no_slower": a_ms <= b_ms, "device_module_kernels": kernels}
        ok = ok and a_ms <= b_ms
        print(f"B {B}: device module {a_ms:.3f} ms, torch bf16 restatement {b_ms:.3f} ms (x{b_ms / a_ms:.2f}); floor {floor_ms:.3f} ms = "
              f"{100 * floor_ms / a_ms:.1f} % of the module's time; ||A - B|| / ||B|| {diff:.2e}")
        for k, v in kernels.items():
            print(f"    {k}: {v['launches_per_forward']:.0f} launches, {v['ms_per_forward']:.3f} ms per forward")
    result["condition_no_slower_at_both_batch_sizes"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
