"""CogVideoX feed-forward, bf16 against e4m3 (CogVideoXTransformer3DModel.enable_fp8), in ONE process so that only the in-session ratio counts:

  1. the block tail (gated residual + norm2 -> W1 -> GELU -> W2 -> gated residual + next norm), forward + backward, at the cfg2 row count
     (M = 2 x 17 776 = 35 552 rows, D = 3072, inner 12 288): ops.ffn_tail_fp8 against the four calls CogVideoXBlock.forward makes otherwise.
     Every call takes the NEXT of several operand sets (a loop over one set is served by the 256 MB infinity cache, the step's operands were
     written a layer ago); the two variants alternate, and each round is reported so that the spread is visible next to the difference.
  2. the same tail once more under the KernelTimer: GB/s of the quantising row kernels, TFLOP/s of the fp8 and bf16 vendor GEMMs.
  3. pair steps of the cfg2 geometry (bench.py's builders; --layers blocks, 42 = the full model) with the switch off / on, alternating.

    PYTHONPATH=. python tools/cogvideox_ffn_ab.py [--layers N] [--steps K] [--out profiles/cogvideox_ffn_ab.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (builders only)
from videogpa_amd import ops, transformer as vtr  # noqa: E402
from videogpa_amd.trainer import CogVideoXDPOTrainer, DPOEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=8, help="transformer blocks of the pair-step A/B (42 = cfg2 itself)")
ap.add_argument("--steps", type=int, default=3, help="pair steps per round and variant")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--tail-iters", type=int, default=6, help="tail forward+backward calls per round and variant")
ap.add_argument("--sets", type=int, default=3, help="operand sets in rotation (each 2 x 218 MB of inputs)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cogvideox_ffn_ab.json"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("cogvideox_ffn_ab.py measures on the GPU; there is none here")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
C = bench.CONFIGS["cfg2"]
B, D, INNER, LT = 2, 3072, 12288, bench.TEXT_LEN
S = LT + C["frames"] * (C["height"] // 2) * (C["width"] // 2)
M = B * S
res = {"geometry": {"rows": M, "B": B, "S": S, "text_len": LT, "D": D, "inner": INNER}}


# ------------------------------------------------------------------------------------------------ 1. the block tail
def tail_sets(n):
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s, std=1.0: std * torch.randn(*s, device=dev, generator=g)       # noqa: E731
    sets = []
    for _ in range(n):
        sets.append({k: r(B, S, D).bfloat16() for k in ("x", "a", "dx", "dn")})

    def mod():                  # (shift_v, 1 + scale_v, shift_t, 1 + scale_t)
        m = r(B, 4, D, std=0.3)
        m[:, 1] += 1
        m[:, 3] += 1
        return m
    p = {"mod2": mod(), "nmod": mod(), "gates1": r(B, 2, D, std=0.3), "gates2": r(B, 2, D, std=0.3), "w2": 1 + r(D, std=0.1), "b2": r(D, std=0.1),
         "wn": 1 + r(D, std=0.1), "bn": r(D, std=0.1), "W1": r(INNER, D, std=0.02).bfloat16(), "b1": r(INNER, std=0.02).bfloat16(),
         "W2": r(D, INNER, std=0.02).bfloat16(), "b2f": r(D, std=0.02).bfloat16()}
    return sets, p


def tail(s, p, fp8):
    x, y = s["x"].detach().requires_grad_(True), s["a"].detach().requires_grad_(True)
    if fp8:
        xo, nn = ops.ffn_tail_fp8(x, y, p["gates1"], p["w2"], p["b2"], p["mod2"], p["W1"], p["b1"], p["W2"], p["b2f"], p["gates2"], p["wn"], p["bn"], p["nmod"],
                                  1e-5, LT, 1e-5, n_pad=192, dy_pad=64)
    else:
        x1, n2 = ops.residual_ln(x, y, p["gates1"], p["w2"], p["b2"], p["mod2"], LT, 1e-5, dy_pad=64)
        f = ops.frozen_linear(ops.gelu_tanh(ops.frozen_linear(n2, p["W1"], p["b1"])), p["W2"], p["b2f"])
        xo, nn = ops.residual_ln(x1, f, p["gates2"], p["wn"], p["bn"], p["nmod"], LT, 1e-5, n_pad=192)
    torch.autograd.backward([xo, nn], [s["dx"], s["dn"]])


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


sets, par = tail_sets(a.sets)
for fp8 in (False, True):                  # warm-up: code objects, the vendor library's algorithm choice, the e4m3 weight copies
    for i in range(2):
        tail(sets[i % len(sets)], par, fp8)
rounds = {"bf16": [], "fp8": []}
for _ in range(a.rounds):
    for name, fp8 in (("bf16", False), ("fp8", True)):
        rounds[name].append(timed(lambda i: tail(sets[i % len(sets)], par, fp8), a.tail_iters))
mean = {k: sum(v) / len(v) for k, v in rounds.items()}
spread = {k: (max(v) - min(v)) / mean[k] for k, v in rounds.items()}
res["tail_fwd_bwd"] = {"ms_per_call_by_round": rounds, "ms_mean": mean, "spread_over_mean": spread, "fp8_over_bf16": mean["fp8"] / mean["bf16"],
                       "calls_per_round": a.tail_iters, "operand_sets_in_rotation": a.sets}
print(f"tail fwd+bwd at M = {M}: bf16 {mean['bf16']:.2f} ms (spread {spread['bf16']:.1%}), e4m3 {mean['fp8']:.2f} ms (spread {spread['fp8']:.1%}), "
      f"ratio {mean['fp8'] / mean['bf16']:.3f}", flush=True)

# ------------------------------------------------------------------------------------------------ 2. per kernel
res["tail_kernels"] = {}
for name, fp8 in (("bf16", False), ("fp8", True)):
    ops.TIMER = ops.KernelTimer()
    for i in range(a.sets):
        tail(sets[i], par, fp8)
    torch.cuda.synchronize()
    summ, ops.TIMER = ops.TIMER.summary(), None
    tab = {}
    for k, v in sorted(summ.items(), key=lambda kv: -kv[1]["total_ms"]):
        rate = v["work_per_launch"] / (v["avg_ms"] * 1e-3)
        tab[k] = {"launches": v["launches"], "avg_ms": v["avg_ms"], ("TFLOP_per_s" if v["unit"] == "flop" else "GB_per_s"): rate / (1e12 if v["unit"] == "flop" else 1e9)}
        print(f"  {name:5s} {k:32s} {v['launches']:3d} x {v['avg_ms']:7.3f} ms   {rate / 1e12:7.0f} TFLOP/s" if v["unit"] == "flop" else
              f"  {name:5s} {k:32s} {v['launches']:3d} x {v['avg_ms']:7.3f} ms   {rate / 1e9:7.0f} GB/s", flush=True)
    res["tail_kernels"][name] = tab
del sets, par
torch.cuda.empty_cache()

# ------------------------------------------------------------------------------------------------ 3. pair steps
torch.manual_seed(0)
model = bench.build_model(dict(vtr.COGVIDEOX_5B, num_layers=a.layers), dev, seed=0)
trainer = CogVideoXDPOTrainer({"lora_rank": 64, "lora_alpha": 128, "beta": 1.0, "accumulate_grad_batches": 1, "lean_activations": False, "seed": 1234}, transformer=model)
gB = torch.Generator(device=dev).manual_seed(1)
with torch.no_grad():
    for n, p in trainer.transformer.named_parameters():
        if ".lora_B." in n:
            p.normal_(0.0, 1e-3, generator=gB)
trainer.train()
engine = DPOEngine(trainer)
g = torch.Generator(device=dev).manual_seed(1234)
batch = {"x_pair": (0.7 * torch.randn(1, 2, C["frames"], 16, C["height"], C["width"], generator=g, device=dev)).to(torch.bfloat16),
         "prompt_emb": (0.2 * torch.randn(1, LT, 4096, generator=g, device=dev)).to(torch.bfloat16)}


def steps(fp8, n):
    model.enable_fp8(fp8)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(n):
        logs = engine.micro_step(batch)
    logs.update(engine.flush())
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, torch.cuda.max_memory_allocated() / 1e9, float(logs["train/loss"])


peak, loss = {}, {}
steps(False, 1)                             # warm-up of both paths (the first step also makes the optimizer state and the cached transposed weights)
_, peak["bf16_before_the_e4m3_weight_copies_exist"], _ = steps(False, 1)      # the copies stay resident once made, also while the switch is off
steps(True, 1)
rounds = {"bf16": [], "fp8": []}
for _ in range(a.rounds):
    for name, fp8 in (("bf16", False), ("fp8", True)):
        dt, peak[name], loss[name] = steps(fp8, a.steps)
        rounds[name].append(dt)
mean = {k: sum(v) / len(v) for k, v in rounds.items()}
spread = {k: (max(v) - min(v)) / mean[k] for k, v in rounds.items()}
res["pair_step"] = {"layers": a.layers, "note": "cfg2 geometry (49f x 480x720, 1 pair, LoRA r64)" + ("" if a.layers == 42 else f", reduced to {a.layers} of 42 blocks"),
                    "s_per_step_by_round": rounds, "s_mean": mean, "spread_over_mean": spread, "fp8_over_bf16": mean["fp8"] / mean["bf16"],
                    "peak_mem_GB": peak, "last_loss": loss, "steps_per_round": a.steps,
                    "e4m3_weight_copies_GB": 2 * 2 * D * INNER * a.layers / 1e9}
print(f"pair step, {a.layers} blocks: bf16 {mean['bf16']:.3f} s (spread {spread['bf16']:.1%}), e4m3 {mean['fp8']:.3f} s (spread {spread['fp8']:.1%}), "
      f"ratio {mean['fp8'] / mean['bf16']:.3f}; peak {peak['bf16']:.1f} / {peak['fp8']:.1f} GB", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({"out": a.out, "tail_fp8_over_bf16": res["tail_fwd_bwd"]["fp8_over_bf16"], "pair_step_fp8_over_bf16": res["pair_step"]["fp8_over_bf16"]}))
