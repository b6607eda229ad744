"""torch.autograd wrappers over the C-ABI HIP kernels.  PyTorch here is plumbing (device memory, streams,
autograd graph); every op below runs a hand-written gfx950 kernel through `_lib.call` and raises if it cannot."""
import contextlib as _contextlib
import contextvars as _contextvars
import ctypes
import os as _os

import torch

from . import _lib

_DT = {torch.float32: 0, torch.bfloat16: 1}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _req(t, dtype=None, contiguous=True):
    if not t.is_cuda:
        raise RuntimeError("videogpa_amd ops need GPU tensors (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"expected {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise RuntimeError("expected a contiguous tensor")
    return t


def _i64x3(*v):
    return (ctypes.c_int64 * 3)(*v)


class KernelTimer:
    """Optional HIP-event timing of individual kernel launches on the launch stream (bench.py's live roofline leg).
    Disabled (None) by default: zero overhead in the product path.

    Every event pair is a packet between two kernels that keeps the next launch from overlapping the tail of the previous one: timing all
    ~1500 launches of a cfg2 step costs 1.3 % of the step (2.301 vs 2.331 s).  `full_steps` / `always`: after `full_steps` calls of next_step()
    only the kernels named in `always` (the dominant ones the roofline is computed from) are still timed; the others were sampled on the
    first steps of the timed region and run unobserved afterwards."""

    def __init__(self, full_steps=None, always=()):
        self.records = {}
        self.full_steps, self.always = full_steps, frozenset(always)
        self.step = 0
        self.steps_seen = {}

    def next_step(self):
        self.step += 1

    def run(self, name, work, fn, unit="flop"):
        if self.full_steps is not None and self.step >= self.full_steps and name not in self.always:
            fn()
            return
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        self.records.setdefault(name, []).append((a, b, work, unit))
        self.steps_seen.setdefault(name, set()).add(self.step)

    def summary(self):
        out = {}
        for name, recs in self.records.items():
            ms = [a.elapsed_time(b) for a, b, _, _ in recs]
            work = sum(r[2] for r in recs) / len(recs)      # launches of one kernel can differ in size (q,k,v vs out LoRA)
            out[name] = {"launches": len(ms), "avg_ms": sum(ms) / len(ms), "total_ms": sum(ms), "work_per_launch": work,
                         "unit": recs[0][3], "steps": len(self.steps_seen[name])}
        return out


TIMER = None   # set to a KernelTimer() to time launches


def _timed(name, work, fn, unit="flop"):
    """work = algorithmic FLOPs (unit "flop", MFMA-bound kernels) or algorithmic HBM bytes = unique reads + writes
    (unit "byte", HBM-bound kernels) of the launch -- DESIGN.md section 4."""
    if TIMER is None:
        fn()
    else:
        TIMER.run(name, work, fn, unit)


# --------------------------------------------------------------------------------------------- DPO loss
class _DPOLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v_win, v_lose, v_win_ref, v_lose_ref, tgt_win, tgt_lose, beta, label_smoothing, loss_type, round_diff):
        ts = [v_win, v_lose, v_win_ref, v_lose_ref, tgt_win, tgt_lose]
        dt = v_win.dtype
        if dt not in _DT:
            raise RuntimeError(f"dpo_loss: unsupported dtype {dt}")
        ts = [_req(t.contiguous() if not t.is_contiguous() else t, dt) for t in ts]
        B = ts[0].shape[0]
        N = ts[0].numel() // B
        for t in ts:
            if t.shape != ts[0].shape:
                raise RuntimeError("dpo_loss: shape mismatch")
        dev = v_win.device
        out5 = torch.empty(5, dtype=torch.float32, device=dev)
        dlogit = torch.empty(B, dtype=torch.float32, device=dev)
        errs = torch.empty(B, 4, dtype=torch.float32, device=dev)
        ws_bytes = _lib.query("vgpa_dpo_loss_workspace_bytes", B)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        flags = 1 if round_diff else 0
        _lib.call("vgpa_dpo_loss_fwd", *ts, B, N, N, N, N, _DT[dt], float(beta), float(label_smoothing), int(loss_type), flags,
                  out5, dlogit, errs, ws, ws_bytes, _stream())
        ctx.save_for_backward(ts[0], ts[1], ts[4], ts[5], dlogit)
        ctx.meta = (B, N, _DT[dt], float(beta), flags)
        ctx.mark_non_differentiable(errs)
        return out5[0], out5[1], out5[2], out5[3], out5[4], errs

    @staticmethod
    def backward(ctx, g_loss, g_margin, g_wr, g_lr, g_acc, g_errs):
        v_win, v_lose, tgt_win, tgt_lose, dlogit = ctx.saved_tensors
        B, N, dt, beta, flags = ctx.meta
        gw = torch.empty_like(v_win)
        gl = torch.empty_like(v_lose)
        g = g_loss.to(torch.float32).contiguous()
        _lib.call("vgpa_dpo_loss_bwd", v_win, v_lose, tgt_win, tgt_lose, B, N, N, N, N, dt, beta, flags, dlogit, g, gw, gl, _stream())
        return gw, gl, None, None, None, None, None, None, None, None


def dpo_loss(v_win, v_lose, v_win_ref, v_lose_ref, tgt_win, tgt_lose, beta=1.0, label_smoothing=0.0, loss_type="sigmoid",
             round_diff=False):
    """-> (loss, reward_margin, winner_reward, loser_reward, accuracy, errs[B,4]); only `loss` carries grad
    (the reference's logged scalars are detached by use; train/loss.py:116-121)."""
    lt = {"sigmoid": 0, "hinge": 1}.get(loss_type)
    if lt is None:
        raise ValueError(f"Unknown loss type: {loss_type}")
    return _DPOLossFn.apply(v_win, v_lose, v_win_ref, v_lose_ref, tgt_win, tgt_lose, beta, label_smoothing, lt, round_diff)


class _DPOLossPairedFn(torch.autograd.Function):
    """Paired layout: v_pair / vref_pair / tgt_pair are [B,2,...] (win, lose); no de-interleaving copies."""

    @staticmethod
    def forward(ctx, v_pair, vref_pair, tgt_pair, beta, label_smoothing, loss_type, round_diff):
        dt = v_pair.dtype
        if dt not in _DT:
            raise RuntimeError(f"dpo_loss: unsupported dtype {dt}")
        for t in (v_pair, vref_pair, tgt_pair):
            _req(t, dt)
            if t.shape != v_pair.shape or t.shape[1] != 2:
                raise RuntimeError("dpo_loss_paired: expected [B,2,...] tensors of one shape")
        B = v_pair.shape[0]
        N = v_pair.numel() // (2 * B)
        dev = v_pair.device
        out5 = torch.empty(5, dtype=torch.float32, device=dev)
        dlogit = torch.empty(B, dtype=torch.float32, device=dev)
        errs = torch.empty(B, 4, dtype=torch.float32, device=dev)
        ws_bytes = _lib.query("vgpa_dpo_loss_workspace_bytes", B)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        flags = 1 if round_diff else 0
        _lib.call("vgpa_dpo_loss_fwd", v_pair[:, 0], v_pair[:, 1], vref_pair[:, 0], vref_pair[:, 1], tgt_pair[:, 0], tgt_pair[:, 1],
                  B, N, 2 * N, 2 * N, 2 * N, _DT[dt], float(beta), float(label_smoothing), int(loss_type), flags, out5, dlogit, errs, ws,
                  ws_bytes, _stream())
        ctx.save_for_backward(v_pair, tgt_pair, dlogit)
        ctx.meta = (B, N, _DT[dt], float(beta), flags)
        ctx.mark_non_differentiable(errs)
        return out5[0], out5[1], out5[2], out5[3], out5[4], errs

    @staticmethod
    def backward(ctx, g_loss, g_margin, g_wr, g_lr, g_acc, g_errs):
        v_pair, tgt_pair, dlogit = ctx.saved_tensors
        B, N, dt, beta, flags = ctx.meta
        gp = torch.empty_like(v_pair)
        g = g_loss.to(torch.float32).contiguous()
        _lib.call("vgpa_dpo_loss_bwd", v_pair[:, 0], v_pair[:, 1], tgt_pair[:, 0], tgt_pair[:, 1], B, N, 2 * N, 2 * N, 2 * N, dt, beta, flags,
                  dlogit, g, gp[:, 0], gp[:, 1], _stream())
        return gp, None, None, None, None, None, None


def dpo_loss_paired(v_pair, vref_pair, tgt_pair, beta=1.0, label_smoothing=0.0, loss_type="sigmoid", round_diff=False):
    lt = {"sigmoid": 0, "hinge": 1}.get(loss_type)
    if lt is None:
        raise ValueError(f"Unknown loss type: {loss_type}")
    return _DPOLossPairedFn.apply(v_pair, vref_pair, tgt_pair, beta, label_smoothing, lt, round_diff)


# --------------------------------------------------------------------------------------------- optimizer
def grad_norm(flat_grad, grad_scale=1.0, out=None):
    _req(flat_grad, torch.float32)
    out = torch.empty(1, dtype=torch.float32, device=flat_grad.device) if out is None else out
    ws_bytes = _lib.query("vgpa_grad_norm_workspace_bytes")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=flat_grad.device)
    _lib.call("vgpa_grad_norm", flat_grad, flat_grad.numel(), float(grad_scale), out, ws, ws_bytes, _stream())
    return out


def adamw_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_norm=0.0, total_norm=None):
    for t in (param, grad, exp_avg, exp_avg_sq):
        _req(t, torch.float32)
    _lib.call("vgpa_adamw_step", param, grad, exp_avg, exp_avg_sq, param.numel(), float(lr), float(beta1), float(beta2), float(eps),
              float(weight_decay), int(step), float(grad_scale), float(max_norm), total_norm, _stream())


# --------------------------------------------------------------------------------------------- noise / velocity
def noise_velocity_paired(x_pair, noise, t, sqrt_abar, sqrt_1m_abar):
    """x_pair [B,2,...], noise [B,...] (shared by the pair), t [B] int64 -> (x_noisy_pair, v_target_pair)."""
    dt = x_pair.dtype
    _req(x_pair, dt), _req(noise, dt), _req(t, torch.int64), _req(sqrt_abar, torch.float32), _req(sqrt_1m_abar, torch.float32)
    B = x_pair.shape[0]
    if x_pair.shape[1] != 2 or x_pair.shape[2:] != noise.shape[1:] or noise.shape[0] != B:
        raise RuntimeError("noise_velocity_paired: expected x_pair [B,2,...] and noise [B,...]")
    N = noise.numel() // B
    xt = torch.empty_like(x_pair)
    v = torch.empty_like(x_pair)
    _lib.call("vgpa_noise_velocity_paired", x_pair, noise, t, sqrt_abar, sqrt_1m_abar, B, N, sqrt_abar.numel(), _DT[dt], xt, v, _stream())
    return xt, v


def flow_sigma(timesteps, num_train_timesteps=1000, shift=5.0):
    """get_sigma_from_timestep (train/Wan2.2-TI2V-5B/03_train.py:103-106)."""
    s = timesteps.float() / num_train_timesteps
    return shift * s / (1 + (shift - 1) * s)


def flow_noise_velocity_paired(x_pair, noise, sigma, xt_fp32=True):
    """Flow-matching noising + velocity target over the paired layout: x_pair [B,2,...], noise [B,...], sigma [B] fp32 ->
    (x_t pair [fp32 like the reference's promoted result, or latent dtype], v-target pair = noise - x)."""
    dt = x_pair.dtype
    _req(x_pair, dt), _req(noise, dt), _req(sigma, torch.float32)
    B = x_pair.shape[0]
    N = noise.numel() // B
    xt = torch.empty(x_pair.shape, dtype=torch.float32 if (xt_fp32 or dt == torch.float32) else dt, device=x_pair.device)
    v = torch.empty_like(x_pair)
    _lib.call("vgpa_flow_noise_velocity_paired", x_pair, noise, sigma, B, N, _DT[dt], 1 if xt.dtype == torch.float32 else 0, xt, v, _stream())
    return xt, v


# --------------------------------------------------------------------------------------------- sampler step of the generate loop
def sampler_step(v, x, coef, guidance_scale=None, x0_old=None, noise=None, image_latents=None, out=None):
    """One pass of csrc/sampler.hip behind the transformer: guidance, the v-prediction data estimate, the scheduler's update and the next input.
        v = v_u + g (v_c - v_u)  (guidance_scale given: v is [2B, ...] = [uncond | cond]; None: v [B, ...] as it is),   x0 = sa x - sb v,
        x_next = k_x x + k_0 x0 + k_old x0_old + k_n noise
    `coef` is a scheduler's step_coefficients(i) (Python floats; k_old / k_n None leave the term out, and then x0_old / noise are not read).
    v: the model output in its own dtype (bf16 | fp32); x, noise, image_latents [B,F,C_img,h,w]: the latent dtype; x0_old: fp32.
    -> (x_next [latent dtype], x0 [fp32], packed): packed is None without image_latents, else the next transformer input
    [G*B, F, C + C_img, h, w] (G = 2 under guidance) = cat([cat([x_next] * G), cat([image_latents] * G)], dim=2), written by the same pass.
    `out`: an (x_next, x0, packed) triple of a previous call to write into (none of them may be an input of this call)."""
    _req(v), _req(x)
    if x.dim() != 5:
        raise RuntimeError(f"sampler_step: x is [B,F,C,h,w], got {tuple(x.shape)}")
    B, F, C, h, w = x.shape
    G = 1 if guidance_scale is None else 2
    if tuple(v.shape) != (G * B, F, C, h, w):
        raise RuntimeError(f"sampler_step: v {tuple(v.shape)} is not [{G * B},{F},{C},{h},{w}]")
    use_old, use_noise = coef["k_old"] is not None, coef["k_n"] is not None
    if use_old:
        if x0_old is None or tuple(_req(x0_old, torch.float32).shape) != tuple(x.shape):
            raise RuntimeError("sampler_step: these coefficients use the history: x0_old must be fp32 of x's shape")
    if use_noise:
        if noise is None or tuple(_req(noise, x.dtype).shape) != tuple(x.shape):
            raise RuntimeError("sampler_step: these coefficients use noise: it must have x's shape and dtype")
    C_img = 0
    if image_latents is not None:
        _req(image_latents, x.dtype)
        C_img = image_latents.shape[2] if image_latents.dim() == 5 else 0
        if tuple(image_latents.shape) != (B, F, C_img, h, w) or C_img == 0:
            raise RuntimeError(f"sampler_step: image_latents {tuple(image_latents.shape)} is not [{B},{F},C_img,{h},{w}]")
    if out is None:
        out = (torch.empty_like(x), torch.empty(x.shape, dtype=torch.float32, device=x.device),
               None if image_latents is None else torch.empty(G * B, F, C + C_img, h, w, dtype=x.dtype, device=x.device))
    x_next, x0, packed = out
    _lib.call("vgpa_sampler_step", v, _dtype_code(v.dtype, "sampler_step"), G - 1, x, x0_old if use_old else None, noise if use_noise else None,
              image_latents, B, F, C, C_img, h * w, _dtype_code(x.dtype, "sampler_step"), float(guidance_scale or 0.0), coef["sa"], coef["sb"],
              coef["k_x"], coef["k_0"], coef["k_old"] or 0.0, coef["k_n"] or 0.0, x_next, x0, packed, G, _stream())
    return x_next, x0, packed


# --------------------------------------------------------------------------------------------- PIL-exact image resize (csrc/preprocess.hip)
RESIZE_FILTERS = {"bicubic": 0, "lanczos": 1}


def image_resize(frames, out_h, out_w, filter="lanczos"):
    """uint8 [T,H,W,3] -> uint8 [T,out_h,out_w,3] = PIL `Image.resize((out_w, out_h), BICUBIC | LANCZOS)` of every frame, bit for bit (Pillow's 8-bit
    ImagingResample: two passes, 22-bit fixed weights, a clip after each pass)"""
    _req(frames, torch.uint8)
    if frames.dim() != 4 or frames.shape[-1] != 3 or filter not in RESIZE_FILTERS:
        raise RuntimeError(f"image_resize: expected uint8 [T,H,W,3] and a filter of {sorted(RESIZE_FILTERS)}, got {tuple(frames.shape)}, {filter!r}")
    T, H, W, _ = frames.shape
    code = RESIZE_FILTERS[filter]
    out = torch.empty(T, int(out_h), int(out_w), 3, dtype=torch.uint8, device=frames.device)
    ws_bytes = _lib.query("vgpa_image_resize_workspace_bytes", T, H, W, int(out_h), int(out_w), code)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=frames.device)
    _lib.call("vgpa_image_resize", frames, T, H, W, int(out_h), int(out_w), code, out, ws, ws_bytes, _stream())
    return out


def image_to_pm1(frames, dtype=torch.float32):
    """uint8 [T,H,W,3] -> [T,3,H,W] in `dtype` (fp32 | bf16) = x / 255 * 2 - 1, formed in fp32 in that order and rounded once (diffusers
    VaeImageProcessor: pil_to_numpy / 255, then normalize 2 x - 1)"""
    _req(frames, torch.uint8)
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise RuntimeError(f"image_to_pm1: expected uint8 [T,H,W,3], got {tuple(frames.shape)}")
    T, H, W, _ = frames.shape
    out = torch.empty(T, 3, H, W, dtype=dtype, device=frames.device)
    _lib.call("vgpa_image_to_pm1", frames, T, H, W, _dtype_code(dtype, "image_to_pm1"), out, _stream())
    return out


# --------------------------------------------------------------------------------------------- Depth Anything 3 input processing (csrc/da3_input.hip)
DA3_RESIZE_MODES = {"area": 0, "cubic": 1}


def _da3_frames(frames, name):
    _req(frames, torch.uint8)
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise RuntimeError(f"{name}: expected uint8 [T,H,W,3], got {tuple(frames.shape)}")
    return frames.shape[:3]


def _da3_pair(frames, T, h, w, table):
    _req(table, torch.uint8)
    if tuple(table.shape) != (3, 256):
        raise RuntimeError(f"processed_images table: expected uint8 [3,256], got {tuple(table.shape)}")
    return (torch.empty(1, T, 3, h, w, dtype=torch.float32, device=frames.device), torch.empty(T, h, w, 3, dtype=torch.uint8, device=frames.device))


def da3_resize(frames, out_h, out_w, mode, table=None):
    """uint8 [T,H,W,3] -> cv2.resize(frame, (out_w, out_h), INTER_AREA | INTER_CUBIC) of every frame, OpenCV's 8-bit semantics restated (the header of
    csrc/da3_input.hip says which).  Without `table`: uint8 [T,out_h,out_w,3].  With `table` (uint8 [3,256] on the device, da3_input.processed_table) the
    last stage is the resize's epilogue: (x fp32 [1,T,3,out_h,out_w] ImageNet-normalised, processed_images uint8 [T,out_h,out_w,3]), the resized uint8
    image never written.  "area" refuses out > in (RuntimeError, nothing launched)."""
    T, H, W = _da3_frames(frames, "da3_resize")
    if mode not in DA3_RESIZE_MODES:
        raise RuntimeError(f"da3_resize: mode is one of {sorted(DA3_RESIZE_MODES)}, got {mode!r}")
    code, out_h, out_w = DA3_RESIZE_MODES[mode], int(out_h), int(out_w)
    if table is None:
        out, x, proc = torch.empty(T, out_h, out_w, 3, dtype=torch.uint8, device=frames.device), None, None
    else:
        out, (x, proc) = None, _da3_pair(frames, T, out_h, out_w, table)
    ws_bytes = _lib.query("vgpa_da3_resize_workspace_bytes", H, W, out_h, out_w, code)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=frames.device)
    _lib.call("vgpa_da3_resize", frames, T, H, W, out_h, out_w, code, out, x, proc, table, ws, ws_bytes, _stream())
    return out if table is None else (x, proc)


def da3_normalize(frames, table, box=None):
    """The last stage alone: uint8 [T,H,W,3] and an optional crop box (top, left, h, w) -> (x fp32 [1,T,3,h,w] = ToTensor then Normalize in torchvision's
    order and roundings, processed_images uint8 [T,h,w,3] = table[c][u]) in one launch"""
    T, H, W = _da3_frames(frames, "da3_normalize")
    top, left, h, w = (0, 0, H, W) if box is None else (int(v) for v in box)
    x, proc = _da3_pair(frames, T, h, w, table)
    _lib.call("vgpa_da3_normalize", frames, T, H, W, top, left, h, w, x, proc, table, _stream())
    return x, proc


# --------------------------------------------------------------------------------------------- AdaLN-Zero pieces
class _LNModulateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ln_w, ln_b, mod, text_len, eps):
        # x [B,S,D] bf16; ln_w/ln_b fp32 [D]; mod fp32 [B,4,D] = (shift_v, 1+scale_v, shift_t, 1+scale_t) or None
        _req(x, torch.bfloat16), _req(ln_w, torch.float32), _req(ln_b, torch.float32)
        B, S, D = x.shape
        out = torch.empty_like(x)
        mean = torch.empty(B, S, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        if mod is not None:
            _req(mod, torch.float32)
            sv, s1v, st, s1t = mod[:, 0], mod[:, 1], mod[:, 2], mod[:, 3]
            stride = mod.stride(0)
        else:
            sv = s1v = st = s1t = None
            stride = 0
        _lib.call("vgpa_ln_modulate_fwd", x, ln_w, ln_b, sv, s1v, st, s1t, stride, B, S, D, text_len, float(eps), out, mean, rstd, _stream())
        ctx.save_for_backward(x, mean, rstd, ln_w, mod)
        ctx.text_len = text_len
        return out

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, ln_w, mod = ctx.saved_tensors
        B, S, D = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        if mod is not None:
            s1v, s1t, stride = mod[:, 1], mod[:, 3], mod.stride(0)
        else:
            s1v = s1t = None
            stride = 0
        _lib.call("vgpa_ln_modulate_bwd", dy, x, mean, rstd, ln_w, s1v, s1t, stride, B, S, D, ctx.text_len, None, dx, _stream())
        return dx, None, None, None, None, None


def ln_modulate(x, ln_w, ln_b, mod=None, text_len=0, eps=1e-5, n_pad=0):
    return _ResidualLNFn.apply(x, None, None, ln_w, ln_b, mod, text_len, eps, n_pad, 0)[1]


def ln_modulate_recompute(x, ln_w, ln_b, mod=None, text_len=0, eps=1e-5):
    """The LN-modulate output again, outside autograd: the residual+LN kernel with no residual branch normalises the (already bf16) x exactly
    as the fused pass that produced it did, so the result is bit-identical to the n that pass returned (lean activations)."""
    B, S, D = x.shape
    n = torch.empty_like(x)
    mean = torch.empty(B, S, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    sv, s1v, st, s1t, mstride = _mod_ptrs(mod)
    _timed("ln_modulate_fwd", 4.0 * B * S * D, lambda: _lib.call("vgpa_residual_ln_fwd", x, None, None, None, 0, ln_w, ln_b, sv, s1v, st, s1t, mstride, B, S, D,
                                                                  text_len, float(eps), None, n, D, mean, rstd, _stream()), "byte")
    return n


def ln_modulate_v1(x, ln_w, ln_b, mod=None, text_len=0, eps=1e-5):
    """First-generation LN-modulate kernels (kept for A/B and as a second implementation under test)."""
    return _LNModulateFn.apply(x, ln_w, ln_b, mod, text_len, eps)


def _mod_ptrs(mod):
    if mod is None:
        return None, None, None, None, 0
    return mod[:, 0], mod[:, 1], mod[:, 2], mod[:, 3], mod.stride(0)


class _ResidualLNFn(torch.autograd.Function):
    """(x, y) -> (x_new = x + gate*y, n = LN(x_new)*alpha + beta) in one pass; backward fuses the residual-path add, the
    LN backward and the gate multiply.  y / gates may be None: plain LN-modulate of x (x_new is then x itself)."""

    @staticmethod
    def forward(ctx, x, y, gates, ln_w, ln_b, mod, text_len, eps, n_pad, dy_pad):
        """n_pad: n is returned as the first D columns of a fresh [B,S,D+n_pad] buffer (its consumer, linear_lora_ext, puts the
        LoRA down-projections into the tail and runs ONE GEMM over K = D+n_pad); dy_pad: the same for the gradient of y."""
        _req(x, torch.bfloat16), _req(ln_w, torch.float32), _req(ln_b, torch.float32)
        B, S, D = x.shape
        n = _padded_empty((B, S), D, n_pad, x.dtype, x.device) if n_pad else _empty_rows(x.shape, x.dtype, x.device)
        mean = torch.empty(B, S, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        sv, s1v, st, s1t, mstride = _mod_ptrs(mod)
        if y is not None:
            _req(y, torch.bfloat16), _req(gates, torch.float32)
            x_new = torch.empty_like(x)
            gv, gt, gstride = gates[:, 0], gates[:, 1], gates.stride(0)
        else:
            x_new, gv, gt, gstride = None, None, None, 0
        _timed("residual_ln_fwd" if y is not None else "ln_modulate_fwd", (8.0 if y is not None else 4.0) * B * S * D,
               lambda: _lib.call("vgpa_residual_ln_fwd", x, y, gv, gt, gstride, ln_w, ln_b, sv, s1v, st, s1t, mstride, B, S, D, text_len,
                                 float(eps), x_new, n, D + n_pad, mean, rstd, _stream()), "byte")
        xs = x if y is None else x_new
        ctx.save_for_backward(xs, mean, rstd, ln_w, mod, gates if y is not None else None)
        ctx.text_len = text_len
        ctx.has_y = y is not None
        ctx.dy_pad = dy_pad
        return x_new, n          # x_new is None when there is no y (plain LN-modulate)

    @staticmethod
    def backward(ctx, dx_new, dn):
        xs, mean, rstd, ln_w, mod, gates = ctx.saved_tensors
        B, S, D = xs.shape
        if dn is None:
            dn = torch.zeros_like(xs)
        dn = dn.contiguous()
        dres = None if dx_new is None else dx_new.contiguous()
        dx = torch.empty_like(xs)
        _, s1v, _, s1t, mstride = _mod_ptrs(mod)
        dyp = ctx.dy_pad
        if ctx.has_y:
            dy = _padded_empty((B, S), D, dyp, xs.dtype, xs.device) if dyp else _empty_rows(xs.shape, xs.dtype, xs.device)
            gv, gt, gstride = gates[:, 0], gates[:, 1], gates.stride(0)
        else:
            dy, gv, gt, gstride = None, None, None, 0
        passes = 3 + (1 if dres is not None else 0) + (1 if ctx.has_y else 0)     # dn, x, dx (+ dres) (+ dy)
        _timed("residual_ln_bwd" if ctx.has_y else "ln_modulate_bwd", 2.0 * passes * B * S * D,
               lambda: _lib.call("vgpa_residual_ln_bwd", dn, xs, mean, rstd, ln_w, s1v, s1t, mstride, gv, gt, gstride, dres, B, S, D,
                                 ctx.text_len, dx, dy, D + dyp, _stream()), "byte")
        return dx, dy, None, None, None, None, None, None, None, None


def residual_ln(x, y, gates, ln_w, ln_b, mod=None, text_len=0, eps=1e-5, n_pad=0, dy_pad=0):
    """-> (x + gate*y, LN-modulate of that).  One HIP pass forward, one backward."""
    return _ResidualLNFn.apply(x, y, gates, ln_w, ln_b, mod, text_len, eps, n_pad, dy_pad)


class _GateResidualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, gates, text_len):
        # out = x + gate[range] * y ; gates fp32 [B,2,D] = (gate_v, gate_t)
        _req(x, torch.bfloat16), _req(y, torch.bfloat16), _req(gates, torch.float32)
        B, S, D = x.shape
        out = torch.empty_like(x)
        _lib.call("vgpa_gate_residual", x, y, gates[:, 0], gates[:, 1], gates.stride(0), B, S, D, text_len, out, _stream())
        ctx.save_for_backward(gates)
        ctx.text_len = text_len
        return out

    @staticmethod
    def backward(ctx, dout):
        (gates,) = ctx.saved_tensors
        dout = dout.contiguous()
        B, S, D = dout.shape
        dy = _empty_rows(dout.shape, dout.dtype, dout.device)
        _lib.call("vgpa_gate_residual", None, dout, gates[:, 0], gates[:, 1], gates.stride(0), B, S, D, ctx.text_len, dy, _stream())
        return dout, dy, None, None


def gate_residual(x, y, gates, text_len):
    return _GateResidualFn.apply(x, y, gates, text_len)


class _GeluTanhFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u):
        _req(u, torch.bfloat16)
        out = _empty_rows(u.shape, u.dtype, u.device, wide=True)      # feeds the long-K down-projection
        _timed("gelu_tanh_fwd", 4.0 * u.numel(), lambda: _lib.call("vgpa_gelu_tanh_fwd", u, u.numel(), out, _stream()), "byte")
        ctx.save_for_backward(u)
        return out

    @staticmethod
    def backward(ctx, dy):
        (u,) = ctx.saved_tensors
        dy = dy.contiguous()
        du = _empty_rows(u.shape, u.dtype, u.device, wide=True)
        _timed("gelu_tanh_bwd", 6.0 * u.numel(), lambda: _lib.call("vgpa_gelu_tanh_bwd", u, dy, u.numel(), du, _stream()), "byte")
        return du


def gelu_tanh(u):
    return _GeluTanhFn.apply(u)


# --------------------------------------------------------------------------------------------- linear (+ LoRA)
def _pad_rank(r):
    rp = 16
    while rp < r:
        rp *= 2
    return rp


def lora_down(x2, a_cat, out=None):
    """T[M,R] = x2[M,K] @ a_cat[R,K]^T on MFMA (x2 may be a column slice: row stride = x2.stride(0))."""
    M, K = x2.shape
    R = a_cat.shape[0]
    t = torch.empty(M, R, dtype=torch.bfloat16, device=x2.device) if out is None else out
    _timed("lora_down_kernel", 2.0 * M * (K + R), lambda: _lib.call("vgpa_lora_down", x2, x2.stride(0), a_cat, t, t.stride(0), M, K, R, _stream()),
           "byte")
    return t


def lora_up_add(y2, t, bw, s, accumulate=True):
    """y2[M,N] (+)= s * t[M,rp] @ bw[N,rp]^T in place (y2 / t may be column slices)."""
    M, N = y2.shape
    _timed("lora_up_add_kernel", (4.0 if accumulate else 2.0) * M * N + 2.0 * M * t.shape[1],
           lambda: _lib.call("vgpa_lora_up_add", y2, y2.stride(0), t, t.stride(0), bw, bw.stride(0), float(s), M, N, t.shape[1],
                             1 if accumulate else 0, _stream()), "byte")


def lora_grad(u, v, s=1.0):
    """fp32 G[P,Q] = s * u[M,P]^T @ v[M,Q] (contraction over tokens)."""
    M, P = u.shape
    Q = v.shape[1]
    g = torch.empty(P, Q, dtype=torch.float32, device=u.device)
    ws_bytes = _lib.query("vgpa_lora_grad_workspace_bytes", M, P, Q)       # per-row-range partials + ordered merge: bit-reproducible
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=u.device)
    _timed("lora_grad_kernel", 2.0 * M * (P + Q), lambda: _lib.call("vgpa_lora_grad_ws", u, u.stride(0), v, v.stride(0), g, Q, float(s), M, P, Q,
                                                                     ws, ws_bytes, _stream()), "byte")
    return g


# ---------------------------------------------------------------------------------------------------------------- vendor-GEMM solution selection
# The dense projections are hipBLASLt's (north_star: MFMA by hand for attention and LoRA only): 31 % of the cfg2 step.  torch asks hipBLASLt's heuristic for ONE
# solution per shape; the library holds hundreds that are valid for it.  tools/gemm_tune.py times every one of them at the shapes of the step (PyTorch TunableOp:
# the same hipblasLtMatmul call, algo chosen by index) and writes the winners to videogpa_amd/tuned/tunableop_gfx950.csv; use_tuned_gemms() makes torch pick them.
# The file is keyed by (torch, ROCm, hipBLASLt versions, gfx arch): on any other stack torch ignores it and the default heuristic runs -- never a wrong kernel.
TUNED_GEMM_FILE = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "tuned", "tunableop_gfx950.csv")
_TUNED_GEMMS = None          # None: undecided; else {"enabled": bool, "file": path | None, "entries": int}


def use_tuned_gemms(enabled=True, path=None):
    """Select the vendor-GEMM solutions found by tools/gemm_tune.py (PyTorch TunableOp reading a results file, tuning itself OFF: an unknown shape runs the default
    heuristic's kernel).  Called once by the trainers (config key "tuned_gemms", default True); process-wide because torch's GEMM dispatch is.  -> the decision, logged
    by the caller.  A process that already runs TunableOp its own way (PYTORCH_TUNABLEOP_ENABLED set) is left alone."""
    global _TUNED_GEMMS
    import torch.cuda.tunable as tn
    if _os.environ.get("PYTORCH_TUNABLEOP_ENABLED") is not None:
        gpu = torch.cuda.is_available()
        _TUNED_GEMMS = {"enabled": tn.is_enabled() if gpu else False, "file": tn.get_filename() if gpu else None, "entries": None,
                        "note": "PYTORCH_TUNABLEOP_* set by the caller: left as is"}
        return _TUNED_GEMMS
    path = path or TUNED_GEMM_FILE
    if not torch.cuda.is_available():
        _TUNED_GEMMS = {"enabled": False, "file": None, "entries": 0}
        return _TUNED_GEMMS
    if not enabled or not _os.path.isfile(path):
        if _TUNED_GEMMS is not None and _TUNED_GEMMS.get("enabled"):
            tn.enable(False)
        _TUNED_GEMMS = {"enabled": False, "file": None, "entries": 0}
        return _TUNED_GEMMS
    if _TUNED_GEMMS is not None and _TUNED_GEMMS.get("enabled") and _TUNED_GEMMS.get("file") == path:
        return _TUNED_GEMMS
    with open(path) as f:
        entries = sum(1 for ln in f if ln.startswith(("Gemm", "ScaledGemm")))
    tn.enable(True)
    tn.tuning_enable(False)
    tn.record_untuned_enable(False)
    tn.set_filename(path, False)
    _TUNED_GEMMS = {"enabled": True, "file": path, "entries": entries}
    return _TUNED_GEMMS


def tuned_gemms_state():
    return _TUNED_GEMMS


# dX = dY W of a frozen projection: torch.autograd issues it as an "NN" GEMM, which hipBLASLt runs 4-25 % slower at these
# shapes than the "TN" form x W^T (tools/gemm_bench.py: fused q,k,v 1.91 -> 1.44 ms, FF 2.24 -> 2.07 / 2.08 -> 1.89 ms).  The
# base weights never change during LoRA training, so a transposed copy is kept next to each weight (11 GB for CogVideoX-5B,
# made at the first backward) and dX is computed as dY (W^T)^T.
# Dispatch constants below (this one, GEMM_SPLIT_*, GEMM_ROW_SLACK, ATTN_*) are MODULE constants: a measurement tool flips them from Python before its first call
# (tools/*.py); nothing here reads the environment.  The environment carries only the three model-level settings -- VGPA_PRECISE_DELTA (default of the per-model
# precise_delta), VGPA_DP_COLLECTIVE (optim.FlatAdamW), lean activations are a trainer config key -- plus VGPA_LIB (which build of the library to load) and
# VGPA_FORCE_DIST (run the N > 1 code path on one GPU: tests).
_WT_CACHE = True


def _transposed(W):
    if not _WT_CACHE:
        return None
    c = getattr(W, "_vgpa_wt", None)
    if c is None or c[0] != W._version or c[1].device != W.device or c[1].dtype != W.dtype:
        c = (W._version, W.detach().t().contiguous())
        W._vgpa_wt = c          # lives and dies with the weight tensor
    return c[1]


# Rows per vendor-GEMM call (0 = one call).  hipBLASLt's bf16 kernels lose ~10 % at M = 36 960 (two Wan2.2 samples as one batch) against two calls of
# M = 18 480, also inside the power-limited step: cfg5 bf16 GEMMs 300 -> 272 ms per step, measured A/B in one session (profiles/r04_gemm_split_ab.txt);
# at the CogVideoX shapes (M = 35 552) the same split changes nothing or costs (feed-forward shapes: +20 ms), and the fp8 GEMMs do not care.  So the
# split is set by the model that knows its rows per sample (WanModel.forward) and applies only to row counts that are a multiple of it.
# GEMM_SPLIT_OVERRIDE (tools: an int overrides the models' choice, 0 = never split); GEMM_SPLIT_EXT_ONLY restricts the split to the LoRA-extended GEMMs.
GEMM_SPLIT_OVERRIDE = None
GEMM_SPLIT_EXT_ONLY = False
# The setting is SCOPED, not process state: a model wraps its forward in `with gemm_rows_per_call(L):` (a contextvar: other models / threads of the process
# see 0), every autograd node below records the value it ran its forward GEMM with (ctx.rows_per_call) and runs its backward GEMMs with the same one -- the
# autograd engine's threads never consult the context.  A checkpointed block re-enters the context in its recomputation (WanModel.forward).
_GEMM_ROWS = _contextvars.ContextVar("vgpa_gemm_rows_per_call", default=0)


@_contextlib.contextmanager
def gemm_rows_per_call(rows):
    """for the duration of a model's forward: vendor GEMMs whose row count is a multiple (>= 2x) of `rows` run one call per `rows` rows (0: one call)"""
    tok = _GEMM_ROWS.set(int(rows))
    try:
        yield
    finally:
        _GEMM_ROWS.reset(tok)


def current_gemm_rows():
    return int(GEMM_SPLIT_OVERRIDE) if GEMM_SPLIT_OVERRIDE is not None else _GEMM_ROWS.get()


def _slack_rows(x2):
    """rows of [M, K] storage behind x2 that _empty_rows (directly, or under a _padded_empty head view) allocated for the vendor GEMM to run over: the
    row count it may cover (>= M), or M when x2 is anything else -- a caller's view of some other buffer is never read or written past its shape."""
    base = x2 if x2._base is None else x2._base
    tag = getattr(base, "_vgpa_rows", None)
    if tag is None or x2.dim() != 2 or x2.stride(1) != 1:
        return x2.shape[0]
    rows, Mp, width = tag          # logical rows, storage rows, row width of the buffer
    if x2.shape[0] != rows or x2.stride(0) != width or x2.data_ptr() != base.data_ptr() or x2.shape[1] > width:
        return x2.shape[0]
    return Mp


def _linear_rows(x2, W, bias, ext=False, split=0):
    M = x2.shape[0]
    if GEMM_ROW_SLACK and 16384 <= M <= 65536 and x2.is_cuda and x2.dim() == 2 and x2.stride(1) == 1 and (split <= 0 or M % split):
        # the operand was allocated with row slack (_empty_rows, recognised by its tag): run the GEMM over the padded row count -- rows are independent, the
        # extra output rows are never read -- because hipBLASLt is 1-17 % faster at M = 35 840 / 36 864 than at 35 552 (tools/gemm_m_probe.py)
        room = _slack_rows(x2)
        for Mp in (gemm_rows(M, W.shape[0], W.shape[1]), gemm_rows(M)):
            if M < Mp <= room:
                xp = torch.as_strided(x2, (Mp, x2.shape[1]), x2.stride(), x2.storage_offset())
                return torch.nn.functional.linear(xp, W, bias)[:M]
    if split <= 0 or M < 2 * split or M % split or not x2.is_cuda or x2.dim() != 2 or (GEMM_SPLIT_EXT_ONLY and not ext):
        return torch.nn.functional.linear(x2, W, bias)
    out = torch.empty(M, W.shape[0], dtype=x2.dtype, device=x2.device)
    for a in range(0, M, split):
        b = a + split
        if bias is None:
            torch.mm(x2[a:b], W.t(), out=out[a:b])
        else:
            torch.addmm(bias, x2[a:b], W.t(), out=out[a:b])
    return out


def _gemm(x2, W, bias=None, ext=False, split=None):
    """x2 [M,K] @ W[N,K]^T (+ bias) through hipBLASLt (torch), timed like the hand-written kernels when bench.py asks for it.  split: rows per call
    (None: the enclosing gemm_rows_per_call context -- forward passes; backward passes hand in what their node recorded)."""
    split = current_gemm_rows() if split is None else split
    if TIMER is None:
        return _linear_rows(x2, W, bias, ext, split)
    out = []
    _timed("hipblaslt_gemm (vendor)", 2.0 * x2.shape[0] * W.shape[0] * W.shape[1], lambda: out.append(_linear_rows(x2, W, bias, ext, split)))
    return out[0]


def _frozen_dx(dy2, W, split=0):
    Wt = _transposed(W)
    return dy2 @ W if Wt is None else _gemm(dy2, Wt, split=split)


class _FrozenLinearFn(torch.autograd.Function):
    """y = x W^T + b with W, b frozen: backward is dX only, through the cached transposed weight."""

    @staticmethod
    def forward(ctx, x, W, bias):
        ctx.save_for_backward(W)
        ctx.rows_per_call = current_gemm_rows()
        return _gemm(x.reshape(-1, x.shape[-1]), W, bias, split=ctx.rows_per_call).view(*x.shape[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, dy):
        (W,) = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        if dy2.stride(1) != 1:
            dy2 = dy2.contiguous()
        return _frozen_dx(dy2, W, ctx.rows_per_call).view(*dy.shape[:-1], W.shape[1]), None, None


def frozen_linear(x, W, bias):
    """F.linear for a projection whose weight / bias do not train (falls back to F.linear otherwise)."""
    if W.requires_grad or (bias is not None and bias.requires_grad):
        return torch.nn.functional.linear(x, W, bias)
    if not (torch.is_grad_enabled() and x.requires_grad):
        return _gemm(x.reshape(-1, x.shape[-1]), W, bias).view(*x.shape[:-1], W.shape[0])
    return _FrozenLinearFn.apply(x, W, bias)


# The fused AdamW kernel writes adapter values through raw pointers (no autograd version bump): FlatAdamW.step calls
# bump_adapter_epoch() so that the bf16 copies below are refreshed exactly once per optimizer step.
ADAPTER_EPOCH = 0


def bump_adapter_epoch():
    global ADAPTER_EPOCH
    ADAPTER_EPOCH += 1


# Row slack for vendor-GEMM operands.  hipBLASLt's bf16 kernels are markedly faster when the row count is a multiple of 1024 (35 840 instead of cfg2's 35 552:
# fused q/k/v projection -6.7 %, attention-out projection -17 %, FF1 -2 %, for 0.8 % more rows; tools/gemm_m_probe.py, profiles/r04_gemm_m_probe.txt).  GEMM rows are
# independent, so the activation buffers that feed GEMMs are allocated with that many rows of STORAGE (logical shape unchanged, contents of the slack never read
# by anything but the GEMM, whose extra output rows nobody reads) and _linear_rows runs over the padded count.  Only when the padding is <= 1.25 % of the rows.
GEMM_ROW_SLACK = True


def gemm_rows(M, N=None, K=None, wide=False):
    """the row count a vendor GEMM with M real rows is run over.  Multiples of 1024 when that costs <= 1.25 % more rows; the long-K, narrow-N shape
    (feed-forward down-projection and the dX of the up-projection: N = 3072, K = 12 288) is 5 % faster still at a multiple of 4096 (36 864 for
    35 552: profiles/r04_gemm_m_probe.txt), taken when it costs <= 4 %.  wide=True: the largest count any shape may ask for (allocation size)."""
    if not GEMM_ROW_SLACK or M < 16384 or M > 65536:      # measured: gain at 35 552 rows (cfg2 / cfg3), loss at 82 052 (cfg4: 82 944 rows cost +26 ms of GEMM time per step)
        return M
    Mp = (M + 1023) // 1024 * 1024
    Mp = Mp if (Mp - M) * 80 <= M else M
    if wide or (K is not None and N is not None and K >= 8192 and N <= 4096 and K >= 3 * N):
        Mw = (M + 4095) // 4096 * 4096
        if (Mw - M) * 25 <= M:
            return Mw
    return Mp


def _empty_rows(shape, dtype, device, wide=False):
    """torch.empty(shape) whose storage has room for gemm_rows(rows) rows of the last dimension (rows = product of the leading dimensions); not a view"""
    shape = tuple(int(v) for v in shape)
    rows = 1
    for v in shape[:-1]:
        rows *= v
    Mp = gemm_rows(rows, wide=wide)
    if Mp == rows or str(device).startswith("cpu"):
        return torch.empty(shape, dtype=dtype, device=device)
    t = torch.empty(Mp * shape[-1], dtype=dtype, device=device)
    t = t.resize_(shape)
    t._vgpa_rows = (rows, Mp, shape[-1])      # what _slack_rows recognises: ONLY buffers made here are ever run past their logical row count
    return t


def _padded_empty(shape, D, pad, dtype, device):
    """A fresh [..., D + pad] buffer whose tail is zero, marked as a padded operand buffer; returns its [..., :D] head view.  The
    producers of LoRA-carrying GEMM operands (residual_ln, attention, their backwards) allocate through this; `_padded_base`
    recognises ONLY buffers made here (a caller's slice of some wider tensor is never written into)."""
    buf = _empty_rows((*shape, D + pad), dtype, device)
    buf[..., D:].zero_()          # fresh tensor, no autograd history: the reference pass's LoRA tail is zero without touching a view later
    buf._vgpa_pad = (D, pad)
    return buf[..., :D]


def _padded_base(t2, width):
    """If the 2-D tensor `t2` [M, K] is the head of a buffer made by `_padded_empty` with total width `width`, return that buffer as
    [M, width]; else None."""
    b = t2._base
    if b is None or getattr(b, "_vgpa_pad", None) != (t2.shape[-1], width - t2.shape[-1]):
        return None
    if b.shape[-1] != width or not b.is_contiguous() or b.data_ptr() != t2.data_ptr() or b.numel() != t2.shape[0] * width:
        return None
    return b.view(-1, width)


class LoraExt:
    """Operands of one LoRA-carrying projection with the adapters riding the dense GEMM as extra K:

        forward :  y  = [x | T] [W | blockdiag(s_i B_i)]^T + b        T  = x A_cat^T            (lora_down)
        backward:  dx = [dy | dT] [W^T | A_cat^T]^T                    dT_i = dy_i (s_i B_i)     (lora_down)

    so the rank-r update costs (K + R) / K of one hipBLASLt GEMM instead of a read-modify-write pass over the [M, N] output
    (the former lora_up_add kernel: 437 MB per launch at 2.3 TB/s), and it is added in the fp32 accumulator instead of after
    a bf16 rounding of y.  The frozen-reference pass runs the SAME GEMM with a zero tail, so policy and reference share every
    base partial sum bit for bit (loss = ln 2 exactly at B = 0).  bf16 operand copies are cached here and refreshed once per
    optimizer step."""

    def __init__(self):
        self.fkey = self.akey = None

    def refresh(self, W, n_slices, loras):
        act = [i for i, l in enumerate(loras) if l is not None]
        r = loras[act[0]][0].shape[0]
        rp = _pad_rank(r)
        R = len(act) * rp
        N, K = W.shape
        Dn = N // n_slices
        dt, dev = W.dtype, W.device
        fkey = (W.data_ptr(), W._version, tuple(act), rp, N, K)
        if self.fkey != fkey:
            self.W_ext = torch.zeros(N, K + R, dtype=dt, device=dev)
            self.W_ext[:, :K] = W.detach()
            self.Wt_ext = torch.zeros(K, N + R, dtype=dt, device=dev)
            self.Wt_ext[:, :N] = W.detach().t()
            self.A_cat = torch.zeros(R, K, dtype=dt, device=dev)
            self.sBt = torch.zeros(len(act), rp, Dn, dtype=dt, device=dev)
            self.fkey, self.akey = fkey, None
            self.act, self.r, self.rp, self.R, self.N, self.K, self.Dn = act, r, rp, R, N, K, Dn
        akey = (ADAPTER_EPOCH,) + tuple((loras[i][0].data_ptr(), loras[i][0]._version, loras[i][1]._version, float(loras[i][2])) for i in act)
        if self.akey != akey:
            with torch.no_grad():
                for j, i in enumerate(act):
                    A, Bm, sc = loras[i]
                    if A.shape[0] != r:
                        raise RuntimeError("adapters on one projection must share a rank")
                    if dt == torch.bfloat16 and W.is_cuda:
                        # one launch per adapter (csrc/lora.hip lora_ext_refresh_kernel) with PEFT's roundings: a = bf16(A), sB = bf16(float(bf16(B)) * s)
                        # (the adapter is cast to the activation dtype first) -- the eight strided torch copies this replaces were 1300-1900 tiny kernels per step
                        _lib.call("vgpa_lora_ext_refresh", A.detach().float().contiguous(), Bm.detach().float().contiguous(), float(sc), r, K, Dn,
                                  self.A_cat[j * rp:], self.Wt_ext[:, N + j * rp:], N + R, self.W_ext[i * Dn:, K + j * rp:], K + R, self.sBt[j], _stream())
                        continue
                    self.A_cat[j * rp:j * rp + r] = A.to(dt)
                    sB = (Bm.to(dt).float() * sc).to(dt)                     # PEFT casts the adapter to the activation dtype first
                    self.W_ext[i * Dn:(i + 1) * Dn, K + j * rp:K + j * rp + r] = sB
                    self.sBt[j, :r] = sB.t()
                    self.Wt_ext[:, N + j * rp:N + j * rp + r] = self.A_cat[j * rp:j * rp + r].t()
            self.akey = akey
        return self


# ---- fp8 (OCP e4m3) form of a frozen projection: the "fp8 MFMA path" of BASELINE.json configs[4] (Wan2.2-TI2V-5B) ------------------
def quant_fp8_rows(x2):
    """bf16 [M, K] (row stride free) -> (e4m3 [M, K], fp32 scale [M, 1]): per-row dynamic scaling, csrc/fp8.hip"""
    M, K = x2.shape
    q = torch.empty(M, K, dtype=torch.float8_e4m3fn, device=x2.device)
    sc = torch.empty(M, 1, dtype=torch.float32, device=x2.device)
    _timed("quant_fp8_rows", 3.0 * M * K, lambda: _lib.call("vgpa_quant_fp8_rows", x2, x2.stride(0), q, sc, M, K, _stream()), "byte")
    return q, sc


def gelu_tanh_fwd_q8(u2):
    """bf16 [M, K] -> (e4m3(gelu_tanh(u)) [M, K], scale [M, 1]): the activation written as the fp8 GEMM operand by its producer"""
    M, K = u2.shape
    q = torch.empty(M, K, dtype=torch.float8_e4m3fn, device=u2.device)
    sc = torch.empty(M, 1, dtype=torch.float32, device=u2.device)
    _timed("gelu_tanh_fwd_q8", 3.0 * M * K, lambda: _lib.call("vgpa_gelu_tanh_fwd_q8", u2, M, K, q, sc, _stream()), "byte")
    return q, sc


def gelu_tanh_bwd_q8(u2, dy2):
    """(u, dy) bf16 [M, K] -> (e4m3(dy * gelu_tanh'(u)) [M, K], scale [M, 1])"""
    M, K = u2.shape
    q = torch.empty(M, K, dtype=torch.float8_e4m3fn, device=u2.device)
    sc = torch.empty(M, 1, dtype=torch.float32, device=u2.device)
    _timed("gelu_tanh_bwd_q8", 5.0 * M * K, lambda: _lib.call("vgpa_gelu_tanh_bwd_q8", u2, dy2, M, K, q, sc, _stream()), "byte")
    return q, sc


class Fp8Weight:
    """e4m3 copies of a frozen weight W [N, K], one scale per output row, for y = x W^T, and of W^T for dx = dy W; made once
    (the base weights never change in LoRA training) and kept with the weight tensor."""

    def __init__(self, W):
        self.version = W._version
        self.q, self.s = self._rows(W.detach())                 # [N, K], [1, N]
        self.qt, self.st = self._rows(W.detach().t().contiguous())   # [K, N], [1, K]

    @staticmethod
    def _rows(w):
        fmax = torch.finfo(torch.float8_e4m3fn).max
        amax = w.float().abs().amax(dim=1, keepdim=True)
        sc = torch.where(amax > 0, amax / fmax, torch.ones_like(amax))
        return (w.float() / sc).clamp(-fmax, fmax).to(torch.float8_e4m3fn), sc.t().contiguous()

    @staticmethod
    def of(W):
        c = getattr(W, "_vgpa_fp8", None)
        if c is None or c.version != W._version or c.q.device != W.device:
            c = Fp8Weight(W)
            W._vgpa_fp8 = c
        return c


def _fp8_gemm(xq, sx, wq, sw, bias=None):
    """bf16 [M, N] = (xq * sx) (wq * sw)^T through the vendor fp8 GEMM (hipBLASLt); xq [M, K], wq [N, K] e4m3, sx [M, 1], sw [1, N]"""
    M, N, K = xq.shape[0], wq.shape[0], xq.shape[1]
    out = []

    _timed("hipblaslt_gemm_fp8 (vendor)", 2.0 * M * N * K,
           lambda: out.append(torch._scaled_mm(xq, wq.t(), scale_a=sx, scale_b=sw, bias=bias, out_dtype=torch.bfloat16)))
    return out[0]


class _Fp8FrozenLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, bias):
        w8 = Fp8Weight.of(W)
        x2 = x.reshape(-1, x.shape[-1])
        if x2.stride(1) != 1:
            x2 = x2.contiguous()
        xq, sx = quant_fp8_rows(x2)
        ctx.w8 = w8
        return _fp8_gemm(xq, sx, w8.q, w8.s, bias).view(*x.shape[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, dy):
        w8 = ctx.w8
        dy2 = dy.reshape(-1, dy.shape[-1])
        if dy2.stride(1) != 1:
            dy2 = dy2.contiguous()
        dq, sd = quant_fp8_rows(dy2)
        return _fp8_gemm(dq, sd, w8.qt, w8.st).view(*dy.shape[:-1], w8.qt.shape[0]), None, None


def frozen_linear_fp8(x, W, bias):
    """frozen_linear with e4m3 operands (per-row dynamic activation scales, per-output-row weight scales), bf16 result"""
    if W.requires_grad or (bias is not None and bias.requires_grad):
        raise RuntimeError("videogpa_amd: the fp8 path is for frozen projections only")
    if x.dtype != torch.bfloat16:
        raise TypeError("frozen_linear_fp8: bf16 activations")
    return _Fp8FrozenLinearFn.apply(x, W, bias)


class _FfnTailFp8Fn(torch.autograd.Function):
    """The tail of a CogVideoX block with e4m3 operands in its frozen feed-forward, as ONE autograd node (autograd cannot carry an e4m3 tensor between nodes):
        x1 = x + gates1 * a ;  n2 = norm2(x1) modulated  -> e4m3 by the residual+LN kernel itself (vgpa_residual_ln_fwd_q8)
        f  = W2 gelu_tanh(W1 n2 + b1) + b2                  -> both products on the vendor fp8 GEMM, the GELU writes its own e4m3 operand (csrc/fp8.hip)
        x2 = x1 + gates2 * f ;  n_next = next norm of x2    -> the bf16 residual+LN pass as before: n_next feeds a LoRA-carrying projection (n_pad)
    Backward: vgpa_residual_ln_bwd_q8 (dx1 in bf16, gates2 * dx1 as e4m3) -> fp8 GEMM with W2^T -> GELU backward -> fp8 GEMM with W1^T -> the bf16
    residual+LN backward, which adds the residual path's gradient (dres) and writes the attention output's gradient with its LoRA tail (dy_pad).
    Every e4m3 operand is bit-identical to its bf16 producer followed by quant_fp8_rows, so the node equals residual_ln -> frozen_linear_fp8 ->
    gelu_tanh -> frozen_linear_fp8 -> residual_ln without the four bf16 round trips through HBM.  Saves what that chain saves."""

    @staticmethod
    def forward(ctx, x, a, gates1, ln_w, ln_b, mod2, W1, b1, W2, b2, gates2, nxt_w, nxt_b, nxt_mod, nxt_eps, text_len, eps, n_pad, dy_pad):
        _req(x, torch.bfloat16), _req(a, torch.bfloat16), _req(gates1, torch.float32), _req(gates2, torch.float32)
        _req(ln_w, torch.float32), _req(ln_b, torch.float32), _req(nxt_w, torch.float32), _req(nxt_b, torch.float32)
        B, S, D = x.shape
        rows, dev = B * S, x.device
        keep = any(ctx.needs_input_grad)          # forward-only (no_grad): no LN statistics, nothing saved
        w1, w2 = Fp8Weight.of(W1), Fp8Weight.of(W2)
        x1 = torch.empty_like(x)
        hq = torch.empty(rows, D, dtype=torch.float8_e4m3fn, device=dev)
        hs = torch.empty(rows, 1, dtype=torch.float32, device=dev)
        mean1 = torch.empty(B, S, dtype=torch.float32, device=dev) if keep else None
        rstd1 = torch.empty_like(mean1) if keep else None
        sv, s1v, st, s1t, mstride = _mod_ptrs(mod2)
        _timed("residual_ln_fwd_fp8", 7.0 * rows * D,
               lambda: _lib.call("vgpa_residual_ln_fwd_q8", x, a, gates1[:, 0], gates1[:, 1], gates1.stride(0), ln_w, ln_b, sv, s1v, st, s1t, mstride,
                                 B, S, D, text_len, float(eps), x1, hq, hs, mean1, rstd1, _stream()), "byte")
        u = _fp8_gemm(hq, hs, w1.q, w1.s, b1)
        del hq, hs
        gq, gs = gelu_tanh_fwd_q8(u)
        f = _fp8_gemm(gq, gs, w2.q, w2.s, b2)
        del gq, gs
        x2 = torch.empty_like(x)
        n = _padded_empty((B, S), D, n_pad, x.dtype, dev) if n_pad else _empty_rows(x.shape, x.dtype, dev)
        mean2 = torch.empty(B, S, dtype=torch.float32, device=dev) if keep else None
        rstd2 = torch.empty_like(mean2) if keep else None
        nv, n1v, nt, n1t, nstride = _mod_ptrs(nxt_mod)
        _timed("residual_ln_fwd", 8.0 * rows * D,
               lambda: _lib.call("vgpa_residual_ln_fwd", x1, f, gates2[:, 0], gates2[:, 1], gates2.stride(0), nxt_w, nxt_b, nv, n1v, nt, n1t, nstride,
                                 B, S, D, text_len, float(nxt_eps), x2, n, D + n_pad, mean2, rstd2, _stream()), "byte")
        if keep:
            ctx.save_for_backward(x1, mean1, rstd1, u, x2, mean2, rstd2, ln_w, mod2, gates1, nxt_w, nxt_mod, gates2)
            ctx.w, ctx.text_len, ctx.dy_pad = (w1, w2), text_len, dy_pad
        return x2, n

    @staticmethod
    def backward(ctx, dx2, dn):
        x1, mean1, rstd1, u, x2, mean2, rstd2, ln_w, mod2, gates1, nxt_w, nxt_mod, gates2 = ctx.saved_tensors
        w1, w2 = ctx.w
        B, S, D = x1.shape
        rows, dev = B * S, x1.device
        dn = torch.zeros_like(x2) if dn is None else dn.contiguous()
        dres = None if dx2 is None else dx2.contiguous()
        dx1 = torch.empty_like(x1)
        dfq = torch.empty(rows, D, dtype=torch.float8_e4m3fn, device=dev)
        dfs = torch.empty(rows, 1, dtype=torch.float32, device=dev)
        _, n1v, _, n1t, nstride = _mod_ptrs(nxt_mod)
        _timed("residual_ln_bwd_fp8", (7.0 + (2.0 if dres is not None else 0.0)) * rows * D,
               lambda: _lib.call("vgpa_residual_ln_bwd_q8", dn, x2, mean2, rstd2, nxt_w, n1v, n1t, nstride, gates2[:, 0], gates2[:, 1], gates2.stride(0),
                                 dres, B, S, D, ctx.text_len, dx1, dfq, dfs, _stream()), "byte")
        dg = _fp8_gemm(dfq, dfs, w2.qt, w2.st)
        del dfq, dfs
        duq, dus = gelu_tanh_bwd_q8(u, dg)
        del dg
        dh = _fp8_gemm(duq, dus, w1.qt, w1.st)
        del duq, dus
        dx = torch.empty_like(x1)
        dyp = ctx.dy_pad
        da = _padded_empty((B, S), D, dyp, x1.dtype, dev) if dyp else _empty_rows(x1.shape, x1.dtype, dev)
        _, s1v, _, s1t, mstride = _mod_ptrs(mod2)
        _timed("residual_ln_bwd", 10.0 * rows * D,
               lambda: _lib.call("vgpa_residual_ln_bwd", dh, x1, mean1, rstd1, ln_w, s1v, s1t, mstride, gates1[:, 0], gates1[:, 1], gates1.stride(0),
                                 dx1, B, S, D, ctx.text_len, dx, da, D + dyp, _stream()), "byte")
        return (dx, da) + (None,) * 17


def ffn_tail_fp8(x, a, gates1, ln_w, ln_b, mod2, W1, b1, W2, b2, gates2, nxt_w, nxt_b, nxt_mod=None, nxt_eps=1e-5, text_len=0, eps=1e-5, n_pad=0, dy_pad=0):
    """-> (x_out, n_next) of a CogVideoX block given its attention output `a`: gated residual + norm2, the frozen feed-forward on e4m3 operands written by
    their producers, gated residual + the next normalisation (see _FfnTailFp8Fn).  W1 [inner, D] / W2 [D, inner] and their biases are frozen."""
    if W1.requires_grad or W2.requires_grad or (b1 is not None and b1.requires_grad) or (b2 is not None and b2.requires_grad):
        raise RuntimeError("videogpa_amd: the fp8 path is for frozen projections only")
    if W1.shape[0] > 16384:
        raise RuntimeError(f"ffn_tail_fp8: the GELU -> e4m3 kernels hold one feed-forward row per workgroup, inner <= 16384; got {W1.shape[0]}")
    return _FfnTailFp8Fn.apply(x, a, gates1, ln_w, ln_b, mod2, W1, b1, W2, b2, gates2, nxt_w, nxt_b, nxt_mod, nxt_eps, int(text_len), eps, int(n_pad),
                               int(dy_pad))


class _LinearLoraExtFn(torch.autograd.Function):
    """y = x W^T + b (+ LoRA when `enabled`), W / b frozen; see LoraExt.  x / dy are used in place when they are the heads of
    padded buffers (produced by ops.residual_ln / qknorm_attention with n_pad / o_pad / grad pads), copied into one otherwise.
    x_recompute: (fn, tensors) with fn(*tensors) returning x [M, K] again (bit-identical) in the backward; the forward then keeps only the [M, R] LoRA
    down-projections instead of the whole [M, K + R] operand ("lean activations": x is a cheap function of a tensor that is saved anyway)."""

    @staticmethod
    def forward(ctx, x, bias, ext, enabled, scalings, x_recompute, *AB):
        K, R, N = ext.K, ext.R, ext.N
        x2 = x.reshape(-1, K)
        M = x2.shape[0]
        x_ext = _padded_base(x2, K + R)
        if x_ext is None:
            x_ext = torch.zeros(M, K + R, dtype=x.dtype, device=x.device) if not enabled else torch.empty(M, K + R, dtype=x.dtype, device=x.device)
            x_ext[:, :K].copy_(x2)
        xv, tv = x_ext[:, :K], x_ext[:, K:]
        if enabled:
            lora_down(xv, ext.A_cat, out=tv)       # raw kernel write into the tail (no autograd version bump on the producer's buffer)
        # disabled (reference pass): the tail of a `_padded_empty` buffer is zero since its allocation
        ctx.rows_per_call = current_gemm_rows()
        y = _gemm(x_ext, ext.W_ext, bias, ext=True, split=ctx.rows_per_call)
        if x_recompute is not None and enabled:
            fn, srcs = x_recompute
            ctx.save_for_backward(tv.contiguous(), *srcs)     # the recompute sources go through autograd's saved-tensor checks (in-place version, lifetime)
            ctx.x_fn = fn
        else:
            ctx.save_for_backward(x_ext)
            ctx.x_fn = None
        ctx.ext, ctx.enabled, ctx.xshape, ctx.scalings = ext, enabled, x.shape, scalings
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        ext, enabled = ctx.ext, ctx.enabled
        saved, *srcs = ctx.saved_tensors
        K, R, N, Dn, rp, r, act = ext.K, ext.R, ext.N, ext.Dn, ext.rp, ext.r, ext.act
        dy2 = dy.reshape(-1, N)
        M = dy2.shape[0]
        dy_ext = _padded_base(dy2, N + R) if dy2.stride(1) == 1 else None
        if dy_ext is None:
            dy_ext = torch.zeros(M, N + R, dtype=dy.dtype, device=dy.device) if not enabled else torch.empty(M, N + R, dtype=dy.dtype, device=dy.device)
            dy_ext[:, :N].copy_(dy2)
        if enabled:
            for j, i in enumerate(act):
                lora_down(dy_ext[:, i * Dn:(i + 1) * Dn], ext.sBt[j], out=dy_ext[:, N + j * rp:N + (j + 1) * rp])      # dT_i = dy_i (s B_i)
        dx = _gemm(dy_ext, ext.Wt_ext, ext=True, split=ctx.rows_per_call)                                                       # dy W + dT A
        out_grads = [None] * len(ctx.needs_input_grad[6:])
        if enabled:
            if ctx.x_fn is not None:
                t_all, xh = saved, ctx.x_fn(*srcs).reshape(M, K)     # [M, R] kept, x made again
            else:
                t_all, xh = saved[:, K:], saved[:, :K]
            for j, i in enumerate(act):
                # dB_i = s dy_i^T T_i (T_i = x A_i^T sits in the tail of x_ext); the scale is applied to the fp32 result
                out_grads[2 * i + 1] = lora_grad(dy_ext[:, i * Dn:(i + 1) * Dn], t_all[:, j * rp:(j + 1) * rp], ctx.scalings[j])[:, :r]
            dA = lora_grad(dy_ext[:, N:], xh)                                                                        # dT^T x, all adapters at once
            for j, i in enumerate(act):
                out_grads[2 * i] = dA[j * rp:j * rp + r]
        return (dx.view(ctx.xshape), None, None, None, None, None, *out_grads)


def linear_lora_ext(x, W, bias, ext, loras, enabled=True, x_recompute=None):
    """loras: list (one per equal output slice) of None or (A [r,in] fp32, B [out_i,r] fp32, scaling) -- the adapters that EXIST
    on this projection; `enabled` False = the reference pass (same GEMM, zero LoRA tail).  x_recompute: see _LinearLoraExtFn."""
    if W.requires_grad or (bias is not None and bias.requires_grad):
        raise RuntimeError("videogpa_amd: base weights are frozen on this path (LoRA-only training, as in the reference)")
    ext.refresh(W, len(loras), loras)
    flat = []
    for l in loras:
        flat += [None, None] if l is None else [l[0], l[1]]
    return _LinearLoraExtFn.apply(x, bias, ext, bool(enabled), tuple(float(loras[i][2]) for i in ext.act), x_recompute, *flat)


def linear_lora(x, W, bias, loras, ext=None):
    """loras: list (one per equal output slice) of None or (A [r,in] fp32, B [out_i,r] fp32, scaling)."""
    if all(l is None for l in loras):
        return frozen_linear(x, W, bias)
    if ext is None:
        ext = getattr(W, "_vgpa_lora_ext", None)
        if ext is None:
            ext = LoraExt()
            W._vgpa_lora_ext = ext          # lives with the frozen weight
    return linear_lora_ext(x, W, bias, ext, loras, True)


# --------------------------------------------------------------------------------------------- attention
def _bhs_strides(t):
    """element strides {batch, head, token} of a [B,H,S,64] view"""
    assert t.stride(3) == 1
    return _i64x3(t.stride(0), t.stride(1), t.stride(2))


LOG2E = 1.4426950408889634
# The attention kernels are the "w1" family (csrc/attention_w1.hip: one wave per SIMD, LDS-DMA rings, generated hand-scheduled main loops); the
# backward is a deterministic dK/dV kernel + a dQ kernel (7 matrix products per score block).  A one-kernel backward with dQ by fp32 atomics
# (5 products) measured SLOWER on MI355X at the headline shape (46.6 ms vs 26.5 ms per layer: its 60 GB of dQ atomics per launch run at
# ~2.6 TB/s, 23.9 ms without them) and is gone.
# tail-round treatment of the attention launches (split_mode of vgpa_attn_fwd_w1_res / vgpa_attn_bwd_*_w1): -1 automatic (default), 0 off
ATTN_SPLIT_MODE = -1
# "Precise delta": the attention forward also stores what the bf16 rounding of its output dropped, and the backward forms delta = rowsum(dO o O) from the
# completed output.  delta stands for rowsum(P o dP); formed from the bf16 O alone (what every flash-attention backward, torch's included, does) each row's dS
# stops summing to zero and dQ picks up a coherent error -d(delta_i) sum_j P_ij K_j that swamps q / k gradients which are small by cancellation (37-87 % of
# the last block's to_q / to_k adapter gradients at BASELINE configs[0] width: profiles/r04_cfg1_round_diag_*.json).  Two forms of the residual tensor:
#   "int8" (default): one byte per output element = eight further mantissa bits (csrc/common.h res8) -- O to 2^-17; every attention path has it (head_dim 64
#                     and 128, e4m3 forward, short-key kernel, lean activations);
#   "bf16"          : bf16(O_fp32 - bf16(O)), twice the bytes, O to 2^-18 (the round-4 form; head_dim 64 only);
#   None / "off"    : the textbook backward.
# It is NOT process state: models carry `precise_delta` (constructor default = precise_delta_default(), i.e. VGPA_PRECISE_DELTA in the environment: 0 | off |
# bf16 | int8) and hand it to qknorm_attention / attention128 per call; the autograd node keeps what its forward used.
def precise_delta_default():
    v = _os.environ.get("VGPA_PRECISE_DELTA", "int8").lower()
    if v in ("0", "off", "none", "false"):
        return None
    if v in ("1", "int8", "res8", "true"):
        return "int8"
    if v == "bf16":
        return "bf16"
    raise ValueError(f"VGPA_PRECISE_DELTA={v!r}: expected 0 | off | int8 | bf16")


def _res_kind(o_res):
    if o_res is None:
        return 0
    if o_res.dtype == torch.bfloat16:
        return 1
    if o_res.dtype == torch.uint8:
        return 2
    raise TypeError(f"o_res: bf16 (rounding residual) or uint8 (eight further mantissa bits), got {o_res.dtype}")


def res8_decode(o, o_res8):
    """fp32 value of a bf16 tensor `o` completed by its res8 bytes (csrc/common.h): o + (byte - 128) * 2^(E - 142), E = biased exponent of o (tests)"""
    E = (o.contiguous().view(torch.int16).to(torch.int32) >> 7) & 0xFF
    sc = torch.where(E > 15, torch.ldexp(torch.ones((), device=o.device), E - 142), torch.zeros((), device=o.device))
    return o.float() + (o_res8.float() - 128.0) * sc


def prescale_q(q, scale=None):
    """The attention kernels take q * scale * log2(e) (one bf16 rounding).  The fused path gets it from the QK-norm
    kernel; this helper is for callers holding a plain q."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    return (q.float() * (scale * LOG2E)).to(q.dtype)


class AttnFwdPolicy:
    """Which forward one attention layer runs, decided from what the kernel itself reports.  "bound": the w1 kernel (softmax shifted per row by
    min(Cauchy-Schwarz bound, sampled row maximum + 64) instead of a running maximum; strips with a row it cannot represent -- the true maximum more than ~176 log2
    units above the maximum over 64 sampled keys -- are flagged and redone inside the same call by the online-softmax kernel: results never depend on it, time does).
    "online": every strip on the online-softmax kernel (vgpa_attn_fwd_online_res).  On the data that gets strips flagged (near one-hot rows with a huge score range)
    the online kernel itself runs 2.3-2.5 x its usual time (its running maximum keeps moving: measured 17.5 ms against 7.2, profiles/r06b_attn_trained_like.txt), so
    the switch only pays once MORE THAN HALF the strips would be swept twice: SWITCH = 0.5.  The flags of a layer's first CHECKS calls (and of every RECHECK-th call
    after) are read back -- one host sync each -- and the layer switches for good above SWITCH.  `fixed` pins the mode (tools, tests)."""
    SWITCH, CHECKS, RECHECK = 0.5, 2, 1024

    def __init__(self, mode="bound", fixed=False):
        self.mode, self.fixed = mode, fixed
        self.calls = 0
        self.redo_fraction = None          # of the most recent observed call
        self.switched_at = None

    def wants_flags(self):
        return self.mode == "bound" and not self.fixed and (self.calls < self.CHECKS or self.calls % self.RECHECK == 0)

    def observe(self, fraction):
        self.redo_fraction = fraction
        if not self.fixed and fraction > self.SWITCH:
            self.mode, self.switched_at = "online", self.calls


def _strip_flags(ws, head_words, B, H, Sq):
    """the int32 redo flags [B, H, strips of 256 rows] a forward left in its workspace `ws` (uint8), behind `head_words` 32-bit words of other use:
    B*H (max |k|^2 per head) for vgpa_attn_fwd_w1_res / vgpa_attn_fwd_online_res, 5*B*H (amax statistics + max |k|^2) for vgpa_attn128_fwd_f8"""
    strips = (Sq + 255) // 256
    return ws[:4 * (head_words + B * H * strips)].view(torch.int32)[head_words:].view(B, H, strips)


def attention_redo_fraction(ws, B, H, S):
    """fraction of the (batch, head, 256-row strip) tasks the last vgpa_attn_fwd_w1_res call on workspace `ws` flagged and redid (synchronises)"""
    return float((_strip_flags(ws, B * H, B, H, S) != 0).float().mean())


def attention_fwd_raw(q, k, v, scale=None, q_prescaled=False, split_mode=None, o_pad=0, o_res=None, policy=None):
    """q,k,v: bf16 [B,H,S,64] views (any batch/head/token strides).  -> o [B,S,H*64] bf16, lse2 [B,H,S] fp32.
    o_res: optional [B,S,H*64] buffer, bf16 or uint8, that receives what the output's bf16 rounding dropped (see "Precise delta").
    split_mode: -1 lets the launcher cut the tasks of a mostly empty last scheduling round into key-range chunks,
    0 forbids it, k >= 2 forces k chunks for every task (tests).  o_pad: o is the head of a [B,S,H*64+o_pad] buffer (the
    output projection's LoRA tail, see LoraExt)."""
    B, H, S, Dh = q.shape
    scale = Dh ** -0.5 if scale is None else scale
    if not q_prescaled:
        q = prescale_q(q, scale)
    o = _padded_empty((B, S), H * Dh, o_pad, torch.bfloat16, q.device) if o_pad else torch.empty(B, S, H * Dh, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B, H, S, dtype=torch.float32, device=q.device)
    ov = o.unflatten(-1, (H, Dh)).permute(0, 2, 1, 3)
    split_mode = ATTN_SPLIT_MODE if split_mode is None else split_mode
    ws_bytes = _lib.query("vgpa_attn_fwd_w1_workspace_bytes", B, H, S)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
    rv = None if o_res is None else o_res.unflatten(-1, (H, Dh)).permute(0, 2, 1, 3)
    entry = "vgpa_attn_fwd_online_res" if (policy is not None and policy.mode == "online") else "vgpa_attn_fwd_w1_res"
    _timed("attn_fwd_kernel", 4.0 * S * S * Dh * B * H, lambda: _lib.call(
        entry, q, k, v, o, o_res, _res_kind(o_res), lse, _bhs_strides(q), _bhs_strides(k), _bhs_strides(v), _bhs_strides(ov), None if rv is None else _bhs_strides(rv),
        B, H, S, Dh, float(scale), int(split_mode), ws, ws_bytes, _stream()))
    if policy is not None:
        if policy.wants_flags() and not torch.cuda.is_current_stream_capturing():
            policy.observe(attention_redo_fraction(ws, B, H, S))
        policy.calls += 1
    return o, lse


def attention_bwd_raw(q, k, v, o, do, lse, dq, dk, dv, scale=None, q_prescaled=False, split_mode=None, o_res=None):
    """All [B,H,S,64] bf16 views; writes dq, dk, dv in place.  Three launches: delta, dK/dV, dQ.  o_res ([B,H,S,64] view, bf16 or uint8): what the forward
    kept of the output beyond its bf16 rounding; delta is then formed from the completed output ("Precise delta").
    Algorithmic FLOPs (backward = 2 x forward): dK/dV kernel carries dV, dP, dK = 6 S^2 d; dQ kernel 2 S^2 d
    (the S = QK^T recomputes in both kernels and the second dP are overhead, not counted)."""
    B, H, S, Dh = q.shape
    scale = Dh ** -0.5 if scale is None else scale
    if not q_prescaled:
        q = prescale_q(q, scale)
    delta = torch.empty(B, H, S, dtype=torch.float32, device=q.device)
    st = _stream()
    stats = torch.empty(B, H, 2, S, dtype=torch.float32, device=q.device)     # the {-lse2, -delta} planes the dK/dV kernel streams
    _timed("attn_delta_kernel", (4.0 + (0 if o_res is None else o_res.element_size())) * B * H * S * Dh, lambda: _lib.call(
        "vgpa_attn_bwd_prep_w1_res", o, o_res, _res_kind(o_res), do, lse, _bhs_strides(o), None if o_res is None else _bhs_strides(o_res), _bhs_strides(do),
        delta, stats, B, H, S, Dh, st), "byte")
    split_mode = ATTN_SPLIT_MODE if split_mode is None else split_mode
    ws_bytes = _lib.query("vgpa_attn_bwd_split_workspace_bytes", B, H, S) if split_mode != 0 else 0
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=q.device)
    wsp = ws if ws_bytes else None
    _timed("attn_bwd_dkv_kernel", 6.0 * S * S * Dh * B * H, lambda: _lib.call(
        "vgpa_attn_bwd_dkv_w1", q, k, v, do, stats, dk, dv, _bhs_strides(q), _bhs_strides(k), _bhs_strides(v), _bhs_strides(do),
        _bhs_strides(dk), _bhs_strides(dv), B, H, S, Dh, float(scale), int(split_mode), wsp, ws_bytes, st))
    _timed("attn_bwd_dq_kernel", 2.0 * S * S * Dh * B * H, lambda: _lib.call(
        "vgpa_attn_bwd_dq_w1", q, k, v, do, lse, delta, dq, _bhs_strides(q), _bhs_strides(k), _bhs_strides(v), _bhs_strides(do),
        _bhs_strides(dq), B, H, S, Dh, float(scale), int(split_mode), wsp, ws_bytes, st))


ATTN128_W1 = True    # False: the compiler-scheduled hd128 forward everywhere (tools)


ATTN128_F8_MIN_KEYS = 1024      # below this the e4m3 forward's prep passes and pipeline fill do not pay (cross-attention over 512 text tokens stays bf16)


def attention128_uses_f8(f8, Skv):
    """does attention128_fwd_raw(f8=f8) run the e4m3 kernel for a sweep of Skv keys?"""
    return bool(f8) and Skv >= ATTN128_F8_MIN_KEYS


class F8AttnPolicy:
    """Whether one head_dim-128 self-attention layer runs its forward on e4m3 operands (vgpa_attn128_fwd_f8) or in bf16, decided ONCE from the data of its first call.
    The e4m3 forward's time no longer depends on the data (sampled shift), its ACCURACY does: q and k each carry a 2^-4 relative rounding per element, so a score
    q.k (log2 units) is off by ~ ERR_PER_BOUND x |q| |k| scale log2(e) rms -- measured 0.08 log2 units at a row bound of 29 (unit QK-norm gains: the ~5 % per weight of
    the kernel's tests) and 0.73 at a bound of 180 (gains of 2.5: every weight off by a factor 1.7 rms; tools/f8_sharp_diag.py).  `threshold` (log2 units of rms score
    error, default 0.5) is where the layer goes to the bf16 forward for good (6.3 ms per launch at the cfg5 shape against 4.1).  fixed=True pins the mode
    (WanModel.enable_fp8(attention=True): the e4m3 kernel whatever the data).  The decision is taken at the layer's FIRST call only -- the frozen-reference pass of a
    DPO step -- so that reference and policy pass always run the same forward (loss = ln 2 exactly at B = 0); reset() re-arms it."""
    ERR_PER_BOUND = 0.004

    def __init__(self, mode="f8", fixed=False, threshold=0.5):
        self.mode, self.fixed, self.threshold = mode, fixed, float(threshold)
        self.decided = False
        self.estimated_score_error = None

    def reset(self):
        self.decided = False

    @staticmethod
    def score_error_estimate(q, k, H, scale):
        """q [B, Lq, H*d], k [B, Lk, H*d] (token-major, as the model holds them) -> estimated rms error of an e4m3 score in log2 units, worst (batch, head)"""
        B, Lq, D = q.shape
        d = D // H
        qn = q.view(B, Lq, H, d).float().pow(2).sum(-1).amax(dim=1).sqrt()          # [B, H]: the longest query row per head
        kn = k.view(B, k.shape[1], H, d).float().pow(2).sum(-1).amax(dim=1).sqrt()
        return float((qn * kn).amax()) * float(scale) * LOG2E * F8AttnPolicy.ERR_PER_BOUND

    def use_f8(self, q, k, H, scale):
        if not self.fixed and not self.decided and self.mode == "f8":
            self.estimated_score_error = self.score_error_estimate(q, k, H, scale)      # one host sync, once per layer
            if self.estimated_score_error > self.threshold:
                self.mode = "bf16"
        self.decided = True
        return self.mode == "f8"


def attention128_f8_redo_fraction(ws, B, H, Sq):
    """fraction of the (batch, head, 256-row strip) tasks the last vgpa_attn128_fwd_f8 call on workspace `ws` flagged and redid in bf16 (synchronises)"""
    return float((_strip_flags(ws, 5 * B * H, B, H, Sq) != 0).float().mean())


def attention128_fwd_raw(q, k, v, scale, o_pad=0, f8=False, o_res8=None, deq=None, report=None):
    """q [B,H,Sq,128], k / v [B,H,Skv,128] bf16 views (any batch / head / token strides, last dim contiguous) -> (o, lse2 [B,H,Sq] fp32).
    f8: the e4m3 forward (csrc/attention_hd128.hip, vgpa_attn128_fwd_f8) for sweeps of at least ATTN128_F8_MIN_KEYS keys.
    deq (e4m3 forward only): three bf16 buffers [B, Sq, H*128], [B, Skv, H*128], [B, Skv, H*128] that receive the operands the e4m3 products really ran
    on, dequantised EXACTLY (q: times scale * log2 e) -- what the backward of THIS forward runs on (attention128_bwd_raw(..., q_prescaled=True) on them recomputes
    the forward's own scores bit for bit).
    o_res8: optional uint8 [B, Sq, H*128] buffer that receives eight further mantissa bits of every output value ("Precise delta").
    report: optional dict; the e4m3 forward stores "redo_fraction" (strips it flagged and redid in bf16) and "strip_flags" (bool [B, H, strips of 256 rows])
    there -- one host sync.
    o is a [B,H,Sq,128] view of token-major storage [B, Sq, H*128 (+ o_pad)]: the caller's flatten to [B*Sq, H*128] is free, and with
    o_pad it is the head of a `_padded_empty` buffer (the output projection's LoRA tail, see LoraExt)."""
    B, H, Sq, D = q.shape
    Skv = k.shape[2]
    assert D == 128 and k.shape == (B, H, Skv, 128) and v.shape == k.shape and q.dtype == k.dtype == v.dtype == torch.bfloat16
    o2 = _padded_empty((B, Sq), H * D, o_pad, torch.bfloat16, q.device) if o_pad else torch.empty(B, Sq, H * D, dtype=torch.bfloat16, device=q.device)
    o = o2.unflatten(-1, (H, D)).permute(0, 2, 1, 3)
    lse = torch.empty(B, H, Sq, dtype=torch.float32, device=q.device)
    rv = rs = None
    if o_res8 is not None:
        if o_res8.dtype != torch.uint8 or o_res8.shape != (B, Sq, H * D) or not o_res8.is_contiguous():
            raise TypeError("attention128_fwd_raw: o_res8 is a contiguous uint8 [B, Sq, H*128] buffer")
        rv = o_res8.unflatten(-1, (H, D)).permute(0, 2, 1, 3)
        rs = _bhs_strides(rv)
    if attention128_uses_f8(f8, Skv):
        ws_bytes = _lib.query("vgpa_attn128_fwd_f8_workspace_bytes", B, H, Sq, Skv)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
        dv_ = [None] * 3
        if deq is not None:
            for t, S_ in zip(deq, (Sq, Skv, Skv)):
                if t.dtype != torch.bfloat16 or t.shape != (B, S_, H * D) or not t.is_contiguous():
                    raise TypeError("attention128_fwd_raw: deq = three contiguous bf16 [B, S, H*128] buffers (q, k, v)")
            dv_ = [t.unflatten(-1, (H, D)).permute(0, 2, 1, 3) for t in deq]
        ds_ = [None if t is None else _bhs_strides(t) for t in dv_]
        _timed("attn128_fwd_f8", 4.0 * B * H * Sq * Skv * D, lambda: _lib.call(
            "vgpa_attn128_fwd_f8", q, k, v, o, lse, _bhs_strides(q), _bhs_strides(k), _bhs_strides(v), _bhs_strides(o), rv, rs, dv_[0], dv_[1], dv_[2],
            ds_[0], ds_[1], ds_[2], B, H, Sq, Skv, float(scale), ws, ws_bytes, _stream()))
        if report is not None:          # tools / tests: what fraction of the strips the e4m3 kernel handed to the bf16 redo pass
            report["redo_fraction"] = attention128_f8_redo_fraction(ws, B, H, Sq)
            report["strip_flags"] = _strip_flags(ws, 5 * B * H, B, H, Sq) != 0
        return o, lse
    if deq is not None:
        raise ValueError("attention128_fwd_raw: deq buffers are written by the e4m3 forward only (f8=True and at least ATTN128_F8_MIN_KEYS keys)")
    ws_bytes = _lib.query("vgpa_attn128_fwd_workspace_bytes", B, H, Sq) if ATTN128_W1 else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device) if ws_bytes else None
    _timed("attn128_fwd" if Skv >= 1024 else "attn128_fwd (short keys)", 4.0 * B * H * Sq * Skv * D, lambda: _lib.call(
        "vgpa_attn128_fwd", q, k, v, o, lse, _bhs_strides(q), _bhs_strides(k), _bhs_strides(v), _bhs_strides(o), rv, rs, B, H, Sq, Skv, float(scale),
        ws, ws_bytes, _stream()))
    return o, lse


def attention128_bwd_raw(q, k, v, o, do, lse, dq, dk, dv, scale, o_res8=None, q_prescaled=False):
    """all [B,H,S,128] bf16 views; writes dq, dk, dv in place (they may be strided slices of a fused gradient buffer).  o_res8 (uint8 [B, Sq, H*128], as the
    forward wrote it): delta = rowsum(dO o O) is formed from the output completed by those eight further mantissa bits ("Precise delta").
    q_prescaled: q is the e4m3 forward's q_deq (the query times scale * log2 e, exact): vgpa_attn128_bwd_prescaled -- scores bit for bit the forward's, dq still
    the gradient w.r.t. the unscaled query."""
    B, H, Sq, D = q.shape
    Skv = k.shape[2]
    rv = None if o_res8 is None else o_res8.unflatten(-1, (H, D)).permute(0, 2, 1, 3)
    ws_bytes = _lib.query("vgpa_attn128_bwd_workspace_bytes", B, H, Sq)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
    # algorithmic work as SURVEY 8d counts it: backward = 2 x forward (dV, dP, dK, dQ); the S = QK^T recomputes of the split kernels are overhead
    _timed("attn128_bwd" if Skv >= 1024 else "attn128_bwd (short keys)", 8.0 * B * H * Sq * Skv * D, lambda: _lib.call(
        "vgpa_attn128_bwd_prescaled" if q_prescaled else "vgpa_attn128_bwd", q, k, v, o, do, lse, dq, dk, dv, _bhs_strides(q), _bhs_strides(k), _bhs_strides(v), _bhs_strides(o), _bhs_strides(do),
        _bhs_strides(dq), _bhs_strides(dk), _bhs_strides(dv), rv, None if rv is None else _bhs_strides(rv), B, H, Sq, Skv, float(scale),
        -1 if ATTN128_W1 else 0, ws, ws_bytes, _stream()))


class _Attention128Fn(torch.autograd.Function):
    """softmax(scale q k^T) v for head_dim 128, query and key lengths free (csrc/attention_hd128.hip): Wan2.2's self- and cross-attention"""

    @staticmethod
    def forward(ctx, q, k, v, scale, o_pad, precise_delta):
        q, k, v = (t if t.stride(3) == 1 else t.contiguous() for t in (q, k, v))
        o_res8 = None
        if precise_delta and any(ctx.needs_input_grad[:3]):
            o_res8 = torch.empty(q.shape[0], q.shape[2], q.shape[1] * q.shape[3], dtype=torch.uint8, device=q.device)
        o, lse = attention128_fwd_raw(q, k, v, scale, o_pad, o_res8=o_res8)
        ctx.save_for_backward(q, k, v, o, lse, o_res8)
        ctx.scale = float(scale)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, o_res8 = ctx.saved_tensors
        B, H, Sq, D = q.shape
        Skv = k.shape[2]
        do = do if do.stride(3) == 1 else do.contiguous()
        dq = torch.empty(B, Sq, H, D, dtype=torch.bfloat16, device=q.device).permute(0, 2, 1, 3)      # token-major, like the projections' outputs
        dk = torch.empty(B, Skv, H, D, dtype=torch.bfloat16, device=q.device).permute(0, 2, 1, 3)
        dv = torch.empty(B, Skv, H, D, dtype=torch.bfloat16, device=q.device).permute(0, 2, 1, 3)
        attention128_bwd_raw(q, k, v, o, do, lse, dq, dk, dv, ctx.scale, o_res8=o_res8)
        return dq, dk, dv, None, None, None


def attention128(q, k, v, scale=None, o_pad=0, precise_delta="int8"):
    """q [B, H, Sq, 128], k / v [B, H, Skv, 128] (bf16, last dim contiguous) -> [B, H, Sq, 128].  precise_delta: "int8" (default) / None -- see "Precise delta" above"""
    if precise_delta not in (None, "int8"):
        raise ValueError('attention128: precise_delta is "int8" or None (the bf16 residual form exists at head_dim 64 only)')
    return _Attention128Fn.apply(q, k, v, q.shape[-1] ** -0.5 if scale is None else scale, int(o_pad), precise_delta)


class _QKNormAttentionFn(torch.autograd.Function):
    """qkv [B,S,3*H*64] (fused QKV GEMM output) -> attention output [B,S,H*64].
    QK-norm (+ optional 3D RoPE on tokens >= text_len) -> flash attention; backward returns dqkv in the same layout."""

    @staticmethod
    def forward(ctx, qkv, wq, bq, wk, bk, rope_cos, rope_sin, text_len, H, eps, o_pad, grad_pad, rope_mode=0, recompute_qk=False, precise_delta=None, fwd_policy=None):
        """o_pad / grad_pad: the attention output / the gradient of qkv are returned as heads of buffers that much wider (the
        LoRA tails of the projections on either side, see LoraExt).  recompute_qk: the normalised q / k are not kept for the backward
        but made again from qkv (one more pass of the QK-norm kernel, bit-identical) -- a third of this node's saved bytes."""
        _req(qkv, torch.bfloat16)
        B, S, W = qkv.shape
        Dh = W // (3 * H)
        qkv5 = qkv.view(B, S, 3, H, Dh)
        q_in, k_in, v = (qkv5[:, :, i].permute(0, 2, 1, 3) for i in range(3))  # [B,H,S,Dh] views
        qn = torch.empty(B, H, S, Dh, dtype=torch.bfloat16, device=qkv.device)
        kn = torch.empty_like(qn)
        _timed("qknorm_rope_fwd", 8.0 * B * H * S * Dh, lambda: _lib.call(
            "vgpa_qknorm_rope_fwd", q_in, k_in, qn, kn, _bhs_strides(q_in), _bhs_strides(k_in), _bhs_strides(qn), _bhs_strides(kn),
            wq, bq, wk, bk, rope_cos, rope_sin, text_len, B, H, S, Dh, float(eps), float(Dh ** -0.5 * LOG2E), int(rope_mode), _stream()), "byte")
        # what the output's bf16 rounding drops, for the backward's delta -- only where a backward will run and on the w1 forward; lean activations keep it too
        # (1 byte per output element next to the 6 that recompute_qk gives back)
        o_res = None
        if precise_delta and ctx.needs_input_grad[0]:
            o_res = torch.empty(B, S, H * Dh, dtype=torch.uint8 if precise_delta == "int8" else torch.bfloat16, device=qkv.device)
        o, lse = attention_fwd_raw(qn, kn, v, q_prescaled=True, o_pad=o_pad, o_res=o_res, policy=fwd_policy)
        if recompute_qk:
            ctx.save_for_backward(qkv, o, lse, wq, wk, rope_cos, rope_sin, bq, bk, o_res)
        else:
            ctx.save_for_backward(qkv, qn, kn, o, lse, wq, wk, rope_cos, rope_sin, o_res)
        ctx.meta = (text_len, H, eps, grad_pad, int(rope_mode), bool(recompute_qk))
        return o

    @staticmethod
    def backward(ctx, do):
        text_len, H, eps, grad_pad, rope_mode, recompute_qk = ctx.meta
        if recompute_qk:
            qkv, o, lse, wq, wk, rope_cos, rope_sin, bq, bk, o_res = ctx.saved_tensors
        else:
            qkv, qn, kn, o, lse, wq, wk, rope_cos, rope_sin, o_res = ctx.saved_tensors
        B, S, W = qkv.shape
        Dh = W // (3 * H)
        do = do.contiguous()
        qkv5 = qkv.view(B, S, 3, H, Dh)
        q_in, k_in, v = (qkv5[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        if recompute_qk:
            qn = torch.empty(B, H, S, Dh, dtype=torch.bfloat16, device=qkv.device)
            kn = torch.empty_like(qn)
            _timed("qknorm_rope_fwd", 8.0 * B * H * S * Dh, lambda: _lib.call(
                "vgpa_qknorm_rope_fwd", q_in, k_in, qn, kn, _bhs_strides(q_in), _bhs_strides(k_in), _bhs_strides(qn), _bhs_strides(kn),
                wq, bq, wk, bk, rope_cos, rope_sin, text_len, B, H, S, Dh, float(eps), float(Dh ** -0.5 * LOG2E), int(rope_mode), _stream()), "byte")
        dqkv = _padded_empty((B, S), W, grad_pad, qkv.dtype, qkv.device) if grad_pad else torch.empty_like(qkv)
        d5 = dqkv.unflatten(-1, (3, H, Dh))
        dq_in, dk_in, dv = (d5[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        dqn = torch.empty_like(qn)
        dkn = torch.empty_like(kn)
        ov = o.unflatten(-1, (H, Dh)).permute(0, 2, 1, 3)
        dov = do.view(B, S, H, Dh).permute(0, 2, 1, 3)
        attention_bwd_raw(qn, kn, v, ov, dov, lse, dqn, dkn, dv, q_prescaled=True,
                          o_res=None if o_res is None else o_res.unflatten(-1, (H, Dh)).permute(0, 2, 1, 3))
        _timed("qknorm_rope_bwd", 12.0 * B * H * S * Dh, lambda: _lib.call(
            "vgpa_qknorm_rope_bwd", dqn, dkn, q_in, k_in, dq_in, dk_in, _bhs_strides(dqn), _bhs_strides(dkn), _bhs_strides(q_in),
            _bhs_strides(k_in), _bhs_strides(dq_in), _bhs_strides(dk_in), wq, wk, rope_cos, rope_sin, text_len, B, H, S, Dh,
            float(eps), rope_mode, _stream()), "byte")
        return dqkv, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None


def qknorm_attention(qkv, wq, bq, wk, bk, H, text_len=0, rope=None, eps=1e-6, o_pad=0, grad_pad=0, rope_mode=0, recompute_qk=False, precise_delta="int8", fwd_policy=None):
    """rope = (cos, sin) fp32 [S - text_len, 64]; rope_mode 0: interleaved pairs (diffusers' CogVideoX), 1: half-split pairs inside each
    32-feature half (VGGT's RotaryPositionEmbedding2D, tables from `rope2d_tables`).  precise_delta: "int8" | "bf16" | None, see "Precise delta"."""
    cos, sin = (None, None) if rope is None else rope
    if precise_delta not in (None, "int8", "bf16"):
        raise ValueError(f'precise_delta: "int8", "bf16" or None, got {precise_delta!r}')
    return _QKNormAttentionFn.apply(qkv, wq, bq, wk, bk, cos, sin, text_len, H, eps, o_pad, grad_pad, rope_mode, bool(recompute_qk), precise_delta, fwd_policy)


def rope2d_tables(pos, head_dim=64, frequency=100.0):
    """cos / sin rows [N, head_dim] fp32 of vggt/layers/rope.py:103-112,154-188 for integer positions pos [N, 2] = (y, x): features
    [0, d/2) rotate with y, [d/2, d) with x; inside a half, feature i and i + d/4 share the angle pos * frequency^(-2i / (d/2))."""
    half = head_dim // 2
    inv = 1.0 / (frequency ** (torch.arange(0, half, 2, device=pos.device).float() / half))
    ang = pos.float()[:, :, None] * inv[None, None, :]                 # [N, 2, half/2]
    ang = torch.cat([ang, ang], dim=-1).reshape(pos.shape[0], head_dim)  # [y-angles x2 | x-angles x2]
    return ang.cos().contiguous(), ang.sin().contiguous()


# ---- prediction heads of VGGT and Depth Anything 3 (csrc/vggt_heads.hip, csrc/dualdpt.hip): fp32, channels-last, forward only ----------------
def _heads_in(*ts):
    for t in ts:
        if t is None:
            continue
        _req(t, torch.float32)
        if torch.is_grad_enabled() and t.requires_grad:
            raise RuntimeError("the fp32 head kernels are forward only: call them under torch.no_grad()")


def pack_conv_weight(w):
    """Conv2d weight [Cout, Cin, kh, kw] -> [kh][kw][Cin][Cout] fp32 contiguous, the layout the convolution kernels read"""
    return w.detach().float().permute(2, 3, 1, 0).contiguous()


def _conv_out(name, x, w_packed, taps, out_shape, *res, refuse=None):
    """what the convolution wrappers share: w_packed must be [*taps, Cin, Cout] for x's Cin channels, both widths multiples of 16; returns the empty fp32
    output [*out_shape, Cout], whose shape every residual that is given must have.  `refuse` is the wrapper's own complaint about the call's geometry,
    raised behind the weight check (out_shape is not looked at then)"""
    Cin, Cout = x.shape[-1], w_packed.shape[-1]
    if tuple(w_packed.shape) != (*taps, Cin, Cout) or Cin % 16 or Cout % 16:
        raise RuntimeError(f"{name}: weight {tuple(w_packed.shape)} does not fit input channels {Cin} (multiples of 16)")
    if refuse:
        raise RuntimeError(f"{name}: {refuse}")
    out = torch.empty(*out_shape, Cout, device=x.device, dtype=torch.float32)
    if any(r is not None and r.shape != out.shape for r in res):
        raise RuntimeError(f"{name}: residual shape differs from the output's")
    return out


def conv3x3_f32(x, w_packed, bias=None, res=None, res2=None, relu_in=False, relu_res=False, stride=1):
    """x [N,H,W,Cin] -> conv3x3(relu?(x), pad 1, stride) + bias? + relu?(res)? + res2? as [N,Ho,Wo,Cout]; w_packed [3,3,Cin,Cout]"""
    _heads_in(x, w_packed, bias, res, res2)
    N, H, W, Cin = x.shape
    out = _conv_out("conv3x3_f32", x, w_packed, (3, 3), (N, (H - 1) // stride + 1, (W - 1) // stride + 1), res, res2)
    _timed("conv3x3_f32", 2.0 * out.numel() * 9 * Cin,
           lambda: _lib.call("vgpa_conv3x3_f32", x, w_packed, bias, res, res2, out, N, H, W, Cin, out.shape[-1], stride,
                             (1 if relu_in else 0) | (2 if relu_res else 0), _stream()))
    return out


def conv1x1_f32(x, w_packed, bias=None):
    """x [..., Cin] -> x . w_packed [Cin, Cout] + bias? as [..., Cout]"""
    _heads_in(x, w_packed, bias)
    Cin, Cout = w_packed.shape
    if x.shape[-1] != Cin or Cin % 16 or Cout % 16:
        raise RuntimeError(f"conv1x1_f32: weight {tuple(w_packed.shape)} does not fit input {tuple(x.shape)} (channels in multiples of 16)")
    out = torch.empty(*x.shape[:-1], Cout, device=x.device, dtype=torch.float32)
    M = out.numel() // Cout
    _timed("conv1x1_f32", 2.0 * M * Cin * Cout, lambda: _lib.call("vgpa_conv1x1_f32", x, w_packed, bias, out, M, Cin, Cout, _stream()))
    return out


def uv_embed_tables(width, height, channels, aspect_ratio, device, ratio=0.1, f32_angles=False):
    """The two halves of `position_grid_to_embed(create_uv_grid(width, height, aspect_ratio), channels) * ratio` (vggt/heads/utils.py:11-109,
    dpt_head.py:249-259): the embedding concatenates an x half and a y half, so it is two tables, xtab [width, channels/2] and
    ytab [height, channels/2] (fp32: sin | cos of coordinate * 100^(-i / (channels/4)), angles in float64 as upstream).  f32_angles: Depth
    Anything 3's recipe (model/utils/head_utils.py:123-146), where omega and the angles are float32."""
    if channels % 8:
        raise RuntimeError("uv_embed_tables: channels must be a multiple of 8")
    diag = (aspect_ratio ** 2 + 1.0) ** 0.5
    span_x, span_y = aspect_ratio / diag, 1.0 / diag
    xs = torch.linspace(-span_x * (width - 1) / width, span_x * (width - 1) / width, steps=width, dtype=torch.float32)
    ys = torch.linspace(-span_y * (height - 1) / height, span_y * (height - 1) / height, steps=height, dtype=torch.float32)
    half = channels // 2
    adt = torch.float32 if f32_angles else torch.float64
    omega = torch.arange(half // 2, dtype=adt)
    omega /= half / 2.0
    omega = 1.0 / 100 ** omega

    def table(pos):
        ang = torch.einsum("m,d->md", pos.to(adt), omega)
        return (torch.cat([ang.sin(), ang.cos()], dim=1).float() * ratio).contiguous().to(device)
    return table(xs), table(ys)


def upsample_bilinear_ac_f32(x, H, W, tabs=None):
    """F.interpolate(bilinear, align_corners=True) of x [N,h,w,C] to [N,H,W,C], plus the separable embedding tabs = (xtab [W,C/2], ytab [H,C/2])"""
    xt, yt = tabs if tabs is not None else (None, None)
    _heads_in(x, xt, yt)
    N, h, w, C = x.shape
    if xt is not None and (tuple(xt.shape) != (W, C // 2) or tuple(yt.shape) != (H, C // 2)):
        raise RuntimeError("upsample_bilinear_ac_f32: embedding tables do not fit the output")
    out = torch.empty(N, H, W, C, device=x.device, dtype=torch.float32)
    _timed("upsample_bilinear_ac_f32", 4.0 * out.numel(), lambda: _lib.call("vgpa_upsample_bilinear_ac_f32", x, xt, yt, out, N, h, w, C, H, W, _stream()),
           unit="byte")
    return out


_DPT_ACT = {"exp": 0, "inv_log": 1}


def _tail_fits(name, x, H, W, w1_packed, w2, xt, yt, grid):
    """the shape checks the two tails share: x [N,h,w,C], w1_packed [3,3,C,32], w2 [od,32], the tables on the [H,W] output grid"""
    C, od = x.shape[3], w2.shape[0]
    if tuple(w1_packed.shape) != (3, 3, C, 32) or tuple(w2.shape) != (od, 32) or C % 16:
        raise RuntimeError(f"{name}: weights do not fit the input")
    if xt is not None and (tuple(xt.shape) != (W, C // 2) or tuple(yt.shape) != (H, C // 2)):
        raise RuntimeError(f"{name}: embedding tables do not fit the {grid}")


def dpt_tail_f32(x, H, W, w1_packed, b1, w2, b2, activation="exp", tabs=None):
    """The main end of the DPT heads (dpt.DPTBase._main_tail) in one launch: x [N,h,w,C] -> (preds [N,H,W,output_dim-1], conf [N,H,W]);
    w1_packed [3,3,C,32], w2 [output_dim,32]; confidence activation expp1"""
    xt, yt = tabs if tabs is not None else (None, None)
    _heads_in(x, xt, yt, w1_packed, b1, w2, b2)
    if activation not in _DPT_ACT:
        raise NotImplementedError(f"dpt_tail_f32: activation {activation!r} (exp and inv_log are built)")
    N, h, w, C = x.shape
    od = w2.shape[0]
    _tail_fits("dpt_tail_f32", x, H, W, w1_packed, w2, xt, yt, "output")
    preds = torch.empty(N, H, W, od - 1, device=x.device, dtype=torch.float32)
    conf = torch.empty(N, H, W, device=x.device, dtype=torch.float32)
    _timed("dpt_tail_f32", 2.0 * N * H * W * (9 * C * 32 + 32 * od),
           lambda: _lib.call("vgpa_dpt_tail_f32", x, xt, yt, w1_packed, b1, w2, b2, preds, conf, N, h, w, C, H, W, od, _DPT_ACT[activation], _stream()))
    return preds, conf


def dualdpt_aux_tail_f32(x, w1_packed, b1, ln_w, ln_b, eps, w2, b2, tabs=None):
    """The end of DualDPT's auxiliary branch (dualdpt.py:250-258) in one launch (csrc/dualdpt.hip): x [N,h,w,C] (+ tabs = (xtab [w,C/2], ytab [h,C/2]))
    -> conv3x3 C -> 32, LayerNorm(32) per pixel, ReLU, 1x1 conv 32 -> od as (preds [N,h,w,od-1] linear, conf [N,h,w] = 1 + exp); w1_packed [3,3,C,32],
    ln_w / ln_b [32], w2 [od,32]"""
    xt, yt = tabs if tabs is not None else (None, None)
    _heads_in(x, xt, yt, w1_packed, b1, ln_w, ln_b, w2, b2)
    N, h, w, C = x.shape
    od = w2.shape[0]
    if not 2 <= od <= 8:
        raise RuntimeError("dualdpt_aux_tail_f32: weights do not fit the input")
    _tail_fits("dualdpt_aux_tail_f32", x, h, w, w1_packed, w2, xt, yt, "map")
    if b1.numel() != 32 or ln_w.numel() != 32 or ln_b.numel() != 32 or b2.numel() != od:
        raise RuntimeError("dualdpt_aux_tail_f32: biases / LayerNorm parameters do not fit 32 hidden channels and the output width")
    preds = torch.empty(N, h, w, od - 1, device=x.device, dtype=torch.float32)
    conf = torch.empty(N, h, w, device=x.device, dtype=torch.float32)
    _timed("dualdpt_aux_tail_f32", 2.0 * N * h * w * (9 * C * 32 + 32 * od),
           lambda: _lib.call("vgpa_dualdpt_aux_tail_f32", x, xt, yt, w1_packed, b1, ln_w, ln_b, float(eps), w2, b2, preds, conf, N, h, w, C, od, _stream()))
    return preds, conf


def attn_small_f32(qkv, scale=None):
    """qkv [B,S,3,H,D] fp32 (a Linear's output, read in place) -> softmax(scale q k^T) v as [B,S,H*D]; S <= 128, D a multiple of 32"""
    _heads_in(qkv)
    B, S, three, H, D = qkv.shape
    if three != 3 or S > 128 or D % 32 or D > 256:
        raise RuntimeError(f"attn_small_f32: qkv {tuple(qkv.shape)} outside S <= 128, D in multiples of 32 up to 256")
    o = torch.empty(B, S, H * D, device=qkv.device, dtype=torch.float32)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    _timed("attn_small_f32", 4.0 * B * H * S * S * D,
           lambda: _lib.call("vgpa_attn_small_f32", q, k, v, S * 3 * H * D, D, 3 * H * D, o, B, H, S, D, float(scale if scale is not None else D ** -0.5),
                             _stream()))
    return o


# ---- DINOv2 token embedding (csrc/dino_embed.hip): forward only ----------------------------------------------------------------------------
def pack_patch_weight(conv_weight):
    """Conv2d weight [C, 3, p, p] of a kernel = stride patch projection -> [Kpad, C] fp32 contiguous: k = (channel, ky, kx) as the weight is laid
    out, zero rows up to the next multiple of 16 (the kernel walks K in 16-wide chunks)"""
    C = conv_weight.shape[0]
    w = conv_weight.detach().float().reshape(C, -1).t()
    K = w.shape[0]
    out = torch.zeros((K + 15) // 16 * 16, C, device=w.device, dtype=torch.float32)
    out[:K] = w
    return out


def dino_embed(images, w_packed, bias, cls, reg, pos, out_dtype=torch.bfloat16):
    """DinoVisionTransformer.prepare_tokens_with_masks(x, masks=None) in one launch.  images [N,3,H,W] fp32 | bf16; w_packed from pack_patch_weight;
    bias [C], cls [C] (or [1,1,C]), reg [R,C] | None, pos [1+P,C] (or [1,1+P,C]): fp32 -> tokens [N, 1+R+P, C] in out_dtype (fp32 | bf16):
    row 0 = cls + pos[0], rows 1..R = reg, row 1+R+j = W . patch_j + bias + pos[1+j]."""
    _req(images)
    for t in (w_packed, bias, cls, reg, pos):
        if t is not None:
            _req(t, torch.float32)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (images, w_packed, bias, cls, reg, pos)):
        raise RuntimeError("dino_embed is forward only: call it under torch.no_grad()")
    if images.dtype not in _DT or out_dtype not in _DT:
        raise RuntimeError(f"dino_embed: fp32 or bf16 images and output, got {images.dtype} -> {out_dtype}")
    N, three, H, W = images.shape
    Kpad, C = w_packed.shape
    if three != 3 or (Kpad // 3) < 1:
        raise RuntimeError(f"dino_embed: images {tuple(images.shape)} are not [N,3,H,W]")
    R = 0 if reg is None else reg.shape[-2]
    cls, pos = cls.reshape(-1), pos.reshape(-1, C)
    reg = None if reg is None else reg.reshape(R, C)
    p = next((c for c in range(1, 65) if (3 * c * c + 15) // 16 * 16 == Kpad and H % c == 0 and pos.shape[0] == 1 + (H // c) * (W // c)), None) \
        if W > 0 and H > 0 else None
    if p is None or W % p or bias.numel() != C or cls.numel() != C or C % 32:
        raise RuntimeError(f"dino_embed: weight {tuple(w_packed.shape)}, position table {tuple(pos.shape)} and images {tuple(images.shape)} do not "
                           "fit one patch size (H, W multiples of it; channels a multiple of 32)")
    P = (H // p) * (W // p)
    out = torch.empty(N, 1 + R + P, C, device=images.device, dtype=out_dtype)
    _timed("dino_embed", 2.0 * N * P * C * 3 * p * p,
           lambda: _lib.call("vgpa_dino_embed", images, _DT[images.dtype], w_packed, Kpad, bias, cls, reg, pos, out, _DT[out_dtype], N, H, W, p, C, R,
                             _stream()))
    return out


def stream_ln(x, y=None, gamma=None, ln_w=None, ln_b=None, eps=1e-6, n_dtype=torch.bfloat16):
    """The fp32 residual stream of the DINOv2 blocks: x fp32 [..., D]; with y (bf16) and gamma (fp32 [D]) x_new = x + gamma * y; with ln_w / ln_b
    n = LayerNorm(x_new or x) in n_dtype -> (x_new | None, n | None).  Forward only."""
    _req(x, torch.float32)
    for t, dt in ((y, torch.bfloat16), (gamma, torch.float32), (ln_w, torch.float32), (ln_b, torch.float32)):
        if t is not None:
            _req(t, dt)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, y, gamma, ln_w, ln_b)):
        raise RuntimeError("stream_ln is forward only: call it under torch.no_grad()")
    D = x.shape[-1]
    if (y is not None and y.shape != x.shape) or any(t is not None and t.numel() != D for t in (gamma, ln_w, ln_b)) or n_dtype not in _DT:
        raise RuntimeError("stream_ln: shapes of x, y, gamma and the LayerNorm parameters do not fit")
    x_new = torch.empty_like(x) if y is not None else None
    n = torch.empty(x.shape, device=x.device, dtype=n_dtype) if ln_w is not None else None
    M = x.numel() // D
    nbytes = 4.0 + (6.0 if y is not None else 0.0) + (0.0 if n is None else n.element_size())          # per element: x (+ y, x_new) (+ n)
    _timed("stream_ln_f32", nbytes * M * D,
           lambda: _lib.call("vgpa_stream_ln_f32", x, y, gamma, ln_w, ln_b, x_new, n, _DT[n_dtype], M, D, float(eps), _stream()), "byte")
    return x_new, n


# ---- LPIPS-VGG around the convolutions (csrc/lpips.hip): fp32, channels-last, forward only ------------------------------------------------
LPIPS_SHIFT = (-.030, -.088, -.188)     # lpips.ScalingLayer's buffers
LPIPS_SCALE = (.458, .448, .450)


def lpips_input_f32(x, shift=LPIPS_SHIFT, scale=LPIPS_SCALE, normalize=False, out=None):
    """ScalingLayer + layout change: x [N,3,H,W] in [-1,1] ([0,1] with `normalize`) -> [N,H,W,16], channels 0..2 = (x - shift) / scale, the rest 0.
    `out`: a contiguous [N,H,W,16] view to write into (the two halves of one batch)."""
    _heads_in(x, out)
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError(f"lpips_input_f32: expected [N,3,H,W], got {tuple(x.shape)}")
    N, _, H, W = x.shape
    if out is None:
        out = torch.empty(N, H, W, 16, device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (N, H, W, 16):
        raise RuntimeError("lpips_input_f32: `out` must be [N,H,W,16]")
    _timed("lpips_input_f32", 4.0 * (x.numel() + out.numel()),
           lambda: _lib.call("vgpa_lpips_input_f32", x, out, N, H, W, *[float(v) for v in shift], *[float(v) for v in scale], 1 if normalize else 0,
                             _stream()), "byte")
    return out


def maxpool2x2_f32(x, relu=False):
    """F.max_pool2d(relu?(x), 2, 2) of x [N,H,W,C] -> [N,H//2,W//2,C]"""
    _heads_in(x)
    N, H, W, C = x.shape
    if H < 2 or W < 2 or C % 4:
        raise RuntimeError(f"maxpool2x2_f32: needs H, W >= 2 and channels in multiples of 4, got {tuple(x.shape)}")
    out = torch.empty(N, H // 2, W // 2, C, device=x.device, dtype=torch.float32)
    _timed("maxpool2x2_f32", 4.0 * (4 * out.numel() + out.numel()),
           lambda: _lib.call("vgpa_maxpool2x2_f32", x, out, N, H, W, C, 1 if relu else 0, _stream()), "byte")
    return out


def lpips_layer_f32(f0, f1, w, relu=False, total=None, accumulate=False, out=None):
    """One LPIPS layer of f0, f1 [N,H,W,C] with the lin weight w [C]: the spatial mean of sum_c w_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2
    -> fp32 [N] (written into `out` when given).  `total` (fp64 [N]) receives the unrounded value too, added to what it holds with `accumulate`."""
    _heads_in(f0, f1, w, out)
    N, H, W, C = f0.shape
    if f1.shape != f0.shape or w.numel() != C or C % 4 or C > 512:
        raise RuntimeError(f"lpips_layer_f32: maps {tuple(f0.shape)} / {tuple(f1.shape)} and weight {tuple(w.shape)} do not fit (C % 4 == 0, C <= 512)")
    if total is not None:
        _req(total, torch.float64)
        if total.numel() != N:
            raise RuntimeError("lpips_layer_f32: `total` must hold N values")
    if out is None:
        out = torch.empty(N, device=f0.device, dtype=torch.float32)
    elif out.numel() != N:
        raise RuntimeError("lpips_layer_f32: `out` must hold N values")
    ws_bytes = _lib.query("vgpa_lpips_layer_workspace_bytes", N, H, W, C)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=f0.device)
    _timed("lpips_layer_f32", 2.0 * f0.numel() * 4,
           lambda: _lib.call("vgpa_lpips_layer_f32", f0, f1, w, out, total, N, H, W, C, (1 if relu else 0) | (2 if accumulate else 0), ws, ws_bytes,
                             _stream()), "byte")
    return out


# ---- CogVideoX VAE encoder: its convolutions (csrc/vae_conv.hip) and what stands around them (csrc/vae.hip): fp32, channels-last, forward only ---
def _dtype_code(dtype, name):
    if dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"{name}: float32 or bfloat16, got {dtype}")
    return 1 if dtype == torch.bfloat16 else 0


def conv3x3_pad_f32(x, w_packed, bias=None, res=None, stride=1, pad_lo=1, pad_hi=1):
    """x [N,H,W,Cin] -> conv3x3(x, stride) + bias? + res? with `pad_lo` zero rows / columns in front and `pad_hi` behind (each 0 or 1):
    [N,Ho,Wo,Cout], Ho = (H + pad_lo + pad_hi - 3) // stride + 1.  CogVideoXDownsample3D is stride 2, pad_lo 0, pad_hi 1.  The convolution of the
    VAE encoder: the sum over the 9 Cin products runs in chains of 64 that are added up afterwards (csrc/conv_mfma.h, CV_CONV_CHUNKED), so its rounding
    error is a fraction of conv3x3_f32's single chain at the same speed class; the two agree to that rounding, not bit for bit."""
    _heads_in(x, w_packed, bias, res)
    N, H, W, Cin = x.shape
    bad = stride not in (1, 2) or pad_lo not in (0, 1) or pad_hi not in (0, 1) or min(H, W) + pad_lo + pad_hi < 3
    out = _conv_out("conv3x3_pad_f32", x, w_packed, (3, 3),
                    () if bad else (N, (H + pad_lo + pad_hi - 3) // stride + 1, (W + pad_lo + pad_hi - 3) // stride + 1), res,
                    refuse=f"stride {stride}, padding ({pad_lo}, {pad_hi}) on a {H} x {W} map is not supported" if bad else None)
    _timed("conv3x3_pad_f32", 2.0 * out.numel() * 9 * Cin,
           lambda: _lib.call("vgpa_conv3x3_pad_f32", x, w_packed, bias, res, out, N, H, W, Cin, out.shape[-1], stride, pad_lo, pad_hi, _stream()))
    return out


def pack_conv3d_weight(w):
    """Conv3d weight [Cout, Cin, kt, kh, kw] -> [kt][kh][kw][Cin][Cout] fp32 contiguous, the layout conv3d_causal_f32 reads"""
    return w.detach().float().permute(2, 3, 4, 1, 0).contiguous()


def conv3d_causal_f32(x, w_packed, bias=None, res=None, prev=None):
    """CogVideoXCausalConv3d over the frames of a chunk: x [N,T,H,W,Cin] -> conv3x3x3(x) + bias? + res? as [N,T,H,W,Cout], stride 1, spatial zero
    padding 1; w_packed [3,3,3,Cin,Cout].  Temporal tap kt of output frame t reads frame t + kt - 2: in front of frame 0 that is `prev`
    [N,2,H,W,Cin] (the last two input frames of the chunk before, diffusers' conv_cache) or, with prev None, frame 0 again.  Every output sums in
    the same order whatever N, T and prev are (runs of 64 products, csrc/conv_mfma.h CV_CONV3D), so a call over T frames equals its split into
    two calls bit for bit when the second gets x[:, -2:] of the first as `prev`."""
    _heads_in(x, w_packed, bias, res, prev)
    if x.dim() != 5:
        raise RuntimeError(f"conv3d_causal_f32: expected [N,T,H,W,Cin], got {tuple(x.shape)}")
    N, T, H, W, Cin = x.shape
    bad = prev is not None and tuple(prev.shape) != (N, 2, H, W, Cin)
    out = _conv_out("conv3d_causal_f32", x, w_packed, (3, 3, 3), (N, T, H, W), res,
                    refuse=f"prev {tuple(prev.shape)} is not [{N},2,{H},{W},{Cin}]" if bad else None)
    _timed("conv3d_causal_f32", 2.0 * out.numel() * 27 * Cin,
           lambda: _lib.call("vgpa_conv3x3x3_causal_f32", x, prev, w_packed, bias, res, out, N, T, H, W, Cin, out.shape[-1], _stream()))
    return out


def vae_downsample_f32(x, w_packed, bias=None, compress_time=True):
    """CogVideoXDownsample3D in one launch: x [N,T,H,W,C] -> [N,T',Ho,Wo,Cout], conv3x3_pad_f32(stride 2, pad_lo 0, pad_hi 1) of every temporally
    pooled frame, which the loader forms as (a + b) * 0.5 and never writes.  T' = T without compress_time, else (T + 1) // 2: an even T pools
    frames (2t', 2t' + 1); an odd T keeps frame 0 and pools (2t' - 1, 2t').  Bit for bit pooling first and conv3x3_pad_f32 after it."""
    _heads_in(x, w_packed, bias)
    if x.dim() != 5:
        raise RuntimeError(f"vae_downsample_f32: expected [N,T,H,W,C], got {tuple(x.shape)}")
    N, T, H, W, C = x.shape
    out = _conv_out("vae_downsample_f32", x, w_packed, (3, 3), (N, (T + 1) // 2 if compress_time else T, (H - 2) // 2 + 1, (W - 2) // 2 + 1),
                    refuse=f"a {H} x {W} map is too small" if min(H, W) < 2 else None)
    _timed("vae_downsample_f32", 2.0 * out.numel() * 9 * C,
           lambda: _lib.call("vgpa_vae_downsample_f32", x, w_packed, bias, out, N, T, H, W, C, out.shape[-1], 1 if compress_time else 0, _stream()))
    return out


def vae_input_f32(x):
    """x [N,3,H,W] (fp32 or bf16) -> fp32 [N,H,W,16], channels 3..15 zero: the input of the 16-channel form of the 3-channel stem"""
    _req(x)
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError(f"vae_input_f32: expected [N,3,H,W], got {tuple(x.shape)}")
    N, _, H, W = x.shape
    out = torch.empty(N, H, W, 16, device=x.device, dtype=torch.float32)
    _timed("vae_input_f32", float(x.numel() * x.element_size() + 4 * out.numel()),
           lambda: _lib.call("vgpa_vae_input_f32", x, _dtype_code(x.dtype, "vae_input_f32"), out, N, H, W, _stream()), "byte")
    return out


def groupnorm_stats_f32(x, groups, eps):
    """x [N,...,C] channels-last -> fp32 [N,groups,2] = (mean, rstd) of every (sample, group of C / groups neighbouring channels)"""
    _heads_in(x)
    N, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (N * C)
    if C % 4 or C % groups or C > 1024:
        raise RuntimeError(f"groupnorm_stats_f32: {C} channels in {groups} groups is not supported (C a multiple of 4 and of the groups, <= 1024)")
    stats = torch.empty(N, groups, 2, device=x.device, dtype=torch.float32)
    ws_bytes = _lib.query("vgpa_groupnorm_stats_workspace_bytes", N, HW, C, groups)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    _timed("groupnorm_stats_f32", 4.0 * x.numel(),
           lambda: _lib.call("vgpa_groupnorm_stats_f32", x, stats, N, HW, C, groups, float(eps), ws, ws_bytes, _stream()), "byte")
    return stats


def groupnorm_silu_f32(x, gamma, beta, groups, eps, stats=None):
    """silu(F.group_norm(x, groups, gamma, beta, eps)) of x [N,...,C] channels-last, same shape; `stats` from groupnorm_stats_f32, computed when None"""
    _heads_in(x, gamma, beta, stats)
    N, C = x.shape[0], x.shape[-1]
    if gamma.numel() != C or beta.numel() != C:
        raise RuntimeError(f"groupnorm_silu_f32: gamma / beta do not hold {C} values")
    if stats is None:
        stats = groupnorm_stats_f32(x, groups, eps)
    elif tuple(stats.shape) != (N, groups, 2):
        raise RuntimeError(f"groupnorm_silu_f32: `stats` must be [{N},{groups},2]")
    out = torch.empty_like(x)
    _timed("groupnorm_silu_f32", 8.0 * x.numel(),
           lambda: _lib.call("vgpa_groupnorm_silu_f32", x, stats, gamma, beta, out, N, x.numel() // (N * C), C, groups, _stream()), "byte")
    return out


def vae_sample(moments, noise=None, scale=1.0, dtype=torch.float32, want=("sample",)):
    """moments fp32 [N,h,w,2L] (one frame) or [N,T,h,w,2L] -> dict of the requested [N,L,T,h,w] tensors in `dtype` (T = 1 for the 4-D form): "mean",
    "logvar" (clamped to [-30, 20]), "std" = exp(logvar / 2), "sample" = (mean + std * noise) * scale with noise [N,L,T,h,w] in `dtype` (None: no noise)"""
    _heads_in(moments)
    if moments.dim() not in (4, 5):
        raise RuntimeError(f"vae_sample: moments {tuple(moments.shape)} are neither [N,h,w,2L] nor [N,T,h,w,2L]")
    shape = tuple(moments.shape)
    N, T, h, w, L2 = shape if len(shape) == 5 else (shape[0], 1) + shape[1:]
    L = L2 // 2
    if L2 % 2 or not want or any(k not in ("sample", "mean", "logvar", "std") for k in want):
        raise RuntimeError(f"vae_sample: moments {tuple(moments.shape)}, outputs {want!r}")
    if noise is not None:
        _req(noise, dtype)
        if tuple(noise.shape) != (N, L, T, h, w):
            raise RuntimeError(f"vae_sample: noise {tuple(noise.shape)} is not [{N},{L},{T},{h},{w}]")
    out = {k: torch.empty(N, L, T, h, w, device=moments.device, dtype=dtype) for k in want}
    _timed("vae_sample", 4.0 * moments.numel(),
           lambda: _lib.call("vgpa_vae_sample", moments, noise, float(scale), out.get("sample"), out.get("mean"), out.get("logvar"), out.get("std"),
                             _dtype_code(dtype, "vae_sample"), N, T * h * w, L, _stream()), "byte")
    return out


# ---- CogVideoX VAE decoder: the entry points above plus these three ------------------------------------------------------------------------
def vae_upsample_frames(T, compress_time):
    """frames CogVideoXUpsample3D leaves of T: T without compress_time or of one frame, 2T of an even count, 2T - 1 of an odd one (frame 0 stays single)"""
    return T if not compress_time or T == 1 else 2 * T - 1 if T % 2 else 2 * T


def vae_upsample_f32(x, w_packed, bias=None, compress_time=True):
    """CogVideoXUpsample3D in one launch: x [N,T,H,W,C] -> [N,T',2H,2W,Cout], conv3x3_pad_f32 (padding 1) of the nearest-neighbour x2 map, which the
    loader reads as source pixel (y >> 1, x >> 1) of source frame f(t') and never writes.  T' = vae_upsample_frames(T, compress_time); f(t') = t'
    (T' = T), t' >> 1 (T' = 2T), or 0 for t' = 0 and 1 + (t' - 1) // 2 after it (T' = 2T - 1).  Bit for bit up-sampling first and conv3x3_pad_f32
    after it."""
    _heads_in(x, w_packed, bias)
    if x.dim() != 5:
        raise RuntimeError(f"vae_upsample_f32: expected [N,T,H,W,C], got {tuple(x.shape)}")
    N, T, H, W, C = x.shape
    out = _conv_out("vae_upsample_f32", x, w_packed, (3, 3), (N, vae_upsample_frames(T, compress_time), 2 * H, 2 * W))
    _timed("vae_upsample_f32", 2.0 * out.numel() * 9 * C,
           lambda: _lib.call("vgpa_vae_upsample_f32", x, w_packed, bias, out, N, T, H, W, C, out.shape[-1], 1 if compress_time else 0, _stream()))
    return out


def spatial_norm_silu_f32(f, stats, gamma, beta, yb):
    """silu(CogVideoXSpatialNorm3D(f, zq)) of f [N,T,H,W,C] channels-last: silu(((f - mean) * rstd * gamma + beta) * Y + B), `stats` [N,G,2] from
    groupnorm_stats_f32, yb [N,t,h,w,2C] = (Y | B) = conv_y | conv_b of the latent zq at ITS resolution (one conv1x1_f32 with the two weights side
    by side).  The nearest-neighbour resize to (T,H,W) is a gather in the kernel -- a 1x1 convolution commutes with it exactly -- with upstream's
    special case: an odd T > 1 takes frame 0 from latent frame 0 and resizes the other frames on their own.  H, W must be multiples of h, w."""
    _heads_in(f, stats, gamma, beta, yb)
    if f.dim() != 5 or yb.dim() != 5:
        raise RuntimeError(f"spatial_norm_silu_f32: expected f [N,T,H,W,C] and yb [N,t,h,w,2C], got {tuple(f.shape)} and {tuple(yb.shape)}")
    N, T, H, W, C = f.shape
    n, t, h, w, C2 = yb.shape
    if n != N or C2 != 2 * C or gamma.numel() != C or beta.numel() != C or stats.dim() != 3 or stats.shape[0] != N or stats.shape[2] != 2:
        raise RuntimeError(f"spatial_norm_silu_f32: f {tuple(f.shape)}, yb {tuple(yb.shape)}, stats {tuple(stats.shape)} and gamma / beta do not fit")
    G = stats.shape[1]
    if C % 4 or C % G or C > 1024:
        raise RuntimeError(f"spatial_norm_silu_f32: {C} channels in {G} groups is not supported (C a multiple of 4 and of the groups, <= 1024)")
    if H % h or W % w:
        raise RuntimeError(f"spatial_norm_silu_f32: a {H} x {W} map over a {h} x {w} latent: the ratios must be integral")
    if t > T or (T > 1 and T % 2 and t < 2):
        raise RuntimeError(f"spatial_norm_silu_f32: {t} latent frames do not resize to {T} frames (an odd count takes its frame 0 aside)")
    out = torch.empty_like(f)
    _timed("spatial_norm_silu_f32", 8.0 * f.numel(),
           lambda: _lib.call("vgpa_spatial_norm_silu_f32", f, stats, gamma, beta, yb, out, N, T, H, W, C, G, t, h, w, _stream()), "byte")
    return out


def vae_output(x, dtype=torch.float32, uint8=False):
    """behind the decoder's conv_out (3 channels padded to 16): x fp32 [N,T,H,W,16] -> [N,3,T,H,W] in `dtype` (fp32 | bf16), channels 0..2 rounded
    once -- the inverse of vae_input_f32.  uint8=True: the pipeline's postprocess_video instead, [N,T,H,W,3] uint8 =
    round(clamp(x / 2 + 0.5, 0, 1) * 255), the layout the scorer's frame input takes."""
    _heads_in(x)
    if x.dim() != 5 or x.shape[-1] != 16:
        raise RuntimeError(f"vae_output: expected [N,T,H,W,16], got {tuple(x.shape)}")
    N, T, H, W, _ = x.shape
    if uint8:
        out, code = torch.empty(N, T, H, W, 3, device=x.device, dtype=torch.uint8), 2
    else:
        out, code = torch.empty(N, 3, T, H, W, device=x.device, dtype=dtype), _dtype_code(dtype, "vae_output")
    _timed("vae_output", 4.0 * x.numel() + out.numel() * out.element_size(),
           lambda: _lib.call("vgpa_vae_output", x, out, code, N, T * H * W, _stream()), "byte")
    return out


# ---- Depth Anything 3's backbone between its blocks, and its camera decoding (csrc/da3.hip): fp32, forward only ---------------------------
DA3_REF_VIEW_STRATEGIES = {"first": 0, "middle": 1, "saddle_balanced": 2, "saddle_sim_range": 3}


def _da3_tokens(name, x, *more):
    _req(x, torch.float32)
    if x.dim() != 4:
        raise RuntimeError(f"{name}: tokens are fp32 [B,S,N,C], got {tuple(x.shape)}")
    for t in more:
        if t is not None:
            _req(t, torch.float32)
            if t.shape != x.shape:
                raise RuntimeError(f"{name}: the two token tensors do not fit ({tuple(x.shape)}, {tuple(t.shape)})")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, *more)):
        raise RuntimeError(f"{name} is forward only: call it under torch.no_grad()")
    return x.shape


def _da3_ref(name, ref_idx, B):
    _req(ref_idx, torch.int32)
    if ref_idx.numel() != B:
        raise RuntimeError(f"{name}: ref_idx is a device int32 [B]")
    return ref_idx


def da3_ref_view(x, strategy="saddle_balanced", return_metrics=False):
    """select_reference_view on token 0 of x fp32 [B,S,N,C] -> ref_idx, a DEVICE int32 [B] (it is never read on the host; the kernels below take it as it
    is).  return_metrics: also fp64 [B,S,4] = (mean off-diagonal cosine similarity, norm, variance of the normalised token, ranking score) per view."""
    B, S, N, C = _da3_tokens("da3_ref_view", x)
    if strategy not in DA3_REF_VIEW_STRATEGIES:
        raise ValueError(f"Unknown reference view selection strategy: {strategy}. Must be one of: {', '.join(map(repr, DA3_REF_VIEW_STRATEGIES))}")
    ref_idx = torch.empty(B, device=x.device, dtype=torch.int32)
    metrics = torch.empty(B, S, 4, device=x.device, dtype=torch.float64) if return_metrics else None
    _timed("da3_ref_view", 4.0 * B * S * C, lambda: _lib.call("vgpa_da3_ref_view", x, B, S, N, C, DA3_REF_VIEW_STRATEGIES[strategy], metrics, ref_idx,
                                                               _stream()), "byte")
    return (ref_idx, metrics) if return_metrics else ref_idx


def da3_view_gather(x, ref_idx, other=None, inverse=False):
    """reorder_by_reference (inverse: restore_original_order) of x fp32 [B,S,N,C] -- and of `other`, same shape, in the same launch -- into new tensors:
    -> reordered x, or (x, other)"""
    B, S, N, C = _da3_tokens("da3_view_gather", x, other)
    _da3_ref("da3_view_gather", ref_idx, B)
    out = torch.empty_like(x)
    out2 = None if other is None else torch.empty_like(other)
    _timed("da3_view_gather", 8.0 * x.numel() * (1 if other is None else 2),
           lambda: _lib.call("vgpa_da3_view_gather", x, out, other, out2, ref_idx, 1 if inverse else 0, B, S, N, C, _stream()), "byte")
    return out if other is None else (out, out2)


def da3_cam_token(x, cam, per_view):
    """x[:, :, 0] = cam IN PLACE.  per_view: cam fp32 [B,S,C], one token per view (the caller's); else cam is the camera_token parameter [1,2,C]: row 0
    for view 0 and row 1 for every other view.  -> x"""
    B, S, N, C = _da3_tokens("da3_cam_token", x)
    _req(cam, torch.float32)
    if tuple(cam.shape) != ((B, S, C) if per_view else (1, 2, C)):
        raise RuntimeError(f"da3_cam_token: cam {tuple(cam.shape)} is not {'[B,S,C]' if per_view else 'the camera_token parameter [1,2,C]'}")
    _timed("da3_cam_token", 8.0 * B * S * C, lambda: _lib.call("vgpa_da3_cam_token", x, cam, 1 if per_view else 0, B, S, N, C, _stream()), "byte")
    return x


def da3_tap(local_x, x, ln_w, ln_b, eps=1e-5, ref_idx=None):
    """One out layer of the backbone: -> (features fp32 [B,S,N-1,2C] = [local_x | LayerNorm(x)] of tokens 1.., camera token fp32 [B,S,2C] = [local_x | x]
    of token 0), views restored to their original order when ref_idx (device int32 [B]) is given"""
    B, S, N, C = _da3_tokens("da3_tap", x, local_x)
    for t in (ln_w, ln_b):
        _req(t, torch.float32)
    if ln_w.numel() != C or ln_b.numel() != C:
        raise RuntimeError("da3_tap: the LayerNorm parameters do not fit the tokens")
    if ref_idx is not None:
        _da3_ref("da3_tap", ref_idx, B)
    feats = torch.empty(B, S, N - 1, 2 * C, device=x.device, dtype=torch.float32)
    cam = torch.empty(B, S, 2 * C, device=x.device, dtype=torch.float32)
    _timed("da3_tap", 16.0 * x.numel(), lambda: _lib.call("vgpa_da3_tap", local_x, x, ln_w, ln_b, float(eps), ref_idx, feats if N > 1 else None, cam,
                                                          B, S, N, C, _stream()), "byte")
    return feats, cam


def da3_pose_decode(pose_enc, image_size_hw):
    """pose_enc fp32 [..., 9] (camera-to-world) -> (extrinsics fp32 [..., 3, 4] world-to-camera, intrinsics fp32 [..., 3, 3])"""
    _req(pose_enc, torch.float32)
    if pose_enc.shape[-1] != 9 or pose_enc.numel() == 0:
        raise RuntimeError(f"da3_pose_decode: pose encodings are [..., 9], got {tuple(pose_enc.shape)}")
    if torch.is_grad_enabled() and pose_enc.requires_grad:
        raise RuntimeError("da3_pose_decode is forward only: call it under torch.no_grad()")
    lead, n = pose_enc.shape[:-1], pose_enc.numel() // 9
    ext = torch.empty(*lead, 3, 4, device=pose_enc.device, dtype=torch.float32)
    intr = torch.empty(*lead, 3, 3, device=pose_enc.device, dtype=torch.float32)
    H, W = image_size_hw
    _timed("da3_pose_decode", 4.0 * n * 30, lambda: _lib.call("vgpa_da3_pose_decode", pose_enc, n, float(H), float(W), ext, intr, _stream()), "byte")
    return ext, intr


# ray-based cameras (csrc/da3_ray_pose.hip; depth_anything_3/utils/ray_utils.py:313-432): upstream's constants
DA3_RAY_N_ITER, DA3_RAY_SAMPLES, DA3_RAY_SAMPLE_RATIO, DA3_RAY_MAX_INLIERS, DA3_RAY_Z_THRESHOLD = 100, 8, 0.3, 8000, 1e-4
_DA3_RAY_GRIDS = {}


def da3_ray_grid(ph, pw):
    """The source points of the ray-pose homography: the identity camera's plane grid of `unproject_depth(..., ixt_normalized=True)` (utils/geometry.py:
    461-487 through the inverse of K = [[1,0,1],[0,1,1],[0,0,1]]) -> host fp32 (x [pw], y [ph]), cell centres in (-1, 1); z is 1.  A host fp32 linspace
    minus 1, which is bit for bit what upstream's CPU run builds."""
    axis = lambda n: torch.linspace(-(1 - 1 / n) + 1.0, (1 - 1 / n) + 1.0, n, dtype=torch.float32) - 1.0
    return axis(pw), axis(ph)


def da3_ray_sample_table(n_sample, generator=None, device=None, n_iter=DA3_RAY_N_ITER):
    """The RANSAC sample table: int32 [n_iter, 8] on `device`, every row 8 distinct positions in [0, n_sample) drawn uniformly (the 8 largest of n_sample
    uniform numbers: the first 8 of a random permutation, which is what upstream's randperm(n_sample)[:8] per row is) from `generator`, on the
    generator's own device; None: the default generator of `device`"""
    if n_sample < DA3_RAY_SAMPLES:
        raise ValueError(f"da3_ray_sample_table: {DA3_RAY_SAMPLES} distinct samples need n_sample >= {DA3_RAY_SAMPLES}, got {n_sample}")
    src = generator.device if generator is not None else device
    keys = torch.rand(n_iter, n_sample, generator=generator, device=src)
    return keys.topk(DA3_RAY_SAMPLES, dim=1).indices.to(device=device, dtype=torch.int32).contiguous()


def da3_ray_pose(ray, ray_conf, image_hw, sample_idx=None, generator=None, reproj_threshold=0.2):
    """DepthAnything3Net._process_ray_pose_estimation (da3.py:181-201 over ray_utils.get_extrinsic_from_camray): ray fp32 [B,S,ph,pw,6] and ray_conf fp32
    [B,S,ph,pw] of the auxiliary DualDPT branch -> (extrinsics fp32 [B,S,3,4] world-to-camera, intrinsics fp32 [B,S,3,3] in pixels of image_hw, info).
    Per view: the top max(8, int(0.3 N)) points by masked confidence (ties: lower index first) are the candidates, `sample_idx` (integer [n_iter, 8]
    positions among them; None: da3_ray_sample_table from `generator`) picks 8 per hypothesis, the hypothesis with the largest inlier weight wins and
    is refitted on its inliers -- on a random 8000 of the top 95 % by weight when there are more, drawn from `generator`.  Neither input is written
    (upstream zeroes the masked confidences in place; their effect on T is reproduced).  info: R [B,S,3,3], T [B,S,3], focal and pp [B,S,2]
    (normalised), H [B,S,3,3] (the refitted homography), best, n_inliers, n_used int32 [B,S], sample_idx int32 [n_iter,8].  Reads n_inliers back once;
    a view with fewer than 4 inliers raises ValueError, as upstream."""
    _req(ray, torch.float32)
    _req(ray_conf, torch.float32)
    if ray.dim() != 5 or ray.shape[-1] != 6 or tuple(ray_conf.shape) != tuple(ray.shape[:-1]) or ray.numel() == 0:
        raise RuntimeError(f"da3_ray_pose: ray [B,S,ph,pw,6] and ray_conf [B,S,ph,pw], got {tuple(ray.shape)} and {tuple(ray_conf.shape)}")
    if torch.is_grad_enabled() and (ray.requires_grad or ray_conf.requires_grad):
        raise RuntimeError("da3_ray_pose is forward only: call it under torch.no_grad()")
    B, S, ph, pw, _ = ray.shape
    V, N, dev = B * S, ph * pw, ray.device
    if N < DA3_RAY_SAMPLES:
        raise RuntimeError(f"da3_ray_pose: a ray map of {N} points cannot give {DA3_RAY_SAMPLES} samples")
    n_sample = max(DA3_RAY_SAMPLES, int(N * DA3_RAY_SAMPLE_RATIO))
    if sample_idx is None:
        sample_idx = da3_ray_sample_table(n_sample, generator, dev)
    else:
        if sample_idx.dim() != 2 or sample_idx.shape[1] != DA3_RAY_SAMPLES or sample_idx.is_floating_point():
            raise RuntimeError(f"da3_ray_pose: sample_idx is an integer table [n_iter, {DA3_RAY_SAMPLES}], got {tuple(sample_idx.shape)} {sample_idx.dtype}")
        sample_idx = sample_idx.to(device=dev, dtype=torch.int32).contiguous()
    n_iter = sample_idx.shape[0]
    key = (ph, pw, str(dev))
    if key not in _DA3_RAY_GRIDS:
        if len(_DA3_RAY_GRIDS) > 16:
            _DA3_RAY_GRIDS.clear()
        _DA3_RAY_GRIDS[key] = tuple(t.to(dev) for t in da3_ray_grid(ph, pw))
    gx, gy = _DA3_RAY_GRIDS[key]
    z_thr, H, W = DA3_RAY_Z_THRESHOLD, *image_hw

    wm = torch.empty(V, N, device=dev, dtype=torch.float32)
    _timed("da3_ray_weights", 32.0 * V * N, lambda: _lib.call("vgpa_da3_ray_weights", ray, ray_conf, V, N, z_thr, wm, _stream()), "byte")
    order = torch.sort(wm, dim=1, descending=True, stable=True).indices                       # ties: the lower index first
    cand = order[:, :n_sample].to(torch.int32).contiguous()
    ws_bytes = _lib.query("vgpa_da3_ray_pose_workspace_bytes", V, N, n_iter)
    if ws_bytes == 0:
        raise RuntimeError(f"da3_ray_pose: {V} views x {N} points x {n_iter} hypotheses is outside what the kernels take (n_iter <= 128)")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    best = torch.empty(V, device=dev, dtype=torch.int32)
    n_inl = torch.empty(V, device=dev, dtype=torch.int32)
    inlier = torch.empty(V, N, device=dev, dtype=torch.uint8)
    _timed("da3_ray_ransac", 30.0 * V * n_iter * N,
           lambda: _lib.call("vgpa_da3_ray_ransac", ray, wm, gx, gy, cand, sample_idx, V, ph, pw, n_sample, n_iter, z_thr, float(reproj_threshold), best,
                             inlier, n_inl, ws, ws_bytes, _stream()))
    counts = n_inl.tolist()                                    # the one read-back: the refit's subset sizes are host arithmetic, as upstream's
    if min(counts) < 4:
        raise ValueError("At least 4 points are required to compute homography.")
    use = inlier
    if max(counts) > DA3_RAY_MAX_INLIERS:                      # a random 8000 of the top 95 % by weight (ray_utils.py:402-411), view after view
        use = inlier.clone()
        for v, n in enumerate(counts):
            if n <= DA3_RAY_MAX_INLIERS:
                continue
            keep_len = max(int(n * 0.95), DA3_RAY_MAX_INLIERS)
            by_weight = torch.sort(torch.where(inlier[v].bool(), wm[v], wm.new_tensor(float("-inf"))), descending=True, stable=True).indices[:keep_len]
            perm = torch.randperm(keep_len, generator=generator, device=generator.device if generator is not None else dev)[:DA3_RAY_MAX_INLIERS]
            use[v].zero_()
            use[v, by_weight[perm.to(dev)]] = 1
    out = {k: torch.empty(B, S, *shape, device=dev, dtype=torch.float32)
           for k, shape in (("H", (3, 3)), ("R", (3, 3)), ("T", (3,)), ("focal", (2,)), ("pp", (2,)), ("extrinsics", (3, 4)), ("intrinsics", (3, 3)))}
    n_used = torch.empty(V, device=dev, dtype=torch.int32)
    _timed("da3_ray_refit", 32.0 * V * N,
           lambda: _lib.call("vgpa_da3_ray_refit", ray, wm, gx, gy, use, V, ph, pw, z_thr, float(H), float(W), out["H"], out["R"], out["T"], out["focal"],
                             out["pp"], out["extrinsics"], out["intrinsics"], n_used, _stream()), "byte")
    ext, intr = out.pop("extrinsics"), out.pop("intrinsics")
    out.update(best=best.view(B, S), n_inliers=n_inl.view(B, S), n_used=n_used.view(B, S), sample_idx=sample_idx)
    return ext, intr, out


# ---- T5 encoder between its GEMMs (csrc/t5.hip): forward only -------------------------------------------------------------------------------
T5_MAX_S = 512


def _t5_forward_only(name, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError(f"{name} is forward only: call it under torch.no_grad()")


def t5_attention(q, k, v, bias_delta, mask=None):
    """softmax(q k^T + bias[h][j - i] + mask[b][j]) v, no 1/sqrt(d) scale.  q, k, v bf16 [B,S,H,64] views (slices of the fused QKV GEMM output, read in
    place; last dim contiguous); bias_delta fp32 [H, 2S-1] indexed by j - i + S - 1; mask None | uint8 / bool [B,S], 1 = keep (every sample must keep
    a key) -> o bf16 [B,S,H*64].  S <= 512."""
    for t in (q, k, v):
        _req(t, torch.bfloat16, contiguous=False)
    _req(bias_delta, torch.float32)
    _t5_forward_only("t5_attention", q, k, v, bias_delta)
    if q.dim() != 4 or q.shape[-1] != 64 or k.shape != q.shape or v.shape != q.shape or any(t.stride(3) != 1 for t in (q, k, v)):
        raise RuntimeError(f"t5_attention: q, k, v must be [B,S,H,64] views with a contiguous last dim, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    B, S, H, _ = q.shape
    if S < 1 or S > T5_MAX_S:
        raise RuntimeError(f"t5_attention: 1 <= S <= {T5_MAX_S}, got {S}")
    if tuple(bias_delta.shape) != (H, 2 * S - 1):
        raise RuntimeError(f"t5_attention: bias_delta must be [H, 2S-1] = {(H, 2 * S - 1)}, got {tuple(bias_delta.shape)}")
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8) if mask.is_contiguous() else mask.to(torch.uint8)
        _req(mask, torch.uint8)
        if tuple(mask.shape) != (B, S):
            raise RuntimeError(f"t5_attention: mask must be [B,S] = {(B, S)}, got {tuple(mask.shape)}")
    o = torch.empty(B, S, H * 64, device=q.device, dtype=torch.bfloat16)
    st = [_i64x3(t.stride(0), t.stride(2), t.stride(1)) for t in (q, k, v)]
    _timed("t5_attn_fwd", 4.0 * B * H * S * S * 64,
           lambda: _lib.call("vgpa_t5_attn_fwd", q, k, v, st[0], st[1], st[2], bias_delta, mask, o, B, H, S, _stream()))
    return o


def t5_rms(x, w, y=None, eps=1e-6, n_dtype=torch.bfloat16, keep_stream=True):
    """The fp32 residual stream with T5LayerNorm: x fp32 [..., D], y (bf16, the GEMM output in front) or None; x_new = x + y;
    n = w * x_new * rsqrt(mean(x_new^2) + eps) in n_dtype (w fp32 [D]) -> (x_new | None, n).  x_new is None without y, and with keep_stream=False
    (the final norm, behind which nobody reads the stream).  D a multiple of 64, at most 4096."""
    _req(x, torch.float32)
    _req(w, torch.float32)
    if y is not None:
        _req(y, torch.bfloat16)
    _t5_forward_only("t5_rms", x, y, w)
    D = x.shape[-1]
    if D % 64 or D > 4096 or w.numel() != D or (y is not None and y.shape != x.shape) or n_dtype not in _DT or x.numel() == 0:
        raise RuntimeError(f"t5_rms: x {tuple(x.shape)}, y and w {tuple(w.shape)} do not fit (D a multiple of 64, at most 4096; fp32 or bf16 output)")
    x_new = torch.empty_like(x) if (y is not None and keep_stream) else None
    n = torch.empty(x.shape, device=x.device, dtype=n_dtype)
    M = x.numel() // D
    nbytes = 4.0 + (2.0 if y is not None else 0.0) + (4.0 if x_new is not None else 0.0) + n.element_size()
    _timed("t5_rms", nbytes * M * D, lambda: _lib.call("vgpa_t5_rms", x, y, None, None, 0, w, x_new, n, _DT[n_dtype], M, D, float(eps), _stream()), "byte")
    return x_new, n


def t5_embed_rms(ids, table, w, eps=1e-6):
    """The first norm of the network fused with the embedding gather: ids int64 [...], table bf16 [V,D], w fp32 [D] ->
    (x fp32 [..., D] = table[ids], n bf16 = T5LayerNorm(x)).  An id outside [0,V) gives a row of NaN."""
    _req(ids, torch.int64)
    _req(table, torch.bfloat16)
    _req(w, torch.float32)
    _t5_forward_only("t5_embed_rms", table, w)
    if table.dim() != 2 or table.shape[1] % 64 or table.shape[1] > 4096 or w.numel() != table.shape[1] or ids.numel() == 0:
        raise RuntimeError(f"t5_embed_rms: table {tuple(table.shape)} and w {tuple(w.shape)} do not fit (D a multiple of 64, at most 4096)")
    V, D = table.shape
    M = ids.numel()
    x = torch.empty(*ids.shape, D, device=table.device, dtype=torch.float32)
    n = torch.empty(*ids.shape, D, device=table.device, dtype=torch.bfloat16)
    _timed("t5_embed_rms", 8.0 * M * D + 8.0 * M, lambda: _lib.call("vgpa_t5_rms", None, None, ids, table, V, w, x, n, 1, M, D, float(eps), _stream()), "byte")
    return x, n


def t5_gated_gelu(u):
    """u bf16 [..., 2 d_ff] (the output of one GEMM against wi_0 | wi_1) -> bf16 [..., d_ff] = gelu_new(u[..., :d_ff]) * u[..., d_ff:]"""
    _req(u, torch.bfloat16)
    _t5_forward_only("t5_gated_gelu", u)
    F2 = u.shape[-1]
    if F2 % 16 or u.numel() == 0:
        raise RuntimeError(f"t5_gated_gelu: the last dim holds both halves, d_ff a multiple of 8; got {tuple(u.shape)}")
    g = torch.empty(*u.shape[:-1], F2 // 2, device=u.device, dtype=torch.bfloat16)
    _timed("t5_gated_gelu", 3.0 * u.numel(), lambda: _lib.call("vgpa_t5_gated_gelu", u, g, u.numel() // F2, F2 // 2, _stream()), "byte")
    return g


# ---- SuperPoint around its convolutions (csrc/superpoint.hip): fp32, channels-last, forward only -------------------------------------------------
def conv1x1_relu_f32(x, w_packed, bias=None):
    """conv1x1_f32 of relu(x): for a producer that stored its output before the ReLU"""
    _heads_in(x, w_packed, bias)
    Cin, Cout = w_packed.shape
    if x.shape[-1] != Cin or Cin % 16 or Cout % 16:
        raise RuntimeError(f"conv1x1_relu_f32: weight {tuple(w_packed.shape)} does not fit input {tuple(x.shape)} (channels in multiples of 16)")
    out = torch.empty(*x.shape[:-1], Cout, device=x.device, dtype=torch.float32)
    M = out.numel() // Cout
    _timed("conv1x1_relu_f32", 2.0 * M * Cin * Cout, lambda: _lib.call("vgpa_conv1x1_relu_f32", x, w_packed, bias, out, M, Cin, Cout, _stream()))
    return out


def sp_gray_table(device=None):
    """g / 255.0 for the 256 bytes as the reference's `_frame2tensor` forms it: float64 division, then .float()"""
    t = (torch.arange(256, dtype=torch.float64) / 255.0).float()
    return t if device is None else t.to(device)


def sp_input_conv1a(src, w_packed, bias, size=None, table=None, return_gray=False):
    """uint8 RGB frames [T,H,W,3], or a float image [T,1,H,W] / [T,3,H,W] -> conv1a's pre-ReLU output [T,Ho,Wo,64] (gray conversion, g / 255 through
    `table`, bilinear resize to `size` = (Ho, Wo), the 1 -> 64 convolution); with return_gray also the resized gray image [T,Ho,Wo]"""
    _heads_in(w_packed, bias)
    _req(src)
    if src.dtype == torch.uint8:
        if src.dim() != 4 or src.shape[-1] != 3:
            raise RuntimeError(f"sp_input_conv1a: uint8 frames are [T,H,W,3], got {tuple(src.shape)}")
        mode, (T, H, W) = 0, src.shape[:3]
        table = sp_gray_table(src.device) if table is None else _req(table, torch.float32)
        if table.numel() != 256:
            raise RuntimeError("sp_input_conv1a: the gray table holds 256 values")
    elif src.dtype == torch.float32 and src.dim() == 4 and src.shape[1] in (1, 3):
        _heads_in(src)
        mode, T, (H, W), table = int(src.shape[1]), src.shape[0], src.shape[2:], None
    else:
        raise RuntimeError(f"sp_input_conv1a: expected uint8 [T,H,W,3] or fp32 [T,1|3,H,W], got {src.dtype} {tuple(src.shape)}")
    if tuple(w_packed.shape) != (3, 3, 1, 64) or bias.numel() != 64:
        raise RuntimeError(f"sp_input_conv1a: conv1a is [3,3,1,64] with 64 biases, got {tuple(w_packed.shape)}")
    Ho, Wo = (H, W) if size is None else size
    out = torch.empty(T, Ho, Wo, 64, device=src.device, dtype=torch.float32)
    gray = torch.empty(T, Ho, Wo, device=src.device, dtype=torch.float32) if return_gray else None
    _timed("sp_input_conv1a", float(src.numel() * src.element_size() + 4 * out.numel()),
           lambda: _lib.call("vgpa_sp_input_conv1a", src, mode, table, w_packed, bias, out, gray, T, H, W, Ho, Wo, _stream()), "byte")
    return (out, gray) if return_gray else out


def sp_head_f32(x, w, bias):
    """convPa's pre-ReLU map [T,h,w,256] -> the score image [T,8h,8w]: relu, 1x1 to 65 (w [256,65]), softmax, dustbin dropped, depth-to-space"""
    _heads_in(x, w, bias)
    if x.dim() != 4 or x.shape[-1] != 256 or tuple(w.shape) != (256, 65) or bias.numel() != 65:
        raise RuntimeError(f"sp_head_f32: expected x [T,h,w,256], w [256,65], bias [65], got {tuple(x.shape)}, {tuple(w.shape)}, {tuple(bias.shape)}")
    T, h, wd, _ = x.shape
    score = torch.empty(T, 8 * h, 8 * wd, device=x.device, dtype=torch.float32)
    _timed("sp_head_f32", 2.0 * T * h * wd * 256 * 65, lambda: _lib.call("vgpa_sp_head_f32", x, w, bias, score, T, h, wd, _stream()))
    return score


def sp_nms_f32(score, radius=4, border=0):
    """lightglue's simple_nms (three rounds, exact) of score [T,Hs,Ws], then the outer `border` rows and columns set to -1"""
    _heads_in(score)
    if score.dim() != 3 or not 1 <= int(radius) <= 4 or int(border) < 0:
        raise RuntimeError(f"sp_nms_f32: expected [T,Hs,Ws], radius 1..4 and border >= 0, got {tuple(score.shape)}, {radius}, {border}")
    T, Hs, Ws = score.shape
    out = torch.empty_like(score)
    _timed("sp_nms_f32", 8.0 * score.numel(), lambda: _lib.call("vgpa_sp_nms_f32", score, out, T, Hs, Ws, int(radius), int(border), _stream()), "byte")
    return out


SP_MAX_CUT = 4096   # a cut sorts its survivors in LDS


def sp_select(nms, threshold, max_num_keypoints=None):
    """pixels of nms [T,Hs,Ws] above `threshold`: (keypoints [T,K,2] as (x, y), scores [T,K], counts int32 [T]), rows past a frame's count unwritten.
    All of them in row-major order when they fit `max_num_keypoints`; else the top ones in descending score, ties in row-major order."""
    _heads_in(nms)
    T, Hs, Ws = nms.shape
    k = Hs * Ws if max_num_keypoints is None else min(int(max_num_keypoints), Hs * Ws)
    if k < 1 or (SP_MAX_CUT < k < Hs * Ws):
        raise RuntimeError(f"sp_select: max_num_keypoints is 1..{SP_MAX_CUT} or None, got {max_num_keypoints}")
    kp = torch.empty(T, k, 2, device=nms.device, dtype=torch.float32)
    sc = torch.empty(T, k, device=nms.device, dtype=torch.float32)
    counts = torch.empty(T, device=nms.device, dtype=torch.int32)
    ws_bytes = _lib.query("vgpa_sp_select_workspace_bytes", T, Hs, Ws)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=nms.device)
    _timed("sp_select", 12.0 * nms.numel(),
           lambda: _lib.call("vgpa_sp_select", nms, float(threshold), T, Hs, Ws, k, kp, sc, counts, ws, ws_bytes, _stream()), "byte")
    return kp, sc, counts


def sp_sample_desc_f32(dmap, kp, counts):
    """sample_descriptors (s = 8) of the raw descriptor map [T,h,w,256] at kp [T,K,2] -> [T,K,256], rows below counts[t] only"""
    _heads_in(dmap, kp)
    _req(counts, torch.int32)
    T, h, wd, C = dmap.shape
    if C != 256 or kp.dim() != 3 or kp.shape[0] != T or kp.shape[2] != 2 or counts.numel() != T:
        raise RuntimeError(f"sp_sample_desc_f32: expected dmap [T,h,w,256], kp [T,K,2], counts [T], got {tuple(dmap.shape)}, {tuple(kp.shape)}")
    K = kp.shape[1]
    out = torch.empty(T, K, 256, device=dmap.device, dtype=torch.float32)
    _timed("sp_sample_desc_f32", 4.0 * 5 * T * K * 256,
           lambda: _lib.call("vgpa_sp_sample_desc_f32", dmap, kp, counts, out, T, h, wd, K, _stream()), "byte")
    return out


# ---- LightGlue between its GEMMs (csrc/lightglue.hip): fp32, forward only, variable-length --------------------------------------------------------
LG_MAX_N = 4096   # rows per image


def _lg_f32(name, *ts, contiguous=True):
    for t in ts:
        if t is not None:
            _req(t, torch.float32, contiguous=contiguous)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError(f"{name} is forward only: call it under torch.no_grad()")


def _lg_seg(name, B, R, seg):
    """seg = (S0, c0, c1): rows [0, S0) of a sample are image 0 with counts c0 int32 [B], rows [S0, R) image 1 with counts c1 (None: one segment)"""
    S0, c0, c1 = seg
    for c in (c0, c1):
        if c is not None and (_req(c, torch.int32).numel() != B):
            raise RuntimeError(f"{name}: counts are int32 [B] = [{B}]")
    if not (0 < S0 <= R and (S0 < R if c1 is not None else S0 == R) and S0 <= LG_MAX_N and R - S0 <= LG_MAX_N):
        raise RuntimeError(f"{name}: segments S0 = {S0} of R = {R} rows (at most {LG_MAX_N} rows per image)")
    return int(S0), c0, c1


def lg_gemm(a, w, out=None, bias=None, accumulate=False, alpha=1.0, seg=None, ncount=None):
    """out[b, r, n] = alpha sum_k a[b, r, k] w[(b,) n, k] + bias[n] (accumulate: out += alpha sum, no bias) in exact fp32.  a [B,R,K] and out [B,R,N]
    are views with contiguous rows and one batch stride, w an nn.Linear weight [N,K] as it stands or a second activation view [B,N,K]; K a multiple of
    16.  Every element is one fixed sum over k wherever it sits, so a sample's rows come out bit-equal in any batch (a vendor GEMM may change its order
    with the row count).  seg = (S0, c0, c1): only rows below the counts are computed and written; ncount int32 [B]: only columns below it."""
    _lg_f32("lg_gemm", a, w, out, contiguous=False)
    _lg_f32("lg_gemm", bias)
    if a.dim() != 3 or w.dim() not in (2, 3) or a.stride(2) != 1 or w.stride(-1) != 1 or a.shape[2] != w.shape[-1] or (w.dim() == 3 and w.shape[0] != a.shape[0]):
        raise RuntimeError(f"lg_gemm: a [B,R,K] and w [N,K] | [B,N,K] with contiguous rows, got {tuple(a.shape)}, {tuple(w.shape)}")
    B, R, K = a.shape
    N = w.shape[-2]
    if out is None:
        if accumulate:
            raise RuntimeError("lg_gemm: accumulate needs out")
        out = torch.empty(B, R, N, device=a.device, dtype=torch.float32)
    if tuple(out.shape) != (B, R, N) or out.stride(2) != 1 or K % 16 or (bias is not None and (accumulate or bias.numel() != N)):
        raise RuntimeError(f"lg_gemm: out is a [B,R,N] = [{B},{R},{N}] view with contiguous rows, K a multiple of 16, bias [N] without accumulate")
    S0, c0, c1 = (0, None, None) if seg is None else _lg_seg("lg_gemm", B, R, seg)
    if ncount is not None and _req(ncount, torch.int32).numel() != B:
        raise RuntimeError("lg_gemm: ncount is int32 [B]")
    _timed("lg_gemm", 2.0 * B * R * N * K,
           lambda: _lib.call("vgpa_lg_gemm", a, a.stride(0), a.stride(1), w, w.stride(0) if w.dim() == 3 else 0, w.stride(-2), bias, out, out.stride(0),
                             out.stride(1), B, R, N, K, float(alpha), int(bool(accumulate)), S0, c0, c1, ncount, _stream()))
    return out


def lg_attention(dirs, q_premul=1.0):
    """softmax(q k^T / 8) v per head of 64 for one or two directions in one launch.  Each direction is a dict: q [B,Tq,H,64], k, v [B,Tk,H,64] fp32 VIEWS
    (last-dim stride 1, or 3 for the interleaved Wqkv output, the same in all of them), nq, nk int32 [B], rope_q / rope_k = (cos, sin) views
    [B,T,32] or None, out = an fp32 [B,Tq,H*64] view (last dim contiguous; created when absent).  The loader applies rotary and q_premul to q and k in fp32
    and rounds once to fp16.  -> the list of outs.  Rows at or past nq are not written; nk = 0 writes zeros."""
    if len(dirs) not in (1, 2):
        raise RuntimeError("lg_attention: one or two directions")
    B, _, H, _ = dirs[0]["q"].shape
    ds = dirs[0]["q"].stride(3)
    ptrs, strides, outs, keep = [], [], [], []
    for d in dirs:
        q, k, v = d["q"], d["k"], d["v"]
        _lg_f32("lg_attention", q, k, v, contiguous=False)
        if q.dim() != 4 or q.shape[3] != 64 or k.shape != v.shape or k.shape[0] != B or q.shape[0] != B or k.shape[2:] != q.shape[2:] or q.shape[2] != H:
            raise RuntimeError(f"lg_attention: q [B,Tq,H,64] and k, v [B,Tk,H,64], got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
        if ds not in (1, 3) or any(t.stride(3) != ds for t in (q, k, v)):
            raise RuntimeError("lg_attention: the last-dim stride of q, k and v is 1 or 3, the same in all")
        Tq, Tk = q.shape[1], k.shape[1]
        if not (1 <= Tq <= LG_MAX_N and 1 <= Tk <= LG_MAX_N):
            raise RuntimeError(f"lg_attention: 1 <= T <= {LG_MAX_N}, got {Tq}, {Tk}")
        nq, nk = _req(d["nq"], torch.int32), _req(d["nk"], torch.int32)
        if nq.numel() != B or nk.numel() != B:
            raise RuntimeError("lg_attention: nq and nk are int32 [B]")
        out = d.get("out")
        if out is None:
            out = torch.empty(B, Tq, H * 64, device=q.device, dtype=torch.float32)
        _lg_f32("lg_attention", out, contiguous=False)
        if tuple(out.shape) != (B, Tq, H * 64) or out.stride(2) != 1:
            raise RuntimeError(f"lg_attention: out is [B,Tq,{H * 64}] with a contiguous last dim, got {tuple(out.shape)}")
        rp, rs = [], []
        for key, T in (("rope_q", Tq), ("rope_k", Tk)):
            r = d.get(key)
            if r is None:
                rp += [None, None]
                rs.append(0)
                continue
            c, s = r
            _lg_f32("lg_attention", c, s, contiguous=False)
            if tuple(c.shape) != (B, T, 32) or c.shape != s.shape or c.stride()[1:] != (32, 1) or s.stride() != c.stride():
                raise RuntimeError(f"lg_attention: {key} is (cos, sin), each a [B,T,32] view with contiguous rows, got {tuple(c.shape)}")
            rp += [c.data_ptr(), s.data_ptr()]
            rs.append(c.stride(0))
        ptrs += [q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), nq.data_ptr(), nk.data_ptr()] + rp
        strides += [q.stride(0), q.stride(2), q.stride(1), k.stride(0), k.stride(2), k.stride(1), v.stride(0), v.stride(2), v.stride(1),
                    out.stride(0), out.stride(1), rs[0], rs[1], Tq, Tk, 0]
        outs.append(out)
        keep += [nq, nk]
    pa = (ctypes.c_void_p * len(ptrs))(*ptrs)
    sa = (ctypes.c_int64 * len(strides))(*strides)
    flops = sum(4.0 * B * H * d["q"].shape[1] * d["k"].shape[1] * 64 for d in dirs)
    _timed("lg_attn_fwd", flops, lambda: _lib.call("vgpa_lg_attn_fwd", pa, sa, B, H, len(dirs), ds, float(q_premul), _stream()))
    return outs


def lg_posenc(kpts, counts, Wr, image_size=None, out=None):
    """kpts [B,N,2], counts int32 [B], Wr [32,2], image_size [B,2] or None (then 1 + max - min of the sample's keypoints) -> (cos, sin), each [B,N,32]
    (`out` = a pair of [B,N,32] views with contiguous rows to write into)"""
    _lg_f32("lg_posenc", kpts, Wr, image_size)
    _req(counts, torch.int32)
    B, N = kpts.shape[:2]
    if kpts.dim() != 3 or kpts.shape[2] != 2 or tuple(Wr.shape) != (32, 2) or counts.numel() != B or not 1 <= N <= LG_MAX_N or \
            (image_size is not None and tuple(image_size.shape) != (B, 2)):
        raise RuntimeError(f"lg_posenc: kpts [B,N,2], counts [B], Wr [32,2], image_size [B,2] | None, got {tuple(kpts.shape)}, {tuple(Wr.shape)}")
    if out is None:
        out = (torch.empty(B, N, 32, device=kpts.device, dtype=torch.float32), torch.empty(B, N, 32, device=kpts.device, dtype=torch.float32))
    c, s = out
    _lg_f32("lg_posenc", c, s, contiguous=False)
    if tuple(c.shape) != (B, N, 32) or c.shape != s.shape or c.stride() != s.stride() or c.stride()[1:] != (32, 1):
        raise RuntimeError("lg_posenc: out is a pair of [B,N,32] views with contiguous rows and equal strides")
    _timed("lg_posenc", 8.0 * B * N * 32, lambda: _lib.call("vgpa_lg_posenc", kpts, counts, image_size, Wr, c, s, B, N, c.stride(0), _stream()), "byte")
    return c, s


def lg_ln_gelu(u, gamma, beta, seg, eps=1e-5, resid=None, resid_bias=None):
    """u [B,R,512] -> gelu_erf(LayerNorm(u)) [B,R,512] on the rows below the counts of seg = (S0, c0, c1).  resid ([B,R,256] view with contiguous
    rows, e.g. the left half of a [B,R,512] buffer) gets resid_bias [256] added in place: the bias of the GEMM that then accumulates into it."""
    _lg_f32("lg_ln_gelu", u, gamma, beta, resid_bias)
    B, R = u.shape[:2]
    if u.dim() != 3 or u.shape[2] != 512 or gamma.numel() != 512 or beta.numel() != 512:
        raise RuntimeError(f"lg_ln_gelu: u [B,R,512] with 512 weights and biases, got {tuple(u.shape)}")
    S0, c0, c1 = _lg_seg("lg_ln_gelu", B, R, seg)
    rs = 0
    if resid is not None:
        _lg_f32("lg_ln_gelu", resid, contiguous=False)
        if tuple(resid.shape) != (B, R, 256) or resid.stride(2) != 1 or resid.stride(0) != R * resid.stride(1) or resid_bias is None or resid_bias.numel() != 256:
            raise RuntimeError("lg_ln_gelu: resid is a [B,R,256] view with one row stride and resid_bias holds 256 values")
        rs = resid.stride(1)
    h = torch.empty_like(u)
    _timed("lg_ln_gelu", 4096.0 * B * R, lambda: _lib.call("vgpa_lg_ln_gelu", u, gamma, beta, float(eps), h, resid, rs, resid_bias, B, R, S0, c0, c1, _stream()),
           "byte")
    return h


def lg_confidence(x, w, bias, seg, thr=None, below=None, want_conf=True, want_z=False):
    """x [B,R,256] view with one row stride; z = w . x + bias, conf = sigmoid(z) -> (conf [B,R] | None, z [B,R] | None).  With thr (a Python float,
    compared in double) and below int32 [B] (zeroed by the caller): below[b] += the number of the sample's rows with conf < thr."""
    _lg_f32("lg_confidence", x, contiguous=False)
    _lg_f32("lg_confidence", w)
    B, R = x.shape[:2]
    if x.dim() != 3 or x.shape[2] != 256 or x.stride(2) != 1 or x.stride(0) != R * x.stride(1) or w.numel() != 256 or not (want_conf or want_z):
        raise RuntimeError(f"lg_confidence: x is a [B,R,256] view with one row stride, w holds 256 values, got {tuple(x.shape)}")
    S0, c0, c1 = _lg_seg("lg_confidence", B, R, seg)
    if (thr is None) != (below is None) or (below is not None and _req(below, torch.int32).numel() != B):
        raise RuntimeError("lg_confidence: thr and below (int32 [B]) come together")
    conf = torch.zeros(B, R, device=x.device, dtype=torch.float32) if want_conf else None
    z = torch.zeros(B, R, device=x.device, dtype=torch.float32) if want_z else None
    _timed("lg_confidence", 1024.0 * B * R, lambda: _lib.call("vgpa_lg_confidence", x, x.stride(1), w, float(bias), conf, z, 0.0 if thr is None else float(thr),
                                                                below, B, R, S0, c0, c1, _stream()), "byte")
    return conf, z


def lg_prune(conf, match, thr_conf, thr_keep, prune_min, x_in, x_out, rope_in, rope_out, ind_in, ind_out, prune, seg, counts_out, want_keep=False):
    """Point pruning of every segment with more than prune_min rows: keep row i iff match[i] > thr_keep or conf[i] <= thr_conf (Python floats, compared
    in double); other segments keep everything.  conf, match [B,R]; x_in / x_out [B,R,256] views of two different buffers with the same row stride;
    rope_* = (cos, sin) [B,R,32]; ind_* int32 [B,R]; prune = (prune0 [B,P0], prune1 [B,P1] | None) int32, += 1 at the kept rows' ind;
    counts_out = (c0_out, c1_out | None).  Ordered and stable.  -> the keep mask uint8 [B,R] by input row when want_keep."""
    _lg_f32("lg_prune", conf, match, *rope_in, *rope_out)
    _lg_f32("lg_prune", x_in, x_out, contiguous=False)
    B, R = conf.shape
    S0, c0, c1 = _lg_seg("lg_prune", B, R, seg)
    for t in (x_in, x_out):
        if tuple(t.shape) != (B, R, 256) or t.stride(2) != 1 or t.stride(0) != R * t.stride(1) or t.stride(1) != x_in.stride(1):
            raise RuntimeError("lg_prune: x_in and x_out are [B,R,256] views with one and the same row stride")
    if match.shape != conf.shape or any(tuple(t.shape) != (B, R, 32) for t in (*rope_in, *rope_out)) or any(_req(t, torch.int32).shape != conf.shape for t in (ind_in, ind_out)):
        raise RuntimeError("lg_prune: conf, match, ind [B,R]; rotary tables [B,R,32]")
    p0, p1 = prune
    o0, o1 = counts_out
    for t in (p0, p1, o0, o1):
        if t is not None:
            _req(t, torch.int32)
    if (c1 is None) != (p1 is None) or (c1 is None) != (o1 is None) or p0.shape[0] != B or o0.numel() != B:
        raise RuntimeError("lg_prune: prune and counts_out follow the segments")
    keep = torch.zeros(B, R, device=conf.device, dtype=torch.uint8) if want_keep else None
    _timed("lg_prune", 2.0 * 1280 * B * R,
           lambda: _lib.call("vgpa_lg_prune", conf, match, float(thr_conf), float(thr_keep), int(prune_min), x_in, x_out, x_in.stride(1), rope_in[0], rope_in[1],
                             rope_out[0], rope_out[1], ind_in, ind_out, p0, p1, p0.shape[1], 0 if p1 is None else p1.shape[1], B, R, S0, c0, c1, o0, o1, keep,
                             _stream()), "byte")
    return keep


def lg_assign_workspace(B, Mmax, Nmax, device):
    """the workspace of lg_assign as fp32 words, and its views: rmax, rlog, rbest, rarg [B,Mmax], cmax, clog, cbest, carg [B,Nmax] (the args as int32)"""
    ws = torch.zeros(_lib.query("vgpa_lg_assign_workspace_bytes", B, Mmax, Nmax) // 4, device=device, dtype=torch.float32)
    nr, nc = B * Mmax, B * Nmax
    r = [ws[i * nr:(i + 1) * nr].view(B, Mmax) for i in range(4)]
    c = [ws[4 * nr + i * nc:4 * nr + (i + 1) * nc].view(B, Nmax) for i in range(4)]
    views = {"rmax": r[0], "rlog": r[1], "rbest": r[2], "rarg": r[3].view(torch.int32), "cmax": c[0], "clog": c[1], "cbest": c[2], "carg": c[3].view(torch.int32)}
    return ws, views


def lg_assign(sim, z0, z1, m, n, thr, ind0=None, ind1=None, M0=None, N0=None, want_scores=False, stages=7, workspace=None):
    """LightGlue's assignment and filter_matches from sim [B,Mmax,Nmax], the matchability logits z0 [B,Mmax], z1 [B,Nmax] and the counts m, n int32 [B];
    thr a Python float compared in double.  stages: 1 log-sum-exps, 2 argmax of the log score (ties to the lowest index), 4 matches; a later stage
    alone reads what `workspace` (lg_assign_workspace) holds.  ind0 / ind1 int32 [B,Mmax] / [B,Nmax] map rows to the original indices of a side with
    M0 / N0 points.  -> dict(matches0 [B,M0], matches1 [B,N0] int32, matching_scores0, matching_scores1, matches [B,M0,2] int32, scores [B,M0],
    count int32 [B], log_assignment [B,Mmax+1,Nmax+1] | None, workspace)"""
    _lg_f32("lg_assign", sim, z0, z1)
    B, Mmax, Nmax = sim.shape
    if tuple(z0.shape) != (B, Mmax) or tuple(z1.shape) != (B, Nmax) or _req(m, torch.int32).numel() != B or _req(n, torch.int32).numel() != B or \
            not (1 <= Mmax <= LG_MAX_N and 1 <= Nmax <= LG_MAX_N) or (ind0 is None) != (ind1 is None):
        raise RuntimeError(f"lg_assign: sim [B,M,N], z0 [B,M], z1 [B,N], counts [B], got {tuple(sim.shape)}, {tuple(z0.shape)}, {tuple(z1.shape)}")
    M0, N0 = Mmax if M0 is None else int(M0), Nmax if N0 is None else int(N0)
    if ind0 is not None and (tuple(_req(ind0, torch.int32).shape) != (B, Mmax) or tuple(_req(ind1, torch.int32).shape) != (B, Nmax)):
        raise RuntimeError("lg_assign: ind0 [B,Mmax] and ind1 [B,Nmax] int32")
    if M0 < Mmax or N0 < Nmax:
        raise RuntimeError("lg_assign: M0 >= Mmax and N0 >= Nmax")
    dev = sim.device
    ws = lg_assign_workspace(B, Mmax, Nmax, dev)[0] if workspace is None else _req(workspace, torch.float32)
    i32 = dict(device=dev, dtype=torch.int32)
    out = {"matches0": torch.full((B, M0), -1, **i32), "matches1": torch.full((B, N0), -1, **i32),
           "matching_scores0": torch.zeros(B, M0, device=dev), "matching_scores1": torch.zeros(B, N0, device=dev),
           "matches": torch.zeros(B, M0, 2, **i32), "scores": torch.zeros(B, M0, device=dev), "count": torch.zeros(B, **i32),
           "log_assignment": torch.zeros(B, Mmax + 1, Nmax + 1, device=dev) if want_scores else None, "workspace": ws}
    _timed("lg_assign", 16.0 * sim.numel(),
           lambda: _lib.call("vgpa_lg_assign", sim, z0, z1, m, n, B, Mmax, Nmax, float(thr), ind0, ind1, M0, N0, out["matches0"], out["matches1"],
                             out["matching_scores0"], out["matching_scores1"], out["matches"], out["scores"], out["count"], out["log_assignment"], int(stages),
                             ws, ws.numel() * 4, _stream()), "byte")
    return out
