"""TEST INFRASTRUCTURE -- fp64 restatements for the image-to-video path, independent of videogpa_amd/scheduler.py and csrc/sampler.hip.

DDIM (eta = 0) in the textbook form of Song et al. 2021 eq. 12 on a v-prediction model (Salimans & Ho 2022):
    x0 = sqrt(a_t) x - sqrt(1 - a_t) v,    eps = sqrt(a_t) v + sqrt(1 - a_t) x,    x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps
which is not the (a_t, b_t) form the scheduler class is written in (that one eliminates eps through a division by sqrt(1 - a_t)).

The fused sampler step (ops.sampler_step):  v = v_u + g (v_c - v_u),  x0 = sa x - sb v,  x_next = k_x x + k_0 x0 + k_old old + k_n noise, from the scalars AS THE
C ENTRY RECEIVES THEM (floats: the reference rounds each to fp32 first, that is the interface) and the stored inputs.  Bound per element: every fp32 operation
is off by at most 2^-24 of its result, and every intermediate result is at most the sum of the magnitudes of the leaf terms behind it, so
    |err| <= 2^-23 n_ops S,    S = |k_x x| + |k_0| (|sa x| + |sb| V) + |k_old old| + |k_n noise|,    V = |v_u| + |g| (|v_c| + |v_u|)  (|v| without guidance)
with n_ops the number of fp32 operations on the longest path (3 guidance + 3 data estimate + 3 + 2 + 2 update = 13, fewer when a term is absent); 2^-23
instead of 2^-24 leaves the factor 2 for second-order terms.  A bf16 store adds half a bf16 ulp (tests/row_tol.py half_ulp_bf16)."""
import math

import numpy as np
import torch


def ddim_textbook_step(abar, v, t, x, num_inference_steps, num_train_timesteps=1000, final_alpha=1.0):
    """-> (x_prev, x0) fp64"""
    t = int(t)
    tp = t - num_train_timesteps // num_inference_steps
    a_t = float(abar[t])
    a_p = float(abar[tp]) if tp >= 0 else final_alpha
    x, v = x.double(), v.double()
    x0 = math.sqrt(a_t) * x - math.sqrt(1 - a_t) * v
    eps = math.sqrt(a_t) * v + math.sqrt(1 - a_t) * x
    return math.sqrt(a_p) * x0 + math.sqrt(1 - a_p) * eps, x0


def _f32(c):
    return None if c is None else float(np.float32(c))


def sampler_step_ref(v, x, coef, g=None, x0_old=None, noise=None):
    """-> (x_next, x0, bound of x_next, bound of x0) fp64 on the inputs' device; v [G B, ...] with G = 2 when g is given"""
    sa, sb, kx, k0, ko, kn = (_f32(coef[k]) for k in ("sa", "sb", "k_x", "k_0", "k_old", "k_n"))
    x, v = x.double(), v.double()
    ops0 = 3
    if g is not None:
        g = _f32(g)
        v_u, v_c = v.chunk(2)
        v = v_u + g * (v_c - v_u)
        V = v_u.abs() + abs(g) * (v_c.abs() + v_u.abs())
        ops0 += 3
    else:
        V = v.abs()
    x0 = sa * x - sb * v
    S0 = (sa * x).abs() + abs(sb) * V
    nxt, S, n_ops = kx * x + k0 * x0, (kx * x).abs() + abs(k0) * S0, ops0 + 3
    if ko is not None:
        nxt, S, n_ops = nxt + ko * x0_old.double(), S + (ko * x0_old.double()).abs(), n_ops + 2
    if kn is not None:
        nxt, S, n_ops = nxt + kn * noise.double(), S + (kn * noise.double()).abs(), n_ops + 2
    return nxt, x0, 2.0 ** -23 * n_ops * S, 2.0 ** -23 * ops0 * S0


def packed_ref(x_next, image_latents, G):
    """the next transformer input as the pipeline forms it"""
    return torch.cat([torch.cat([x_next] * G), torch.cat([image_latents] * G)], dim=2)


def i2v_loop_ref(forward, abar, timesteps, latents, image_latents, guidance_scale, round_to=torch.bfloat16):
    """the pipeline's I2V denoising loop in fp64 on the CPU with DDIM: forward(inp [2B,F,C+C_img,h,w] fp64, t) -> v fp64; the latents are rounded to
    `round_to` after every step as the pipeline casts them back to the prompt dtype"""
    lat, img = latents.double(), image_latents.double()
    n = len(timesteps)
    for t in timesteps:
        inp = torch.cat([torch.cat([lat, lat]), torch.cat([img, img])], dim=2)
        v = forward(inp, t)
        v = v[: lat.shape[0]] + guidance_scale * (v[lat.shape[0]:] - v[: lat.shape[0]])
        lat, _ = ddim_textbook_step(abar, v, t, lat, n)
        lat = lat.to(round_to).double()
    return lat
