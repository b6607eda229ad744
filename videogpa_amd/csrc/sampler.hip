// One sampler step of the generate loop in one pass: classifier-free guidance, the v-prediction data estimate, the scheduler's update and the
// next transformer input (generate/CogVideoX-5B-I2V.py:70-89 -> diffusers CogVideoXImageToVideoPipeline.__call__, the body of its denoising loop
// behind the transformer: `.float()`, chunk(2), the guidance combine, scheduler.step, the cast back, and the next iteration's two torch.cat).
// Both CogVideoX samplers are linear in their operands, so the host folds them into scalars (videogpa_amd/scheduler.py step_coefficients):
//   v      = v_u + g * (v_c - v_u)                                 (guided: v is [2B, N] = [uncond | cond]; else v = the model output)
//   x0     = sa * x - sb * v                                       (v-prediction)
//   x_next = k_x * x + k_0 * x0 + k_old * x0_old + k_n * noise     (a term whose pointer is NULL is left out)
// DDIM (eta = 0): k_x = sqrt((1 - a_prev) / (1 - a_t)), k_0 = sqrt(a_prev) - sqrt(a_t) k_x.  DPM-Solver++ 2M (SDE): k_x = m1, k_0 = -m2 (1 + 1/2r),
// k_old = m2 / 2r, k_n = m_noise of CogVideoXDPMScheduler.step.
// fp32 arithmetic, every product and sum rounded on its own (no FMA contraction), one rounding to the latent dtype at the store.
// The packed output is the next transformer input [G * B, F, C + C_img, h, w]: per (guidance half, b, f), C h w elements of x_next and then C_img h w
// elements of the image latents, so the loop never concatenates.  Reads v (G N), x (N), [x0_old 4N, noise N, image N_img]; writes x_next, x0 (fp32),
// packed G (N + N_img): HBM streaming, 8 elements per lane and access.
#include "common.h"

#pragma clang fp contract(off)

struct SamplerArgs {
    const void* v; const void* x; const float* x0_old; const void* noise; const void* image;
    void* x_next; float* x0; void* packed;
    int64_t B, F, lat_per_frame /* C h w */, img_per_frame /* C_img h w */;
    int guided, groups;
    float g, sa, sb, k_x, k_0, k_old, k_n;
};

template <int VDT, int XDT>
__global__ __launch_bounds__(256) void sampler_step_kernel(SamplerArgs a) {
    const int64_t b = blockIdx.y;
    const int64_t N = a.F * a.lat_per_frame, Ni = a.image ? a.F * a.img_per_frame : 0;
    const int64_t n8 = N >> 3, total8 = n8 + (Ni >> 3);
    const int64_t packed_frame = a.lat_per_frame + a.img_per_frame;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < total8; c += (int64_t)gridDim.x * 256) {
        float o[8];
        int64_t dst;                                    // offset inside one sample of the packed layout
        if (c < n8) {
            const int64_t i = c << 3;
            const size_t at = (size_t)(b * N + i);
            float xv[8], vv[8], x0v[8];
            load8<XDT>(a.x, at, xv);
            if (a.guided) {
                float vu[8], vc[8];
                load8<VDT>(a.v, at, vu);
                load8<VDT>(a.v, (size_t)((a.B + b) * N + i), vc);
#pragma unroll
                for (int j = 0; j < 8; ++j) vv[j] = vu[j] + a.g * (vc[j] - vu[j]);
            } else {
                load8<VDT>(a.v, at, vv);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                x0v[j] = a.sa * xv[j] - a.sb * vv[j];
                o[j] = a.k_x * xv[j] + a.k_0 * x0v[j];
            }
            if (a.x0_old) {
                float old[8];
                load8<VGPA_DTYPE_F32>(a.x0_old, at, old);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = o[j] + a.k_old * old[j];
            }
            if (a.noise) {
                float e[8];
                load8<XDT>(a.noise, at, e);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = o[j] + a.k_n * e[j];
            }
            if (a.x0) store8<VGPA_DTYPE_F32>(a.x0, at, x0v);
            store8<XDT>(a.x_next, at, o);
            const int64_t f = i / a.lat_per_frame;
            dst = f * packed_frame + (i - f * a.lat_per_frame);
        } else {
            const int64_t i = (c - n8) << 3;
            load8<XDT>(a.image, (size_t)(b * Ni + i), o);
            const int64_t f = i / a.img_per_frame;
            dst = f * packed_frame + a.lat_per_frame + (i - f * a.img_per_frame);
        }
        if (a.packed) {
            for (int gi = 0; gi < a.groups; ++gi) store8<XDT>(a.packed, (size_t)((gi * a.B + b) * a.F * packed_frame + dst), o);
        }
    }
}

extern "C" int32_t vgpa_sampler_step(const void* v, int32_t v_dtype, int32_t guided, const void* x, const float* x0_old, const void* noise,
                                     const void* image_latents, int64_t B, int64_t F, int64_t C, int64_t C_img, int64_t hw, int32_t dtype, float g,
                                     float sa, float sb, float k_x, float k_0, float k_old, float k_n, void* x_next, float* x0, void* packed,
                                     int32_t packed_groups, hipStream_t stream) {
    if (!v || !x || !x_next || B <= 0 || B > 65535 || F <= 0 || C <= 0 || hw <= 0) return VGPA_ERR_INVALID;
    if ((C * hw) % 8 != 0) return VGPA_ERR_INVALID;
    if ((image_latents != nullptr) != (packed != nullptr)) return VGPA_ERR_INVALID;      // the image latents only travel into the packed input
    if (packed && (C_img <= 0 || (C_img * hw) % 8 != 0 || (packed_groups != 1 && packed_groups != 2))) return VGPA_ERR_INVALID;
    SamplerArgs a;
    a.v = v; a.x = x; a.x0_old = x0_old; a.noise = noise; a.image = image_latents;
    a.x_next = x_next; a.x0 = x0; a.packed = packed;
    a.B = B; a.F = F; a.lat_per_frame = C * hw; a.img_per_frame = packed ? C_img * hw : 0;
    a.guided = guided ? 1 : 0; a.groups = packed_groups;
    a.g = g; a.sa = sa; a.sb = sb; a.k_x = k_x; a.k_0 = k_0; a.k_old = k_old; a.k_n = k_n;
    const int64_t total8 = F * (a.lat_per_frame + a.img_per_frame) / 8;
    int64_t nb = (total8 + 255) / 256;
    if (nb > 2048) nb = 2048;
    dim3 grid((unsigned)nb, (unsigned)B);
#define SS(VDT, XDT) VGPA_LAUNCH((sampler_step_kernel<VDT, XDT>), grid, dim3(256), 0, stream, a)
    if (v_dtype == VGPA_DTYPE_BF16 && dtype == VGPA_DTYPE_BF16) SS(VGPA_DTYPE_BF16, VGPA_DTYPE_BF16);
    else if (v_dtype == VGPA_DTYPE_F32 && dtype == VGPA_DTYPE_BF16) SS(VGPA_DTYPE_F32, VGPA_DTYPE_BF16);
    else if (v_dtype == VGPA_DTYPE_BF16 && dtype == VGPA_DTYPE_F32) SS(VGPA_DTYPE_BF16, VGPA_DTYPE_F32);
    else if (v_dtype == VGPA_DTYPE_F32 && dtype == VGPA_DTYPE_F32) SS(VGPA_DTYPE_F32, VGPA_DTYPE_F32);
    else return VGPA_ERR_INVALID;
#undef SS
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}
