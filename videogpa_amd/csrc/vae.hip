// CogVideoX VAE encoder on one frame (diffusers' autoencoder_kl_cogvideox.py), the part around its convolutions, which run on conv_kernel through the
// entry points of vae_conv.hip (the 3-D causal kernels fold into 2-D ones at load time: videogpa_amd/vae.py; on a clip they are its CV_CONV3D and CV_POOL_DOWN modes, and
// the kernels below see the clip's frames as part of the pixel extent HW).  Everything fp32, channels-last (NHWC), forward only:
//   vae_input_kernel     layout change in front of conv_in: [N,3,H,W] fp32 | bf16 -> [N,H,W,16] fp32, channels 3..15 = 0, so that the stem is a 16-channel
//                        convolution with zero weight rows
//   gn_partial_kernel    GroupNorm statistics, stage 1: a workgroup owns a run of pixels of one sample and leaves (mean, M2) of every CHANNEL over them.
//                        A thread walks its pixels with Welford's update, the threads of a channel column merge with Chan's formula, all in fp64:
//                        no sum of squares is ever formed, so a map at mean 100 and variance 1 loses nothing
//   gn_combine_kernel    stage 2: one workgroup per (sample, group) merges the partials of the group's channels in a fixed order (Chan again, fp64) and
//                        writes (mean, rstd) as fp32.  No atomics: bit-identical from run to run, and a sample's statistics do not depend on N
//   gn_silu_kernel       y = silu((x - mean) * rstd * gamma + beta), one pass of float4 accesses, grid-stride
//   vae_sample_kernel    DiagonalGaussianDistribution: moments [N,h,w,2L] -> mean, logvar.clamp(-30, 20), std = exp(logvar / 2), sample = (mean + std * noise)
//                        * scale as [N,L,1,h,w] in the output dtype; every output is optional
// and of the decoder (the same convolutions plus conv_kernel's CV_UP2X up-sampler):
//   spatial_norm_silu_kernel  CogVideoXSpatialNorm3D + SiLU: silu(GroupNorm(f) * Y + B), (Y | B) gathered from the latent-resolution map of conv_y | conv_b
//   vae_output_kernel    behind conv_out (3 channels padded to 16): [N,T,H,W,16] fp32 -> [N,3,T,H,W] fp32 | bf16, or the uint8 frames [N,T,H,W,3]
// The statistics and the apply pass are HBM-bound by design: algorithmic bytes N HW C 4 for the statistics, 2 N HW C 4 for the apply.
#include "common.h"

#define VAE_THREADS 256
#define GN_ITERS 64                      // pixels a thread walks in stage 1: a workgroup owns (256 / (C / 4)) * GN_ITERS consecutive pixels of one sample
#define VAE_OUT_U8 2                     // vgpa_vae_output's third out_dtype: the uint8 frames
#define GN_LOADS 4                     // of them loaded ahead of their updates (the Welford chain is serial; its loads need not be)

template <int DT>
__global__ __launch_bounds__(VAE_THREADS) void vae_input_kernel(const void* __restrict__ x, float* __restrict__ out, int64_t HW, int64_t total4) {
    // thread = one 16-byte quarter of an output pixel: quarter 0 carries the three channels, quarters 1..3 are zero
    for (int64_t i = (int64_t)blockIdx.x * VAE_THREADS + threadIdx.x; i < total4; i += (int64_t)gridDim.x * VAE_THREADS) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((i & 3) == 0) {
            const int64_t p = i >> 2, n = p / HW, r = p - n * HW;
            const size_t src = (size_t)n * 3 * HW + r;
            v = make_float4(load1<DT>(x, src), load1<DT>(x, src + HW), load1<DT>(x, src + 2 * HW), 0.f);
        }
        reinterpret_cast<float4*>(out)[i] = v;
    }
}

// (na, ma, Ma) <- the union of (na, ma, Ma) and (nb, mb, Mb): Chan, Golub and LeVeque's pairwise update; an empty side changes nothing
__device__ __forceinline__ void chan_merge(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
    if (nb == 0.0) return;
    if (na == 0.0) {
        na = nb; ma = mb; Ma = Mb;
        return;
    }
    const double n = na + nb, d = mb - ma;
    ma += d * (nb / n);
    Ma += Mb + d * d * (na * nb / n);
    na = n;
}

// how stage 1 cuts a sample: ncol float4 columns, rpp pixel rows per pass of the workgroup, ppc pixels per workgroup
struct GnTiling {
    int ncol, rpp;
    int64_t ppc, chunks;
};
static GnTiling gn_tiling(int64_t HW, int64_t C) {
    GnTiling t;
    t.ncol = (int)(C / 4);
    t.rpp = VAE_THREADS / t.ncol;
    t.ppc = (int64_t)t.rpp * GN_ITERS;
    t.chunks = (HW + t.ppc - 1) / t.ppc;
    return t;
}

// grid (chunks, N); part [N][chunks][C][2] = (mean, M2) of channel c over the chunk's pixels, whose number follows from the chunk index
__global__ __launch_bounds__(VAE_THREADS) void gn_partial_kernel(const float* __restrict__ x, double* __restrict__ part, int64_t HW, int C, int ncol, int rpp,
                                                                  int64_t ppc) {
    __shared__ double s_mean[VAE_THREADS][4], s_m2[VAE_THREADS][4];
    __shared__ int s_cnt[VAE_THREADS];
    const int tid = threadIdx.x, col = tid % ncol, row = tid / ncol;
    const int64_t n = blockIdx.y, p0 = (int64_t)blockIdx.x * ppc, p1 = p0 + ppc < HW ? p0 + ppc : HW;
    double mean[4] = {0.0, 0.0, 0.0, 0.0}, m2[4] = {0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
    if (row < rpp) {                                                            // 256 % ncol threads idle when ncol does not divide 256
        const float* src = x + ((size_t)n * HW) * C + 4 * col;
        for (int64_t p = p0 + row; p < p1; p += (int64_t)GN_LOADS * rpp) {          // GN_LOADS loads in flight, then the updates in pixel order
            float4 v[GN_LOADS];
#pragma unroll
            for (int u = 0; u < GN_LOADS; ++u) {
                const int64_t q = p + (int64_t)u * rpp;
                v[u] = q < p1 ? *reinterpret_cast<const float4*>(src + (size_t)q * C) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < GN_LOADS; ++u) {
                if (p + (int64_t)u * rpp >= p1) break;
                const double f[4] = {(double)v[u].x, (double)v[u].y, (double)v[u].z, (double)v[u].w};
                cnt += 1;
                const double inv = 1.0 / (double)cnt;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d = f[j] - mean[j];
                    mean[j] += d * inv;
                    m2[j] += d * (f[j] - mean[j]);
                }
            }
        }
    }
    s_cnt[tid] = cnt;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s_mean[tid][j] = mean[j];
        s_m2[tid][j] = m2[j];
    }
    __syncthreads();
    if (row == 0) {                                                             // the column's rows, in order
        double* dst = part + (((size_t)n * gridDim.x + blockIdx.x) * C + 4 * col) * 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double na = (double)cnt, ma = mean[j], Ma = m2[j];
            for (int r = 1; r < rpp; ++r) chan_merge(na, ma, Ma, (double)s_cnt[r * ncol + col], s_mean[r * ncol + col][j], s_m2[r * ncol + col][j]);
            dst[2 * j] = ma;
            dst[2 * j + 1] = Ma;
        }
    }
}

// grid (G, N); stats [N][G][2] = (mean, rstd)
__global__ __launch_bounds__(VAE_THREADS) void gn_combine_kernel(const double* __restrict__ part, float* __restrict__ stats, int64_t HW, int C, int cpg,
                                                                  int64_t ppc, int64_t chunks, float eps) {
    __shared__ double s_n[VAE_THREADS], s_mean[VAE_THREADS], s_m2[VAE_THREADS];
    const int tid = threadIdx.x, g = blockIdx.x;
    const int64_t n = blockIdx.y, items = chunks * cpg;
    double na = 0.0, ma = 0.0, Ma = 0.0;
    for (int64_t i = tid; i < items; i += VAE_THREADS) {
        const int64_t chunk = i / cpg;
        const int c = g * cpg + (int)(i - chunk * cpg);
        const int64_t left = HW - chunk * ppc;
        const double* src = part + (((size_t)n * chunks + chunk) * C + c) * 2;
        chan_merge(na, ma, Ma, (double)(left < ppc ? left : ppc), src[0], src[1]);
    }
    s_n[tid] = na; s_mean[tid] = ma; s_m2[tid] = Ma;
    __syncthreads();
    for (int s = VAE_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            chan_merge(s_n[tid], s_mean[tid], s_m2[tid], s_n[tid + s], s_mean[tid + s], s_m2[tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        float* dst = stats + ((size_t)n * gridDim.x + g) * 2;
        dst[0] = (float)s_mean[0];
        dst[1] = (float)(1.0 / sqrt(s_m2[0] / s_n[0] + (double)eps));
    }
}

__device__ __forceinline__ float gn_silu1(float x, float mean, float rstd, float gamma, float beta) {
    const float y = (x - mean) * rstd * gamma + beta;
    return y / (1.0f + expf(-y));
}

__global__ __launch_bounds__(VAE_THREADS) void gn_silu_kernel(const float* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* __restrict__ out, int64_t HW, int C, int G, int cpg,
                                                               int64_t total4) {
    const int ncol = C >> 2;
    for (int64_t i = (int64_t)blockIdx.x * VAE_THREADS + threadIdx.x; i < total4; i += (int64_t)gridDim.x * VAE_THREADS) {
        const int c = (int)(i % ncol) * 4;
        const int64_t n = i / (HW * ncol);
        const float* st = stats + (size_t)n * G * 2;
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        const float4 gm = *reinterpret_cast<const float4*>(gamma + c), bt = *reinterpret_cast<const float4*>(beta + c);
        const int g0 = c / cpg, g1 = (c + 1) / cpg, g2 = (c + 2) / cpg, g3 = (c + 3) / cpg;
        float4 y;
        y.x = gn_silu1(v.x, st[2 * g0], st[2 * g0 + 1], gm.x, bt.x);
        y.y = gn_silu1(v.y, st[2 * g1], st[2 * g1 + 1], gm.y, bt.y);
        y.z = gn_silu1(v.z, st[2 * g2], st[2 * g2 + 1], gm.z, bt.z);
        y.w = gn_silu1(v.w, st[2 * g3], st[2 * g3 + 1], gm.w, bt.w);
        reinterpret_cast<float4*>(out)[i] = y;
    }
}

// CogVideoXSpatialNorm3D + SiLU of the decoder: the GroupNorm value times Y plus B, where (Y | B) [N,t,h,w,2C] is conv_y | conv_b of the latent at
// the latent's own resolution and the nearest-neighbour resize is the gather below (a 1x1 convolution commutes with it exactly).  H = ry h, W = rx w;
// in time floor(dst * t / T), except that an odd T > 1 maps frame 0 to frame 0 and frames 1.. onto latent frames 1.. on their own
__global__ __launch_bounds__(VAE_THREADS) void spatial_norm_silu_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                         const float* __restrict__ yb, float* __restrict__ out, int T, int H, int W, int C,
                                                                         int G, int cpg, int t, int h, int w, int ry, int rx, int64_t total4) {
    const int ncol = C >> 2;
    const bool split = T > 1 && (T & 1);
    for (int64_t i = (int64_t)blockIdx.x * VAE_THREADS + threadIdx.x; i < total4; i += (int64_t)gridDim.x * VAE_THREADS) {
        const int c = (int)(i % ncol) * 4;
        int64_t p = i / ncol;
        const int px = (int)(p % W);
        p /= W;
        const int py = (int)(p % H);
        p /= H;
        const int pt = (int)(p % T);
        const int64_t n = p / T;
        const int tz = split ? (pt == 0 ? 0 : 1 + ((pt - 1) * (t - 1)) / (T - 1)) : (int)(((int64_t)pt * t) / T);
        const float* m = yb + ((((size_t)n * t + tz) * h + py / ry) * w + px / rx) * (size_t)(2 * C) + c;
        const float4 Y = *reinterpret_cast<const float4*>(m), B = *reinterpret_cast<const float4*>(m + C);
        const float* st = stats + (size_t)n * G * 2;
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        const float4 gm = *reinterpret_cast<const float4*>(gamma + c), bt = *reinterpret_cast<const float4*>(beta + c);
        const int g0 = c / cpg, g1 = (c + 1) / cpg, g2 = (c + 2) / cpg, g3 = (c + 3) / cpg;
        float4 y;
        y.x = ((v.x - st[2 * g0]) * st[2 * g0 + 1] * gm.x + bt.x) * Y.x + B.x;
        y.y = ((v.y - st[2 * g1]) * st[2 * g1 + 1] * gm.y + bt.y) * Y.y + B.y;
        y.z = ((v.z - st[2 * g2]) * st[2 * g2 + 1] * gm.z + bt.z) * Y.z + B.z;
        y.w = ((v.w - st[2 * g3]) * st[2 * g3 + 1] * gm.w + bt.w) * Y.w + B.w;
        reinterpret_cast<float4*>(out)[i] = make_float4(y.x / (1.0f + expf(-y.x)), y.y / (1.0f + expf(-y.y)), y.z / (1.0f + expf(-y.z)),
                                                        y.w / (1.0f + expf(-y.w)));
    }
}

// behind conv_out, whose 3 channels are padded to 16: thread = one pixel of x [N,THW,16].  DT fp32 | bf16: out [N,3,THW] (the inverse of
// vae_input_kernel); U8: out [N,THW,3] bytes = round(clamp(x / 2 + 0.5, 0, 1) * 255), ties to even as numpy's round
template <int DT, bool U8>
__global__ __launch_bounds__(VAE_THREADS) void vae_output_kernel(const float* __restrict__ x, void* __restrict__ out, int64_t THW, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * VAE_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * VAE_THREADS) {
        const float4 v = reinterpret_cast<const float4*>(x)[4 * i];
        if constexpr (U8) {
            uint8_t* d = reinterpret_cast<uint8_t*>(out) + (size_t)i * 3;
            d[0] = (uint8_t)rintf(fminf(fmaxf(v.x * 0.5f + 0.5f, 0.f), 1.f) * 255.f);
            d[1] = (uint8_t)rintf(fminf(fmaxf(v.y * 0.5f + 0.5f, 0.f), 1.f) * 255.f);
            d[2] = (uint8_t)rintf(fminf(fmaxf(v.z * 0.5f + 0.5f, 0.f), 1.f) * 255.f);
        } else {
            const int64_t n = i / THW, r = i - n * THW;
            const size_t dst = (size_t)n * 3 * THW + r;
            store1<DT>(out, dst, v.x);
            store1<DT>(out, dst + THW, v.y);
            store1<DT>(out, dst + 2 * THW, v.z);
        }
    }
}

// thread = one element of the [N,L,1,h,w] outputs
template <int DT>
__global__ __launch_bounds__(VAE_THREADS) void vae_sample_kernel(const float* __restrict__ moments, const void* __restrict__ noise, float scale,
                                                                  void* __restrict__ sample, void* __restrict__ mean, void* __restrict__ logvar,
                                                                  void* __restrict__ std_, int64_t hw, int L, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * VAE_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * VAE_THREADS) {
        const int64_t p = i % hw, l = (i / hw) % L, n = i / (hw * L);
        const float* m = moments + ((size_t)n * hw + p) * (2 * L);
        const float mu = m[l], lv = fminf(fmaxf(m[L + l], -30.0f), 20.0f), sd = expf(0.5f * lv);
        if (mean) store1<DT>(mean, i, mu);
        if (logvar) store1<DT>(logvar, i, lv);
        if (std_) store1<DT>(std_, i, sd);
        if (sample) store1<DT>(sample, i, (mu + sd * (noise ? load1<DT>(noise, i) : 0.f)) * scale);
    }
}

static bool vae_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// blocks of a grid-stride launch over `total` items: enough for every item up to a cap that keeps the grid index in range
static unsigned vae_blocks(int64_t total) {
    const int64_t b = (total + VAE_THREADS - 1) / VAE_THREADS;
    return (unsigned)(b < (1 << 20) ? b : (1 << 20));
}

extern "C" {

int32_t vgpa_vae_input_f32(const void* x, int32_t in_dtype, float* out, int64_t N, int64_t H, int64_t W, hipStream_t stream) {
    if (!x || !out || N <= 0 || H <= 0 || W <= 0 || H > (1 << 20) || W > (1 << 20) || N > (1 << 20) || !vae_aligned16(out)) return VGPA_ERR_INVALID;
    if (in_dtype != VGPA_DTYPE_F32 && in_dtype != VGPA_DTYPE_BF16) return VGPA_ERR_INVALID;
    const int64_t HW = H * W, total4 = N * HW * 4;
    if (in_dtype == VGPA_DTYPE_BF16) VGPA_LAUNCH(vae_input_kernel<VGPA_DTYPE_BF16>, dim3(vae_blocks(total4)), dim3(VAE_THREADS), 0, stream, x, out, HW, total4);
    else VGPA_LAUNCH(vae_input_kernel<VGPA_DTYPE_F32>, dim3(vae_blocks(total4)), dim3(VAE_THREADS), 0, stream, x, out, HW, total4);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

static bool gn_shape_ok(int64_t N, int64_t HW, int64_t C, int64_t G) {
    return N > 0 && N <= 65535 && HW > 0 && HW <= (1LL << 40) && C > 0 && C <= 4 * VAE_THREADS && (C & 3) == 0 && G > 0 && G <= 65535 && C % G == 0;
}

size_t vgpa_groupnorm_stats_workspace_bytes(int64_t N, int64_t HW, int64_t C, int64_t G) {
    if (!gn_shape_ok(N, HW, C, G)) return 0;
    return (size_t)N * (size_t)gn_tiling(HW, C).chunks * (size_t)C * 2 * sizeof(double);
}

int32_t vgpa_groupnorm_stats_f32(const float* x, float* stats, int64_t N, int64_t HW, int64_t C, int64_t G, float eps, void* workspace, size_t ws_bytes,
                                 hipStream_t stream) {
    if (!x || !stats || !workspace || !gn_shape_ok(N, HW, C, G) || !vae_aligned16(x) || ((uintptr_t)workspace & 7)) return VGPA_ERR_INVALID;
    const GnTiling t = gn_tiling(HW, C);
    if (t.chunks > 0x7fffffffLL) return VGPA_ERR_INVALID;
    if (ws_bytes < vgpa_groupnorm_stats_workspace_bytes(N, HW, C, G)) return VGPA_ERR_WORKSPACE;
    double* part = reinterpret_cast<double*>(workspace);
    VGPA_LAUNCH(gn_partial_kernel, dim3((unsigned)t.chunks, (unsigned)N), dim3(VAE_THREADS), 0, stream, x, part, HW, (int)C, t.ncol, t.rpp, t.ppc);
    VGPA_CHECK_LAUNCH();
    VGPA_LAUNCH(gn_combine_kernel, dim3((unsigned)G, (unsigned)N), dim3(VAE_THREADS), 0, stream, part, stats, HW, (int)C, (int)(C / G), t.ppc, t.chunks, eps);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_groupnorm_silu_f32(const float* x, const float* stats, const float* gamma, const float* beta, float* out, int64_t N, int64_t HW, int64_t C,
                                int64_t G, hipStream_t stream) {
    if (!x || !stats || !gamma || !beta || !out || out == x || !gn_shape_ok(N, HW, C, G)) return VGPA_ERR_INVALID;
    if (!vae_aligned16(x) || !vae_aligned16(out) || !vae_aligned16(gamma) || !vae_aligned16(beta)) return VGPA_ERR_INVALID;
    const int64_t total4 = N * HW * (C / 4);
    VGPA_LAUNCH(gn_silu_kernel, dim3(vae_blocks(total4)), dim3(VAE_THREADS), 0, stream, x, stats, gamma, beta, out, HW, (int)C, (int)G, (int)(C / G), total4);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_spatial_norm_silu_f32(const float* x, const float* stats, const float* gamma, const float* beta, const float* yb, float* out, int64_t N,
                                   int64_t T, int64_t H, int64_t W, int64_t C, int64_t G, int64_t t, int64_t h, int64_t w, hipStream_t stream) {
    if (!x || !stats || !gamma || !beta || !yb || !out || out == x || T <= 0 || H <= 0 || W <= 0 || t <= 0 || h <= 0 || w <= 0) return VGPA_ERR_INVALID;
    if (T > (1 << 15) || t > (1 << 15) || H > (1 << 20) || W > (1 << 20) || !gn_shape_ok(N, T * H * W, C, G)) return VGPA_ERR_INVALID;
    if (H % h || W % w || t > T || (T > 1 && (T & 1) && t < 2)) return VGPA_ERR_INVALID;      // integral spatial ratios; the odd-frame split needs a frame behind frame 0
    if (!vae_aligned16(x) || !vae_aligned16(out) || !vae_aligned16(gamma) || !vae_aligned16(beta) || !vae_aligned16(yb)) return VGPA_ERR_INVALID;
    const int64_t total4 = N * T * H * W * (C / 4);
    VGPA_LAUNCH(spatial_norm_silu_kernel, dim3(vae_blocks(total4)), dim3(VAE_THREADS), 0, stream, x, stats, gamma, beta, yb, out, (int)T, (int)H, (int)W,
                (int)C, (int)G, (int)(C / G), (int)t, (int)h, (int)w, (int)(H / h), (int)(W / w), total4);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_vae_output(const float* x, void* out, int32_t out_dtype, int64_t N, int64_t THW, hipStream_t stream) {
    if (!x || !out || N <= 0 || THW <= 0 || N > (1 << 20) || THW > (1LL << 40) || !vae_aligned16(x)) return VGPA_ERR_INVALID;
    const int64_t total = N * THW;
    const dim3 grid(vae_blocks(total)), block(VAE_THREADS);
    if (out_dtype == VGPA_DTYPE_F32) VGPA_LAUNCH((vae_output_kernel<VGPA_DTYPE_F32, false>), grid, block, 0, stream, x, out, THW, total);
    else if (out_dtype == VGPA_DTYPE_BF16) VGPA_LAUNCH((vae_output_kernel<VGPA_DTYPE_BF16, false>), grid, block, 0, stream, x, out, THW, total);
    else if (out_dtype == VAE_OUT_U8) VGPA_LAUNCH((vae_output_kernel<VGPA_DTYPE_F32, true>), grid, block, 0, stream, x, out, THW, total);
    else return VGPA_ERR_INVALID;
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_vae_sample(const float* moments, const void* noise, float scale, void* sample, void* mean, void* logvar, void* std_out, int32_t out_dtype,
                        int64_t N, int64_t hw, int64_t L, hipStream_t stream) {
    if (!moments || N <= 0 || hw <= 0 || L <= 0 || N > (1 << 20) || hw > (1LL << 40) || L > (1 << 20)) return VGPA_ERR_INVALID;
    if (out_dtype != VGPA_DTYPE_F32 && out_dtype != VGPA_DTYPE_BF16) return VGPA_ERR_INVALID;
    if (!sample && !mean && !logvar && !std_out) return VGPA_ERR_INVALID;
    const int64_t total = N * hw * L;
    if (out_dtype == VGPA_DTYPE_BF16)
        VGPA_LAUNCH(vae_sample_kernel<VGPA_DTYPE_BF16>, dim3(vae_blocks(total)), dim3(VAE_THREADS), 0, stream, moments, noise, scale, sample, mean, logvar,
                    std_out, hw, (int)L, total);
    else
        VGPA_LAUNCH(vae_sample_kernel<VGPA_DTYPE_F32>, dim3(vae_blocks(total)), dim3(VAE_THREADS), 0, stream, moments, noise, scale, sample, mean, logvar,
                    std_out, hw, (int)L, total);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

}  // extern "C"
