// Geometry-consistency scorer, third file: SSIMMetric (metrics/mse.py:101-134), i.e. piq.ssim(gt, rep, data_range=1.0) with its
// defaults kernel_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03, downsample=True, reduction="mean", full=False:
//   f = max(1, round_half_even(min(H, W) / 256)); both images through avg_pool2d(f) (trailing rows / columns dropped);
//   11 x 11 Gaussian window (sigma 1.5, sum 1), "valid" correlation per channel of x, y, x^2, y^2, xy;
//   ss = (2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1) * (2 s_xy + c2) / (s_xx + s_yy + c2), c1 = 1e-4, c2 = 9e-4;
//   mean over the valid positions and the channels -> one value per frame; mean over the frames.
// One fused pass: a workgroup owns a 32 x 24 output tile of one frame (one channel of a planar image, up to three interleaved
// channels when an image is [T,H,W,C]), loads the 42 x 34 pooled halo of BOTH images into LDS -- range normalisation and the f x f
// average applied on load, so the pooled images never exist in HBM --, filters separably in LDS (rows, then columns in registers)
// and leaves one fp64 partial sum.  A one-block kernel reduces the partials per frame in a fixed order: no float atomics, the
// result is run-to-run bit-identical.  Each input byte is read once for the range decision and 42 * 34 / (32 * 24) = 1.9 times for the
// halo (mostly from L2); no MFMA.  Measured: the tile kernel is bound by load latency at 2-4 workgroups per CU,
// not by HBM.  All arithmetic fp32, every 11-tap sum in ascending tap order.
#include "common.h"

#pragma clang fp contract(off)

#define SS_THREADS 256
#define SS_WIN 11
#define SS_TW 32                         // output tile: 32 wide (one half-wave per row) ...
#define SS_ROWS 3                        // ... and SS_THREADS / SS_TW * SS_ROWS = 24 tall: a thread owns SS_ROWS outputs of one column
#define SS_TH (SS_THREADS / SS_TW * SS_ROWS)
#define SS_HW (SS_TW + SS_WIN - 1)       // 42 x 34 pooled pixels of halo per tile
#define SS_HH (SS_TH + SS_WIN - 1)
#define SS_MAXCH 3                       // interleaved channels one workgroup takes together (56 KB of LDS then, 33 KB for one channel)

struct SsimWin {
    float w[SS_WIN];
};

struct SsimImg {
    const void* p;
    int dtype, layout, is_tensor;        // 0 f32 / 2 u8; 0 [T,C,H,W] / 1 [T,H,W,C]; torch.Tensor vs numpy range rule
};

__device__ __forceinline__ uint32_t ss_ordered(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ss_unordered(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// min / max of both images for the range decision of _to_tensor_01, one launch (blockIdx.y = image): 16-byte loads where the pointer
// allows, a block reduction, then ONE integer atomicMax pair per block on order-preserving bit patterns (mm[2 * img] = ~min,
// mm[2 * img + 1] = max, zero-initialised) -- same-address atomics serialise in L2, so their count is kept at the grid size, and
// being integer maxima their arrival order does not matter.
__global__ __launch_bounds__(SS_THREADS) void ssim_minmax_kernel(const SsimImg gt, const SsimImg rep, int64_t n, uint32_t* __restrict__ mm) {
    __shared__ uint32_t red[2][SS_THREADS / 64];
    const void* a = blockIdx.y ? rep.p : gt.p;
    const int dtype = blockIdx.y ? rep.dtype : gt.dtype;
    const bool vec_ok = ((uintptr_t)a & 15) == 0;
    uint32_t lo = 0, hi = 0;
    const int64_t gid = (int64_t)blockIdx.x * SS_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * SS_THREADS;
    int64_t done = 0;
    if (vec_ok && dtype == 2) {
        const int64_t nv = n / 16;
        const uint4* p = reinterpret_cast<const uint4*>(a);
        uint32_t bmin = 255u, bmax = 0u;
#pragma unroll 4
        for (int64_t i = gid; i < nv; i += stride) {
            const uint4 v = p[i];
            const uint32_t wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int sh = 0; sh < 32; sh += 8) {
                    const uint32_t b = (wds[q] >> sh) & 255u;
                    bmin = min(bmin, b);
                    bmax = max(bmax, b);
                }
            }
        }
        if (bmin <= bmax) {
            hi = ss_ordered((float)bmax);
            lo = ~ss_ordered((float)bmin);
        }
        done = nv * 16;
    } else if (vec_ok) {
        const int64_t nv = n / 4;
        const float4* p = reinterpret_cast<const float4*>(a);
#pragma unroll 4
        for (int64_t i = gid; i < nv; i += stride) {
            const float4 v = p[i];
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t o = ss_ordered(e[q]);
                hi = max(hi, o);
                lo = max(lo, ~o);
            }
        }
        done = nv * 4;
    }
    for (int64_t i = done + gid; i < n; i += stride) {
        const float x = dtype == 2 ? (float)reinterpret_cast<const uint8_t*>(a)[i] : reinterpret_cast<const float*>(a)[i];
        const uint32_t o = ss_ordered(x);
        hi = max(hi, o);
        lo = max(lo, ~o);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, 64));
        lo = max(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = lo;
        red[1][threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < SS_THREADS / 64; ++w) {
            lo = max(lo, red[0][w]);
            hi = max(hi, red[1][w]);
        }
        atomicMax(&mm[2 * blockIdx.y], lo);
        atomicMax(&mm[2 * blockIdx.y + 1], hi);
    }
}

__device__ __forceinline__ float ss_to01(float x, float mn, float mx, int is_tensor) {   // metrics/mse.py:112-134
    if (is_tensor && mn < 0.f) return (x + 1.0f) / 2.0f;
    if (mx > 1.0f) return x / 255.0f;
    return x;
}

// One pooled, normalised halo pixel of one image.  The work index runs along the image's innermost memory axis (x for planar,
// (x, c) for interleaved frames), so a wave's loads cover whole cache lines and the channel de-interleave happens in the LDS
// store, not in the global load.  F = the pool factor when it is 1 or 2 (its F * F loads are then issued together), 0 = any.
template <int F>
__device__ __forceinline__ void ss_halo_px(const SsimImg im, float mn, float mx, int64_t t, int c0, int nch, int C, int H, int W, int f_rt,
                                           int PH, int PW, int py0, int px0, int idx, float* __restrict__ dst) {
    const int f = F ? F : f_rt;
    int c, py, px;
    if (im.layout) {
        c = idx % nch;
        px = (idx / nch) % SS_HW;
        py = idx / (nch * SS_HW);
    } else {
        px = idx % SS_HW;
        py = (idx / SS_HW) % SS_HH;
        c = idx / (SS_HH * SS_HW);
    }
    const int gy = py0 + py, gx = px0 + px;
    float v = 0.f;
    if (gy < PH && gx < PW) {
        const auto raw01 = [&](int dy, int dx) {
            const int y = gy * f + dy, x = gx * f + dx;
            const size_t i = im.layout ? (((size_t)(t * H + y) * W + x) * C + (c0 + c)) : (((size_t)(t * C + (c0 + c)) * H + y) * W + x);
            const float raw = im.dtype == 2 ? (float)reinterpret_cast<const uint8_t*>(im.p)[i] : reinterpret_cast<const float*>(im.p)[i];
            return ss_to01(raw, mn, mx, im.is_tensor);
        };
        float s = 0.f;                                    // row-major over the window, as avg_pool2d sums it
        if constexpr (F > 0) {
#pragma unroll
            for (int dy = 0; dy < F; ++dy)
#pragma unroll
                for (int dx = 0; dx < F; ++dx) s += raw01(dy, dx);
        } else {
            for (int dy = 0; dy < f; ++dy)
                for (int dx = 0; dx < f; ++dx) s += raw01(dy, dx);
        }
        // avg_pool2d: the window sum over f * f (a multiplication by the exact reciprocal when f is a power of two)
        v = f == 1 ? s : ((f & (f - 1)) == 0 ? s * (1.0f / (float)(f * f)) : s / (float)(f * f));
    }
    dst[(c * SS_HH + py) * SS_HW + px] = v;
}

// Both halos -> sx / sy [ch][SS_HH][SS_HW] (zeros outside the pooled image); gt and rep are handled in the same iteration so that
// their loads are in flight together: the pass is bound by load latency, not by arithmetic.
template <int F>
__device__ __forceinline__ void ss_load_halos(const SsimImg gt, const SsimImg rep, float amin, float amax, float bmin, float bmax, int64_t t,
                                              int c0, int nch, int C, int H, int W, int f, int PH, int PW, int py0, int px0,
                                              float* __restrict__ sx, float* __restrict__ sy) {
    const int n = nch * SS_HH * SS_HW;
#pragma unroll 2
    for (int idx = threadIdx.x; idx < n; idx += SS_THREADS) {
        ss_halo_px<F>(gt, amin, amax, t, c0, nch, C, H, W, f, PH, PW, py0, px0, idx, sx);
        ss_halo_px<F>(rep, bmin, bmax, t, c0, nch, C, H, W, f, PH, PW, py0, px0, idx, sy);
    }
}

// grid.x = T * nchunk * ntile, block (t, chunk, tile) with the tile fastest; partial[blockIdx.x] = sum of ss over the block's outputs.
// Dynamic LDS: 2 * nch_max planes of SS_HH * SS_HW floats (the halos) + 5 * SS_HH * SS_TW floats (the row-filtered moments).
__global__ __launch_bounds__(SS_THREADS) void ssim_tile_kernel(const SsimImg gt, const SsimImg rep, const SsimWin win, int C, int H, int W, int f,
                                                                int PH, int PW, int OH, int OW, int tiles_x, int ntile, int nchunk, int nch_max,
                                                                const uint32_t* __restrict__ mm, double* __restrict__ partial) {
    extern __shared__ float ss_lds[];
    __shared__ double red[16];
    float* sx = ss_lds;
    float* sy = sx + nch_max * SS_HH * SS_HW;
    float* hm = sy + nch_max * SS_HH * SS_HW;       // [5][SS_HH][SS_TW]
    const float amin = ss_unordered(~mm[0]), amax = ss_unordered(mm[1]), bmin = ss_unordered(~mm[2]), bmax = ss_unordered(mm[3]);
    const int tile = blockIdx.x % ntile;
    const int chunk = (blockIdx.x / ntile) % nchunk;
    const int64_t t = blockIdx.x / (ntile * nchunk);
    const int c0 = chunk * nch_max;
    const int nch = min(nch_max, C - c0);
    const int oy0 = (tile / tiles_x) * SS_TH, ox0 = (tile % tiles_x) * SS_TW;

    if (f == 1) ss_load_halos<1>(gt, rep, amin, amax, bmin, bmax, t, c0, nch, C, H, W, f, PH, PW, oy0, ox0, sx, sy);
    else if (f == 2) ss_load_halos<2>(gt, rep, amin, amax, bmin, bmax, t, c0, nch, C, H, W, f, PH, PW, oy0, ox0, sx, sy);
    else ss_load_halos<0>(gt, rep, amin, amax, bmin, bmax, t, c0, nch, C, H, W, f, PH, PW, oy0, ox0, sx, sy);
    __syncthreads();

    const int j = threadIdx.x % SS_TW, i0 = (threadIdx.x / SS_TW) * SS_ROWS;
    float acc = 0.f;
    for (int c = 0; c < nch; ++c) {
        // row pass: lanes run along x, so the LDS reads and writes of a half-wave are 32 consecutive dwords (no bank conflict, no padding needed)
        for (int idx = threadIdx.x; idx < SS_HH * SS_TW; idx += SS_THREADS) {
            const int r = idx / SS_TW, jj = idx % SS_TW;
            const float* xr = sx + (c * SS_HH + r) * SS_HW + jj;
            const float* yr = sy + (c * SS_HH + r) * SS_HW + jj;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
            for (int k = 0; k < SS_WIN; ++k) {
                const float xv = xr[k], yv = yr[k], wk = win.w[k];
                a0 += wk * xv;
                a1 += wk * yv;
                a2 += wk * (xv * xv);
                a3 += wk * (yv * yv);
                a4 += wk * (xv * yv);
            }
            hm[(0 * SS_HH + r) * SS_TW + jj] = a0;
            hm[(1 * SS_HH + r) * SS_TW + jj] = a1;
            hm[(2 * SS_HH + r) * SS_TW + jj] = a2;
            hm[(3 * SS_HH + r) * SS_TW + jj] = a3;
            hm[(4 * SS_HH + r) * SS_TW + jj] = a4;
        }
        __syncthreads();
        // column pass: a thread owns SS_ROWS consecutive outputs of one column; the 13 rows they share are read once, lanes again along x
        float o[5][SS_ROWS];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            float v[SS_ROWS + SS_WIN - 1];
#pragma unroll
            for (int k = 0; k < SS_ROWS + SS_WIN - 1; ++k) v[k] = hm[(m * SS_HH + i0 + k) * SS_TW + j];
#pragma unroll
            for (int q = 0; q < SS_ROWS; ++q) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < SS_WIN; ++k) s += win.w[k] * v[q + k];
                o[m][q] = s;
            }
        }
#pragma unroll
        for (int q = 0; q < SS_ROWS; ++q) {
            if (oy0 + i0 + q < OH && ox0 + j < OW) {
                const float mu_x = o[0][q], mu_y = o[1][q];
                const float mu_xx = mu_x * mu_x, mu_yy = mu_y * mu_y, mu_xy = mu_x * mu_y;
                const float s_xx = o[2][q] - mu_xx, s_yy = o[3][q] - mu_yy, s_xy = o[4][q] - mu_xy;
                const float cs = (2.0f * s_xy + 9e-4f) / (s_xx + s_yy + 9e-4f);
                acc += (2.0f * mu_xy + 1e-4f) / (mu_xx + mu_yy + 1e-4f) * cs;
            }
        }
        __syncthreads();                                  // hm is overwritten by the next channel
    }
    const double s = block_sum<double>((double)acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// per_frame[t] = sum of the frame's nbpf partials / n_per_frame; mean[0] = mean of the (fp32) per-frame values.  One block, fixed order.
__global__ __launch_bounds__(SS_THREADS) void ssim_finish_kernel(const double* __restrict__ partial, int nbpf, int T, double inv_n,
                                                                  float* __restrict__ per_frame, float* __restrict__ mean) {
    __shared__ double red[16];
    double tot = 0;
    for (int t = 0; t < T; ++t) {
        double s = 0;
        for (int i = threadIdx.x; i < nbpf; i += SS_THREADS) s += partial[(size_t)t * nbpf + i];
        s = block_sum<double>(s, red);
        const float v = (float)(s * inv_n);
        if (threadIdx.x == 0 && per_frame) per_frame[t] = v;
        tot += (double)v;
    }
    if (threadIdx.x == 0 && mean) mean[0] = (float)(tot / (double)T);
}

// piq's downsample factor: max(1, round(min(H, W) / 256)) with Python's round (half to even)
static int ssim_factor(int64_t H, int64_t W, int downsample) {
    if (!downsample) return 1;
    const int64_t m = H < W ? H : W;
    int64_t q = m / 256;
    const int64_t r = m % 256;
    if (r > 128 || (r == 128 && (q & 1))) ++q;
    return (int)(q < 1 ? 1 : q);
}

static int64_t ssim_tiles(int64_t n_out, int edge) { return (n_out + edge - 1) / edge; }

extern "C" {

// Enough for any downsample flag: the partial count is largest without pooling and with one channel per block.
size_t vgpa_frame_ssim_workspace_bytes(int64_t T, int64_t C, int64_t H, int64_t W) {
    size_t blocks = 0;
    if (T > 0 && C > 0 && H >= SS_WIN && W >= SS_WIN) blocks = (size_t)(T * C * ssim_tiles(H - SS_WIN + 1, SS_TH) * ssim_tiles(W - SS_WIN + 1, SS_TW));
    return blocks * sizeof(double) + 4 * sizeof(uint32_t);
}

// SSIMMetric.compute, metrics/mse.py:101-134 (piq.ssim with the defaults above).  gt / rep [T,C,H,W] or [T,H,W,C] of one spatial size
// (SSIM does not resize); out_per_frame [T] and / or out_mean [1] (either may be NULL).  downsample = 0 switches piq's average pool off.
int32_t vgpa_frame_ssim(const void* gt, int32_t gt_dtype, int32_t gt_layout, int32_t gt_is_tensor, const void* rep, int32_t rep_dtype,
                        int32_t rep_layout, int32_t rep_is_tensor, int64_t T, int64_t C, int64_t H, int64_t W, int32_t downsample,
                        float* out_per_frame, float* out_mean, void* workspace, size_t ws_bytes, hipStream_t stream) {
    if (!gt || !rep || (!out_per_frame && !out_mean) || !workspace || T <= 0 || C <= 0 || H <= 0 || W <= 0) return VGPA_ERR_INVALID;
    if ((gt_dtype != 0 && gt_dtype != 2) || (rep_dtype != 0 && rep_dtype != 2)) return VGPA_ERR_INVALID;
    if ((gt_layout != 0 && gt_layout != 1) || (rep_layout != 0 && rep_layout != 1)) return VGPA_ERR_INVALID;
    if (H > (1 << 24) || W > (1 << 24)) return VGPA_ERR_INVALID;
    const int f = ssim_factor(H, W, downsample);
    const int64_t PH = H / f, PW = W / f;
    if (PH < SS_WIN || PW < SS_WIN) return VGPA_ERR_INVALID;
    const int64_t OH = PH - SS_WIN + 1, OW = PW - SS_WIN + 1;
    const int64_t tiles_x = ssim_tiles(OW, SS_TW), ntile = tiles_x * ssim_tiles(OH, SS_TH);
    // interleaved frames: a block takes up to SS_MAXCH channels together, so that it uses every byte of the lines it loads
    const int nch_max = (gt_layout || rep_layout) ? (int)(C < SS_MAXCH ? C : SS_MAXCH) : 1;
    const int64_t nchunk = (C + nch_max - 1) / nch_max;
    const int64_t nbpf = ntile * nchunk, nblk = nbpf * T;
    if (nblk > 0x7fffffffLL || C > 0x7fffffffLL) return VGPA_ERR_INVALID;
    if (ws_bytes < (size_t)nblk * sizeof(double) + 4 * sizeof(uint32_t)) return VGPA_ERR_WORKSPACE;
    double* partial = (double*)workspace;
    uint32_t* mm = (uint32_t*)((char*)workspace + (size_t)nblk * sizeof(double));

    SsimWin win;
    {
        double g[SS_WIN], sum = 0;
        for (int k = 0; k < SS_WIN; ++k) {
            const double d = (double)(k - SS_WIN / 2);
            g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
            sum += g[k];
        }
        for (int k = 0; k < SS_WIN; ++k) win.w[k] = (float)(g[k] / sum);
    }
    const SsimImg a = {gt, gt_dtype, gt_layout, gt_is_tensor}, b = {rep, rep_dtype, rep_layout, rep_is_tensor};
    const int64_t n = T * C * H * W;
    int64_t mmb = (n / 16 + SS_THREADS - 1) / SS_THREADS;
    mmb = mmb < 1 ? 1 : (mmb > 512 ? 512 : mmb);
    if (hipMemsetAsync(mm, 0, 4 * sizeof(uint32_t), stream) != hipSuccess) return VGPA_ERR_LAUNCH;
    VGPA_LAUNCH(ssim_minmax_kernel, dim3((unsigned)mmb, 2), dim3(SS_THREADS), 0, stream, a, b, n, mm);
    VGPA_CHECK_LAUNCH();
    const size_t lds = (size_t)(2 * nch_max * SS_HH * SS_HW + 5 * SS_HH * SS_TW) * sizeof(float);
    VGPA_LAUNCH(ssim_tile_kernel, dim3((unsigned)nblk), dim3(SS_THREADS), lds, stream, a, b, win, (int)C, (int)H, (int)W, f, (int)PH, (int)PW,
                (int)OH, (int)OW, (int)tiles_x, (int)ntile, (int)nchunk, nch_max, mm, partial);
    VGPA_CHECK_LAUNCH();
    VGPA_LAUNCH(ssim_finish_kernel, dim3(1), dim3(SS_THREADS), 0, stream, partial, (int)nbpf, (int)T, 1.0 / ((double)C * (double)OH * (double)OW),
                out_per_frame, out_mean);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

}  // extern "C"
