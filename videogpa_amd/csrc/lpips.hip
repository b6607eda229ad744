// LPIPS-VGG (lpips 0.1: lpips/lpips.py, pretrained_networks.py), the part around the thirteen 3x3 convolutions, which run on conv_kernel of
// vggt_heads.hip as they are.  Everything fp32, channels-last (NHWC), forward only:
//   lpips_input_kernel     ScalingLayer + layout change in front of conv1_1: [N,3,H,W] in [-1,1] -> [N,H,W,16], channels 0..2 = (x - shift) / scale
//                          (a true division, as upstream), channels 3..15 = 0 so that conv1_1 is a 16-channel convolution with zero weight rows
//   maxpool_kernel         2 x 2 / stride 2 max pool (floor), optionally of relu(x): relu(max) = max(relu), so the ReLU the convolution did not store is free here
//   lpips_layer_kernel     one LPIPS layer in one pass over both feature maps: per pixel normalize_tensor (x / (||x||_2 + 1e-10)) of both, the squared
//                          difference, the `lin` 1x1 convolution (a dot with w), then the spatial mean.  A pixel's channel vector is read ONCE, 2 x 16 bytes
//                          per lane and map, and stays in registers between the norm and the difference: a group of G = C / 8 lanes owns a pixel (G = 64 at
//                          C = 512, 8 at C = 64), the channel sums are xor shuffles inside the group.  Every workgroup leaves one fp64 partial,
//   lpips_finish_kernel    one workgroup per frame adds the frame's partials in a fixed order in fp64: no float atomics.  A frame's tiles and their order
//                          depend on (H, W, C) only, so its value is bit-identical from run to run and for every N / split of the frames over calls.
// Both reductions are HBM-bound by design: algorithmic bytes 2 N H W C 4 for the layer kernel, (1 + 1/4) N H W C 4 for the pool.
#include "common.h"

#define LP_THREADS 256
#define LP_ITERS 8                       // pixels a lane group walks: a workgroup owns (256 / G) * LP_ITERS consecutive pixels of one frame
#define LP_FLAG_RELU 1
#define LP_FLAG_ACCUMULATE 2
#define LP_FLAG_NORMALIZE 1              // input kernel: x is in [0,1], mapped to 2 x - 1 first

struct LpipsAffine {
    float shift[3], scale[3];
};

// thread = one 16-byte quarter of an output pixel: quarter 0 carries the three channels, quarters 1..3 are zero
__global__ __launch_bounds__(LP_THREADS) void lpips_input_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t HW, int64_t total4,
                                                                  const LpipsAffine af, int normalize) {
    const int64_t i = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= total4) return;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((i & 3) == 0) {
        const int64_t p = i >> 2, n = p / HW, r = p - n * HW;
        const float* src = x + (size_t)n * 3 * HW + r;
        float c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float t = src[(size_t)k * HW];
            if (normalize) t = 2.0f * t - 1.0f;
            c[k] = (t - af.shift[k]) / af.scale[k];
        }
        v = make_float4(c[0], c[1], c[2], 0.f);
    }
    reinterpret_cast<float4*>(out)[i] = v;
}

__device__ __forceinline__ float4 lp_max4(float4 a, float4 b) { return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)); }
__device__ __forceinline__ float4 lp_relu4(float4 a) { return make_float4(fmaxf(a.x, 0.f), fmaxf(a.y, 0.f), fmaxf(a.z, 0.f), fmaxf(a.w, 0.f)); }

// thread = four channels of one output pixel
__global__ __launch_bounds__(LP_THREADS) void maxpool_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int C, int Ho, int Wo,
                                                              int64_t total4, int relu) {
    const int64_t i = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= total4) return;
    const int c4n = C >> 2;
    const int c = (int)(i % c4n) * 4;
    const int64_t q = i / c4n;
    const int ox = (int)(q % Wo), oy = (int)((q / Wo) % Ho);
    const int64_t n = q / ((int64_t)Wo * Ho);
    const float* r0 = x + (((size_t)n * H + 2 * oy) * W + 2 * ox) * C + c;
    const float* r1 = r0 + (size_t)W * C;
    const float4 v00 = *reinterpret_cast<const float4*>(r0), v01 = *reinterpret_cast<const float4*>(r0 + C);
    const float4 v10 = *reinterpret_cast<const float4*>(r1), v11 = *reinterpret_cast<const float4*>(r1 + C);
    float4 v = lp_max4(lp_max4(v00, v01), lp_max4(v10, v11));
    if (relu) v = lp_relu4(v);
    reinterpret_cast<float4*>(out)[i] = v;
}

__device__ __forceinline__ float lp_dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
// sum_c w_c (a_c / na - b_c / nb)^2 over four channels
__device__ __forceinline__ float lp_term4(float4 a, float4 b, float4 w, float na, float nb) {
    const float d0 = a.x / na - b.x / nb, d1 = a.y / na - b.y / nb, d2 = a.z / na - b.z / nb, d3 = a.w / na - b.w / nb;
    return w.x * (d0 * d0) + w.y * (d1 * d1) + w.z * (d2 * d2) + w.w * (d3 * d3);
}

// G lanes per pixel (a power of two, 2 G >= C / 4): lane j of a group holds the float4 slots j and j + G of the pixel's C / 4.
// grid.x = N * nbpf, block (frame, tile) with the tile fastest; partial[blockIdx.x] = sum over the tile's pixels.
template <int G>
__global__ __launch_bounds__(LP_THREADS) void lpips_layer_kernel(const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ w,
                                                                  int64_t HW, int C, int relu, int nbpf, double* __restrict__ partial) {
    __shared__ double red[16];
    constexpr int PPW = 64 / G, PPB = PPW * (LP_THREADS / 64), TILE = PPB * LP_ITERS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & (G - 1), pw = lane / G;
    const int64_t n = blockIdx.x / nbpf, tile = blockIdx.x % nbpf;
    const int slots = C >> 2;
    const bool in0 = j < slots, in1 = j + G < slots;
    const int c0 = 4 * j, c1 = 4 * (j + G);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 w0 = in0 ? *reinterpret_cast<const float4*>(w + c0) : z, w1 = in1 ? *reinterpret_cast<const float4*>(w + c1) : z;
    const size_t base = (size_t)n * HW * C;
    double acc = 0.0;
#pragma unroll 2
    for (int it = 0; it < LP_ITERS; ++it) {
        const int64_t p = tile * TILE + it * PPB + wave * PPW + pw;
        const bool pv = p < HW;                                   // a pixel past the frame is all zero: it contributes 0 / (0 + 1e-10) = 0
        const size_t o = base + (size_t)p * C;
        float4 a0 = pv && in0 ? *reinterpret_cast<const float4*>(f0 + o + c0) : z, a1 = pv && in1 ? *reinterpret_cast<const float4*>(f0 + o + c1) : z;
        float4 b0 = pv && in0 ? *reinterpret_cast<const float4*>(f1 + o + c0) : z, b1 = pv && in1 ? *reinterpret_cast<const float4*>(f1 + o + c1) : z;
        if (relu) {
            a0 = lp_relu4(a0); a1 = lp_relu4(a1); b0 = lp_relu4(b0); b1 = lp_relu4(b1);
        }
        float sa = lp_dot4(a0, a0) + lp_dot4(a1, a1), sb = lp_dot4(b0, b0) + lp_dot4(b1, b1);
#pragma unroll
        for (int s = G >> 1; s > 0; s >>= 1) {
            sa += __shfl_xor(sa, s, 64);
            sb += __shfl_xor(sb, s, 64);
        }
        const float na = sqrtf(sa) + 1e-10f, nb = sqrtf(sb) + 1e-10f;
        acc += (double)(lp_term4(a0, b0, w0, na, nb) + lp_term4(a1, b1, w1, na, nb));
    }
    const double s = block_sum<double>(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// grid.x = N: out[n] = (float)(sum of frame n's partials / HW), total[n] (fp64) = that mean, or total[n] + it when `accumulate`
__global__ __launch_bounds__(LP_THREADS) void lpips_finish_kernel(const double* __restrict__ partial, int nbpf, double hw, float* __restrict__ out,
                                                                   double* __restrict__ total, int accumulate) {
    __shared__ double red[16];
    const double* p = partial + (size_t)blockIdx.x * nbpf;
    double s = 0.0;
    for (int i = threadIdx.x; i < nbpf; i += LP_THREADS) s += p[i];
    s = block_sum<double>(s, red);
    if (threadIdx.x == 0) {
        const double m = s / hw;
        if (out) out[blockIdx.x] = (float)m;
        if (total) total[blockIdx.x] = accumulate ? total[blockIdx.x] + m : m;
    }
}

static bool lp_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// lanes per pixel: the smallest power of two with 2 G float4 slots >= C / 4
static int lp_group(int64_t C) {
    int g = 1;
    while (8 * g < C) g <<= 1;
    return g;
}
static int64_t lp_tiles(int64_t HW, int64_t C) {
    const int64_t tile = (int64_t)(64 / lp_group(C)) * (LP_THREADS / 64) * LP_ITERS;
    return (HW + tile - 1) / tile;
}
static bool lp_layer_shape_ok(int64_t N, int64_t H, int64_t W, int64_t C) {
    return N > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && C <= 512 && H <= (1 << 20) && W <= (1 << 20) && N * lp_tiles(H * W, C) <= 0x7fffffffLL;
}

extern "C" {

int32_t vgpa_lpips_input_f32(const float* x, float* out, int64_t N, int64_t H, int64_t W, float shift0, float shift1, float shift2, float scale0,
                             float scale1, float scale2, int32_t flags, hipStream_t stream) {
    if (!x || !out || N <= 0 || H <= 0 || W <= 0 || H > (1 << 20) || W > (1 << 20) || (flags & ~LP_FLAG_NORMALIZE)) return VGPA_ERR_INVALID;
    if (((uintptr_t)x & 3) || !lp_aligned16(out) || !(scale0 != 0.f) || !(scale1 != 0.f) || !(scale2 != 0.f)) return VGPA_ERR_INVALID;
    const int64_t HW = H * W, total4 = N * HW * 4, blocks = (total4 + LP_THREADS - 1) / LP_THREADS;
    if (blocks > 0x7fffffffLL) return VGPA_ERR_INVALID;
    const LpipsAffine af = {{shift0, shift1, shift2}, {scale0, scale1, scale2}};
    VGPA_LAUNCH(lpips_input_kernel, dim3((unsigned)blocks), dim3(LP_THREADS), 0, stream, x, out, HW, total4, af, flags & LP_FLAG_NORMALIZE);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_maxpool2x2_f32(const float* x, float* out, int64_t N, int64_t H, int64_t W, int64_t C, int32_t flags, hipStream_t stream) {
    if (!x || !out || N <= 0 || H < 2 || W < 2 || C <= 0 || (C & 3) || H > (1 << 20) || W > (1 << 20) || C > (1 << 20) || (flags & ~LP_FLAG_RELU))
        return VGPA_ERR_INVALID;
    if (!lp_aligned16(x) || !lp_aligned16(out)) return VGPA_ERR_INVALID;
    const int64_t Ho = H / 2, Wo = W / 2, total4 = N * Ho * Wo * (C / 4), blocks = (total4 + LP_THREADS - 1) / LP_THREADS;
    if (blocks > 0x7fffffffLL) return VGPA_ERR_INVALID;
    VGPA_LAUNCH(maxpool_kernel, dim3((unsigned)blocks), dim3(LP_THREADS), 0, stream, x, out, (int)H, (int)W, (int)C, (int)Ho, (int)Wo, total4,
                flags & LP_FLAG_RELU);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

size_t vgpa_lpips_layer_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t C) {
    if (!lp_layer_shape_ok(N, H, W, C)) return 0;
    return (size_t)(N * lp_tiles(H * W, C)) * sizeof(double);
}

int32_t vgpa_lpips_layer_f32(const float* f0, const float* f1, const float* w, float* out, double* total, int64_t N, int64_t H, int64_t W, int64_t C,
                             int32_t flags, void* workspace, size_t ws_bytes, hipStream_t stream) {
    if (!f0 || !f1 || !w || (!out && !total) || !workspace || !lp_layer_shape_ok(N, H, W, C) || (flags & ~(LP_FLAG_RELU | LP_FLAG_ACCUMULATE)))
        return VGPA_ERR_INVALID;
    if (!lp_aligned16(f0) || !lp_aligned16(f1) || !lp_aligned16(w) || ((uintptr_t)workspace & 7)) return VGPA_ERR_INVALID;
    const int64_t HW = H * W, nbpf = lp_tiles(HW, C), nblk = N * nbpf;
    if (ws_bytes < (size_t)nblk * sizeof(double)) return VGPA_ERR_WORKSPACE;
    double* partial = (double*)workspace;
    const int relu = flags & LP_FLAG_RELU;
#define LP_CASE(G)                                                                                                                          \
    case G:                                                                                                                                 \
        VGPA_LAUNCH(lpips_layer_kernel<G>, dim3((unsigned)nblk), dim3(LP_THREADS), 0, stream, f0, f1, w, HW, (int)C, relu, (int)nbpf, partial); \
        break;
    switch (lp_group(C)) {
        LP_CASE(1) LP_CASE(2) LP_CASE(4) LP_CASE(8) LP_CASE(16) LP_CASE(32) LP_CASE(64)
        default: return VGPA_ERR_INVALID;
    }
#undef LP_CASE
    VGPA_CHECK_LAUNCH();
    VGPA_LAUNCH(lpips_finish_kernel, dim3((unsigned)N), dim3(LP_THREADS), 0, stream, partial, (int)nbpf, (double)HW, out, total,
                (flags & LP_FLAG_ACCUMULATE) ? 1 : 0);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

}  // extern "C"
