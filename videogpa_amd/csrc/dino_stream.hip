// The residual stream of the DINOv2 backbone in fp32 (vggt/layers/block.py:77-98 as bf16 autocast evaluates it: LayerNorm and the x + gamma * y adds in
// fp32, only the GEMM / attention operands in bf16).  One launch per use, one workgroup per token row:
//   x_new = x + gamma * y          (y bf16: the projection / MLP output; gamma = LayerScale; skipped when y is NULL)
//   n     = LN(x_new) * w + b      (bf16 for the next GEMM, or fp32 for the backbone's final norm; skipped when w is NULL)
// The aggregator's own blocks keep a bf16 stream (residual_ln.hip); behind a final LayerNorm the three extra roundings per block that costs were 2-3.7 x
// the noise of the autocast evaluation, so this forward-only path carries fp32.  HBM-bound: a row is read once from HBM (the later passes hit the cache).
#include "common.h"

#define SL_THREADS 256

__global__ __launch_bounds__(SL_THREADS) void stream_ln_kernel(const float* __restrict__ x, const bf16_t* __restrict__ y, const float* __restrict__ gamma,
                                                               const float* __restrict__ w, const float* __restrict__ b, float eps, int D,
                                                               float* __restrict__ x_new, void* __restrict__ n, int n_bf16) {
    __shared__ float red[16];
    const size_t row = (size_t)blockIdx.x * D;
    const float* src = x + row;
    float s = 0.f;
    if (y) {
        for (int d = threadIdx.x; d < D; d += SL_THREADS) {
            const float v = x[row + d] + gamma[d] * bf16_to_f32(y[row + d]);
            x_new[row + d] = v;            // read back below by the thread that wrote it
            s += v;
        }
        src = x_new + row;
    } else if (w) {
        for (int d = threadIdx.x; d < D; d += SL_THREADS) s += src[d];
    }
    if (!w) return;
    const float mean = block_sum(s, red) / (float)D;
    float q = 0.f;
    for (int d = threadIdx.x; d < D; d += SL_THREADS) {
        const float c = src[d] - mean;
        q += c * c;
    }
    const float rstd = rsqrtf(block_sum(q, red) / (float)D + eps);
    for (int d = threadIdx.x; d < D; d += SL_THREADS) {
        const float v = (src[d] - mean) * rstd * w[d] + b[d];
        if (n_bf16) reinterpret_cast<bf16_t*>(n)[row + d] = f32_to_bf16(v);
        else reinterpret_cast<float*>(n)[row + d] = v;
    }
}

extern "C" {

int32_t vgpa_stream_ln_f32(const float* x, const void* y, const float* gamma, const float* ln_w, const float* ln_b, float* x_new, void* n,
                           int32_t n_dtype, int64_t M, int64_t D, float eps, hipStream_t stream) {
    if (!x || M <= 0 || D <= 0 || M > 0x7fffffffLL || D > (1 << 20)) return VGPA_ERR_INVALID;
    const bool add = y != nullptr, norm = ln_w != nullptr;
    if ((gamma != nullptr) != add || (x_new != nullptr) != add || (ln_b != nullptr) != norm || (n != nullptr) != norm || (!add && !norm))
        return VGPA_ERR_INVALID;
    if (n_dtype != VGPA_DTYPE_F32 && n_dtype != VGPA_DTYPE_BF16) return VGPA_ERR_INVALID;
    if (x_new == x) return VGPA_ERR_INVALID;
    VGPA_LAUNCH(stream_ln_kernel, dim3((unsigned)M), dim3(SL_THREADS), 0, stream, x, reinterpret_cast<const bf16_t*>(y), gamma, ln_w, ln_b, eps, (int)D,
                x_new, n, n_dtype == VGPA_DTYPE_BF16);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

}  // extern "C"
