// VGGT prediction heads (vggt/heads/dpt_head.py, camera_head.py), the part that is not torch plumbing.  Everything fp32 in, fp32 out,
// channels-last (NHWC), forward only:
//   conv_kernel<.., CV_CONV>        3x3 (stride 1 | 2, pad 1, or 0 | 1 in front and 0 | 1 behind) or 1x1 convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32:
//                                   a k-ordered fmaf chain, only the summation order differs from torch's conv2d), with the fused pieces a
//                                   ResidualConvUnit / FeatureFusionBlock needs: out = conv(relu?(x)) + bias? + relu?(res)? + res2?
//   conv_kernel<.., CV_TAIL>        the end of DPTHead._forward_impl (dpt_head.py:229-247) in one launch on the same core: the loader samples the
//                                   [N,h,w,C] map bilinearly (align_corners=True) at the (H,W) grid and adds the 0.1-scaled UV positional
//                                   embedding from two separable tables; the epilogue is bias + ReLU, the 1x1 conv 32 -> output_dim, activate_head.
//                                   The [N,H,W,C] tensor never exists.
//   upsample_kernel                 NHWC align_corners=True bilinear resize (+ the same separable embedding)
//   attn_small_kernel               fp32 softmax attention of the camera trunk, S <= 128 tokens, one workgroup per (batch, head)
//
// The convolution core, with its GEMM view, tile shapes and LDS layout, lives in conv_mfma.h (csrc/dualdpt.hip instantiates a third mode of it,
// csrc/vae_conv.hip the chunked modes of the CogVideoX VAE).
#include "conv_mfma.h"

__global__ __launch_bounds__(256) void upsample_kernel(const float* __restrict__ x, int h, int w, int C, int Ho, int Wo, float sy, float sx,
                                                       const float* __restrict__ xtab, const float* __restrict__ ytab, int64_t total4,
                                                       float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int c4n = C >> 2;
    const int c = (int)(i % c4n) * 4;
    const int64_t q = i / c4n;
    const int ox = (int)(q % Wo), oy = (int)((q / Wo) % Ho);
    const int64_t n = q / ((int64_t)Wo * Ho);
    const float4 v = sample4(x + (size_t)n * h * w * C, h, w, C, sy, sx, oy, ox, c, xtab, ytab);
    *reinterpret_cast<float4*>(out + (size_t)q * C + c) = v;
}

// grid = B * H; q / k / v element (b, h, s, d) at base[b * sb + h * sh + s * ss + d]; o [B,S,H,D].
// LDS: K [S][D + 1] (padded: lane j walks row j), then per wave one q row [D] and one probability row [128].
#define AT_THREADS 256
__global__ __launch_bounds__(AT_THREADS) void attn_small_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                 int64_t sb, int64_t sh, int64_t ss, float* __restrict__ o, int H, int S, int D,
                                                                 float scale) {
    extern __shared__ float at_lds[];
    float* Ks = at_lds;
    float* qs = Ks + S * (D + 1) + (threadIdx.x >> 6) * (D + 128);
    float* ps = qs + D;
    const int b = blockIdx.x / H, hd = blockIdx.x % H;
    const size_t base = (size_t)b * sb + (size_t)hd * sh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < S * D; i += AT_THREADS) {
        const int s = i / D, d = i - s * D;
        Ks[s * (D + 1) + d] = k[base + (size_t)s * ss + d];
    }
    __syncthreads();
    for (int i0 = 0; i0 < S; i0 += AT_THREADS / 64) {
        const int i = i0 + wave;
        const bool on = i < S;
        if (on)
            for (int d = lane; d < D; d += 64) qs[d] = q[base + (size_t)i * ss + d];
        __syncthreads();
        float sc[2], m = -INFINITY;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = lane + 64 * t;
            float s = -INFINITY;
            if (on && j < S) {
                s = 0.f;
                for (int d = 0; d < D; ++d) s = fmaf(qs[d], Ks[j * (D + 1) + d], s);
                s *= scale;
            }
            sc[t] = s;
            m = fmaxf(m, s);
        }
        m = wave_max(m);
        float e[2], sum = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            e[t] = (on && lane + 64 * t < S) ? expf(sc[t] - m) : 0.f;
            sum += e[t];
        }
        sum = wave_sum(sum);
#pragma unroll
        for (int t = 0; t < 2; ++t) ps[lane + 64 * t] = e[t] / sum;
        __syncthreads();
        if (on) {
            for (int d = lane; d < D; d += 64) {
                float acc = 0.f;
                for (int j = 0; j < S; ++j) acc = fmaf(ps[j], v[base + (size_t)j * ss + d], acc);
                o[(((size_t)b * S + i) * H + hd) * D + d] = acc;
            }
        }
        __syncthreads();
    }
}

extern "C" {

int32_t vgpa_conv3x3_f32(const float* x, const float* w_packed, const float* bias, const float* res, const float* res2, float* out, int64_t N,
                         int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t stride, int32_t flags, hipStream_t stream) {
    return conv_entry<CV_CONV>(x, w_packed, bias, res, res2, out, N, H, W, Cin, Cout, 3, stride, 1, 1, flags, stream);
}

int32_t vgpa_conv1x1_f32(const float* x, const float* w_packed, const float* bias, float* out, int64_t M, int64_t Cin, int64_t Cout,
                         hipStream_t stream) {
    return conv_entry<CV_CONV>(x, w_packed, bias, nullptr, nullptr, out, 1, 1, M, Cin, Cout, 1, 1, 0, 0, 0, stream);
}

int32_t vgpa_conv1x1_relu_f32(const float* x, const float* w_packed, const float* bias, float* out, int64_t M, int64_t Cin, int64_t Cout,
                              hipStream_t stream) {
    return conv_entry<CV_CONV>(x, w_packed, bias, nullptr, nullptr, out, 1, 1, M, Cin, Cout, 1, 1, 0, 0, CV_RELU_IN, stream);
}

int32_t vgpa_dpt_tail_f32(const float* x, const float* xtab, const float* ytab, const float* w1_packed, const float* b1, const float* w2,
                          const float* b2, float* preds, float* conf, int64_t N, int64_t h, int64_t w, int64_t C, int64_t H, int64_t W,
                          int32_t output_dim, int32_t activation, hipStream_t stream) {
    ConvArgs a = {};
    const int32_t rc = tail_args(a, x, xtab, ytab, w1_packed, b1, w2, b2, preds, conf, N, h, w, C, H, W, output_dim);
    if (rc != VGPA_OK || (activation != 0 && activation != 1)) return VGPA_ERR_INVALID;
    a.act = activation;
    a.sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    a.sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    return conv_launch<CV_TAIL>(a, stream);
}

int32_t vgpa_upsample_bilinear_ac_f32(const float* x, const float* xtab, const float* ytab, float* out, int64_t N, int64_t h, int64_t w, int64_t C,
                                      int64_t H, int64_t W, hipStream_t stream) {
    if (!x || !out || N <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7) || (xtab == nullptr) != (ytab == nullptr))
        return VGPA_ERR_INVALID;
    if (h > (1 << 20) || w > (1 << 20) || H > (1 << 20) || W > (1 << 20) || C > (1 << 20)) return VGPA_ERR_INVALID;
    if (!aligned16(x) || !aligned16(out) || !aligned16(xtab) || !aligned16(ytab)) return VGPA_ERR_INVALID;
    const int64_t total4 = N * H * W * (C / 4), blocks = (total4 + 255) / 256;
    if (blocks > 0x7fffffffLL) return VGPA_ERR_INVALID;
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    VGPA_LAUNCH(upsample_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, (int)h, (int)w, (int)C, (int)H, (int)W, sy, sx, xtab, ytab, total4,
                out);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_attn_small_f32(const float* q, const float* k, const float* v, int64_t stride_b, int64_t stride_h, int64_t stride_s, float* o,
                            int64_t B, int64_t H, int64_t S, int64_t D, float scale, hipStream_t stream) {
    if (!q || !k || !v || !o || B <= 0 || H <= 0 || S <= 0 || S > 128 || D <= 0 || D > 256 || (D & 31) || B * H > 0x7fffffffLL) return VGPA_ERR_INVALID;
    const size_t lds = (size_t)(S * (D + 1) + (AT_THREADS / 64) * (D + 128)) * sizeof(float);
    if (lds > 160 * 1024) return VGPA_ERR_INVALID;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)attn_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return VGPA_ERR_LAUNCH;
    VGPA_LAUNCH(attn_small_kernel, dim3((unsigned)(B * H)), dim3(AT_THREADS), lds, stream, q, k, v, stride_b, stride_h, stride_s, o, (int)H, (int)S,
                (int)D, scale);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

}  // extern "C"
