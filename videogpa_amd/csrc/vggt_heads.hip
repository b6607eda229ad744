// VGGT prediction heads (vggt/heads/dpt_head.py, camera_head.py), the part that is not torch plumbing.  Everything fp32 in, fp32 out,
// channels-last (NHWC), forward only:
//   conv_kernel<.., CV_CONV>        3x3 (stride 1 | 2, pad 1, or 0 | 1 in front and 0 | 1 behind) or 1x1 convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32:
//                                   a k-ordered fmaf chain, only the summation order differs from torch's conv2d), with the fused pieces a
//                                   ResidualConvUnit / FeatureFusionBlock needs: out = conv(relu?(x)) + bias? + relu?(res)? + res2?
//   conv_kernel<.., CV_CONV_CHUNKED> the convolution of the CogVideoX VAE encoder (vgpa_conv3x3_pad_f32): padding per side, and the K sum in short runs
//                                   (conv_mfma.h), because its outputs are held to a bound that one chain of 9 * 512 fp32 additions does not meet
//   conv_kernel<.., CV_CONV3D>      the encoder's causal 3x3x3 convolution over the frames of a chunk (vgpa_conv3x3x3_causal_f32) and
//   conv_kernel<.., CV_POOL_DOWN>   its downsampler with the temporal pooling in the loader (vgpa_vae_downsample_f32): the chunked core again
//   conv_kernel<.., CV_UP2X>        the decoder's up-sampler (vgpa_vae_upsample_f32): the chunked core over the nearest x2 map (x4 with time), which only
//                                   the loader's index arithmetic forms
//   conv_kernel<.., CV_TAIL>        the end of DPTHead._forward_impl (dpt_head.py:229-247) in one launch on the same core: the loader samples the
//                                   [N,h,w,C] map bilinearly (align_corners=True) at the (H,W) grid and adds the 0.1-scaled UV positional
//                                   embedding from two separable tables; the epilogue is bias + ReLU, the 1x1 conv 32 -> output_dim, activate_head.
//                                   The [N,H,W,C] tensor never exists.
//   upsample_kernel                 NHWC align_corners=True bilinear resize (+ the same separable embedding)
//   attn_small_kernel               fp32 softmax attention of the camera trunk, S <= 128 tokens, one workgroup per (batch, head)
//
// The convolution core, with its GEMM view, tile shapes and LDS layout, lives in conv_mfma.h (csrc/dualdpt.hip instantiates a third mode of it).
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

template <int MODE>
static int32_t conv_entry(const float* x, const float* w, const float* bias, const float* res, const float* res2, float* out, int64_t N, int64_t H,
                          int64_t W, int64_t Cin, int64_t Cout, int ksize, int64_t stride, int pad_lo, int pad_hi, int32_t flags, hipStream_t stream) {
    if (!x || !w || !out || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 15) || (Cout & 15)) return VGPA_ERR_INVALID;
    if ((stride != 1 && stride != 2) || (flags & ~(CV_RELU_IN | CV_RELU_RES)) || H > (1 << 30) || W > (1 << 30) || Cin > (1 << 20) || Cout > (1 << 20))
        return VGPA_ERR_INVALID;
    if (!aligned16(x) || !aligned16(w)) return VGPA_ERR_INVALID;
    ConvArgs a = {};
    a.x = x; a.w = w; a.bias = bias; a.res = res; a.res2 = res2; a.out = out;
    a.N = (int)N; a.H = (int)H; a.W = (int)W; a.Cin = (int)Cin; a.Cout = (int)Cout; a.ksize = ksize; a.stride = (int)stride; a.flags = flags;
    a.pad = pad_lo;
    if (H + pad_lo + pad_hi < ksize || W + pad_lo + pad_hi < ksize) return VGPA_ERR_INVALID;
    a.Ho = (int)((H + pad_lo + pad_hi - ksize) / stride + 1);          // the centred 3x3 (pad 1 | 1): (H - 1) / stride + 1; the 1x1: H
    a.Wo = (int)((W + pad_lo + pad_hi - ksize) / stride + 1);
    a.M = N * a.Ho * a.Wo;
    return conv_launch<MODE>(a, stream);
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

int32_t vgpa_conv3x3_pad_f32(const float* x, const float* w_packed, const float* bias, const float* res, float* out, int64_t N, int64_t H, int64_t W,
                             int64_t Cin, int64_t Cout, int64_t stride, int32_t pad_lo, int32_t pad_hi, hipStream_t stream) {
    if (pad_lo < 0 || pad_lo > 1 || pad_hi < 0 || pad_hi > 1) return VGPA_ERR_INVALID;
    return conv_entry<CV_CONV_CHUNKED>(x, w_packed, bias, res, nullptr, out, N, H, W, Cin, Cout, 3, stride, pad_lo, pad_hi, 0, stream);
}

// The causal 3x3x3 convolution over the frames of a chunk (videogpa_amd/vae.py): only the loader knows about time, see CV_CONV3D in conv_mfma.h
int32_t vgpa_conv3x3x3_causal_f32(const float* x, const float* prev, const float* w_packed, const float* bias, const float* res, float* out, int64_t N,
                                  int64_t T, int64_t H, int64_t W, int64_t Cin, int64_t Cout, hipStream_t stream) {
    if (!x || !w_packed || !out || N <= 0 || T <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 15) || (Cout & 15)) return VGPA_ERR_INVALID;
    if (N > (1 << 20) || T > (1 << 20) || H > (1 << 20) || W > (1 << 20) || Cin > (1 << 20) || Cout > (1 << 20) || N * T > (1 << 30)) return VGPA_ERR_INVALID;
    if (!aligned16(x) || !aligned16(prev) || !aligned16(w_packed) || out == x || out == prev) return VGPA_ERR_INVALID;
    ConvArgs a = {};
    a.x = x; a.prev = prev; a.w = w_packed; a.bias = bias; a.res = res; a.out = out;
    a.N = (int)N; a.T = (int)T; a.H = a.Ho = (int)H; a.W = a.Wo = (int)W; a.Cin = (int)Cin; a.Cout = (int)Cout; a.ksize = 3; a.stride = 1; a.pad = 1;
    a.M = N * T * H * W;
    return conv_launch<CV_CONV3D>(a, stream);
}

// CogVideoXDownsample3D in one launch: the one-sided stride-2 convolution above over N * T' frames, whose loader pools the frame pairs (CV_POOL_DOWN)
int32_t vgpa_vae_downsample_f32(const float* x, const float* w_packed, const float* bias, float* out, int64_t N, int64_t T, int64_t H, int64_t W,
                                int64_t C, int64_t Cout, int32_t compress_time, hipStream_t stream) {
    if (!x || !w_packed || !out || N <= 0 || T <= 0 || H < 2 || W < 2 || C <= 0 || Cout <= 0 || (C & 15) || (Cout & 15)) return VGPA_ERR_INVALID;
    if (N > (1 << 20) || T > (1 << 20) || H > (1 << 20) || W > (1 << 20) || C > (1 << 20) || Cout > (1 << 20) || N * T > (1 << 30)) return VGPA_ERR_INVALID;
    if ((compress_time != 0 && compress_time != 1) || !aligned16(x) || !aligned16(w_packed) || out == x) return VGPA_ERR_INVALID;
    if (!compress_time || T == 1)                                          // nothing to pool: the frames are samples of the 2-D convolution
        return conv_entry<CV_CONV_CHUNKED>(x, w_packed, bias, nullptr, nullptr, out, N * T, H, W, C, Cout, 3, 2, 0, 1, 0, stream);
    ConvArgs a = {};
    a.x = x; a.w = w_packed; a.bias = bias; a.out = out;
    a.Tin = (int)T; a.T = (int)((T + 1) / 2);
    a.N = (int)(N * a.T); a.H = (int)H; a.W = (int)W; a.Cin = (int)C; a.Cout = (int)Cout; a.ksize = 3; a.stride = 2; a.pad = 0;
    a.Ho = (int)((H + 1 - 3) / 2 + 1);                                     // one zero row / column behind the last, none in front
    a.Wo = (int)((W + 1 - 3) / 2 + 1);
    a.M = (int64_t)a.N * a.Ho * a.Wo;
    return conv_launch<CV_POOL_DOWN>(a, stream);
}

// CogVideoXUpsample3D in one launch: the 3x3 padding-1 convolution over N * T' frames of 2H x 2W whose loader reads the source at half the index (CV_UP2X)
int32_t vgpa_vae_upsample_f32(const float* x, const float* w_packed, const float* bias, float* out, int64_t N, int64_t T, int64_t H, int64_t W,
                              int64_t C, int64_t Cout, int32_t compress_time, hipStream_t stream) {
    if (!x || !w_packed || !out || N <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || Cout <= 0 || (C & 15) || (Cout & 15)) return VGPA_ERR_INVALID;
    if (N > (1 << 20) || T > (1 << 20) || H > (1 << 20) || W > (1 << 20) || C > (1 << 20) || Cout > (1 << 20) || N * T > (1 << 29)) return VGPA_ERR_INVALID;
    if ((compress_time != 0 && compress_time != 1) || !aligned16(x) || !aligned16(w_packed) || out == x) return VGPA_ERR_INVALID;
    ConvArgs a = {};
    a.x = x; a.w = w_packed; a.bias = bias; a.out = out;
    a.Tin = (int)T;
    a.T = (int)(!compress_time || T == 1 ? T : (T & 1) ? 2 * T - 1 : 2 * T);   // an odd count keeps frame 0 single
    a.N = (int)(N * a.T); a.H = (int)H; a.W = (int)W; a.Ho = (int)(2 * H); a.Wo = (int)(2 * W);
    a.Cin = (int)C; a.Cout = (int)Cout; a.ksize = 3; a.stride = 1; a.pad = 1;
    a.M = (int64_t)a.N * a.Ho * a.Wo;
    return conv_launch<CV_UP2X>(a, stream);
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
