// Depth Anything 3's DualDPT head (depth_anything_3/model/dualdpt.py), the one piece that the VGGT head kernels do not already cover: the end of
// the auxiliary branch (dualdpt.py:250-258) in one launch on the convolution core of conv_mfma.h, conv_kernel<.., CV_AUX_TAIL>:
//   loader    the [N,h,w,C] map as it is plus the 0.1-scaled UV embedding from two separable tables, zero padding (the embedded tensor never exists)
//   core      the v_mfma_f32_32x32x2_f32 implicit GEMM, 128 pixels x 32 hidden channels per workgroup
//   epilogue  bias, LayerNorm over the pixel's 32 hidden channels (fp32 mean, biased variance of the centred values, rsqrt(var + eps), affine),
//             ReLU, the 1x1 convolution 32 -> output_dim; preds are written as they are, conf = 1 + exp
// Everything else of the head runs on vggt_heads.hip's entry points.
#include "conv_mfma.h"

extern "C" {

int32_t vgpa_dualdpt_aux_tail_f32(const float* x, const float* xtab, const float* ytab, const float* w1_packed, const float* b1, const float* ln_w,
                                  const float* ln_b, float eps, const float* w2, const float* b2, float* preds, float* conf, int64_t N, int64_t h,
                                  int64_t w, int64_t C, int32_t output_dim, hipStream_t stream) {
    ConvArgs a = {};
    const int32_t rc = tail_args(a, x, xtab, ytab, w1_packed, b1, w2, b2, preds, conf, N, h, w, C, h, w, output_dim);
    if (rc != VGPA_OK || !ln_w || !ln_b || !(eps >= 0.f)) return VGPA_ERR_INVALID;
    a.ln_w = ln_w; a.ln_b = ln_b; a.eps = eps;
    return conv_launch<CV_AUX_TAIL>(a, stream);
}

}  // extern "C"
