// The convolutions of the CogVideoX VAE (videogpa_amd/vae.py), encoder and decoder: the four chunked modes of the exact-fp32 MFMA core of conv_mfma.h
// (CV_CONV_CHUNKED, CV_CONV3D, CV_POOL_DOWN, CV_UP2X; their loaders and the K sum in short runs are described there).  The K sum is chunked because the
// outputs are held to a bound that one chain of 9 * 512 fp32 additions does not meet.  Everything fp32 in, fp32 out, channels-last, forward only.
// What stands around the convolutions (layout changes, GroupNorm, the spatial norm, the Gaussian epilogue) is csrc/vae.hip.
#include "conv_mfma.h"

// The checks and the ConvArgs fill that the three frame-wise entry points share: x [N,T,H,W,Cin] and a 3x3(x3) weight [taps][Cin][Cout], H and W at least
// min_hw, N * T at most nt_cap.  An entry adds its own checks and the fields its mode reads (frames, output size, stride and padding) and launches.
static int32_t frames_args(ConvArgs& a, const float* x, const float* w_packed, const float* bias, float* out, int64_t N, int64_t T, int64_t H, int64_t W,
                           int64_t Cin, int64_t Cout, int64_t min_hw, int64_t nt_cap) {
    if (!x || !w_packed || !out || N <= 0 || T <= 0 || H < min_hw || W < min_hw || Cin <= 0 || Cout <= 0 || (Cin & 15) || (Cout & 15)) return VGPA_ERR_INVALID;
    if (N > (1 << 20) || T > (1 << 20) || H > (1 << 20) || W > (1 << 20) || Cin > (1 << 20) || Cout > (1 << 20) || N * T > nt_cap) return VGPA_ERR_INVALID;
    if (!aligned16(x) || !aligned16(w_packed) || out == x) return VGPA_ERR_INVALID;
    a.x = x; a.w = w_packed; a.bias = bias; a.out = out;
    a.H = (int)H; a.W = (int)W; a.Cin = (int)Cin; a.Cout = (int)Cout; a.ksize = 3;
    return VGPA_OK;
}

extern "C" {

int32_t vgpa_conv3x3_pad_f32(const float* x, const float* w_packed, const float* bias, const float* res, float* out, int64_t N, int64_t H, int64_t W,
                             int64_t Cin, int64_t Cout, int64_t stride, int32_t pad_lo, int32_t pad_hi, hipStream_t stream) {
    if (pad_lo < 0 || pad_lo > 1 || pad_hi < 0 || pad_hi > 1) return VGPA_ERR_INVALID;
    return conv_entry<CV_CONV_CHUNKED>(x, w_packed, bias, res, nullptr, out, N, H, W, Cin, Cout, 3, stride, pad_lo, pad_hi, 0, stream);
}

// The causal 3x3x3 convolution over the frames of a chunk (videogpa_amd/vae.py): only the loader knows about time, see CV_CONV3D in conv_mfma.h
int32_t vgpa_conv3x3x3_causal_f32(const float* x, const float* prev, const float* w_packed, const float* bias, const float* res, float* out, int64_t N,
                                  int64_t T, int64_t H, int64_t W, int64_t Cin, int64_t Cout, hipStream_t stream) {
    ConvArgs a = {};
    if (frames_args(a, x, w_packed, bias, out, N, T, H, W, Cin, Cout, 1, 1 << 30) != VGPA_OK || !aligned16(prev) || out == prev) return VGPA_ERR_INVALID;
    a.prev = prev; a.res = res;
    a.N = (int)N; a.T = (int)T; a.Ho = a.H; a.Wo = a.W; a.stride = 1; a.pad = 1;
    a.M = N * T * H * W;
    return conv_launch<CV_CONV3D>(a, stream);
}

// CogVideoXDownsample3D in one launch: the one-sided stride-2 convolution above over N * T' frames, whose loader pools the frame pairs (CV_POOL_DOWN)
int32_t vgpa_vae_downsample_f32(const float* x, const float* w_packed, const float* bias, float* out, int64_t N, int64_t T, int64_t H, int64_t W,
                                int64_t C, int64_t Cout, int32_t compress_time, hipStream_t stream) {
    ConvArgs a = {};
    if (frames_args(a, x, w_packed, bias, out, N, T, H, W, C, Cout, 2, 1 << 30) != VGPA_OK || (compress_time != 0 && compress_time != 1)) return VGPA_ERR_INVALID;
    if (!compress_time || T == 1)                                          // nothing to pool: the frames are samples of the 2-D convolution
        return conv_entry<CV_CONV_CHUNKED>(x, w_packed, bias, nullptr, nullptr, out, N * T, H, W, C, Cout, 3, 2, 0, 1, 0, stream);
    a.Tin = (int)T; a.T = (int)((T + 1) / 2);
    a.N = (int)(N * a.T); a.stride = 2; a.pad = 0;
    a.Ho = (int)((H + 1 - 3) / 2 + 1);                                     // one zero row / column behind the last, none in front
    a.Wo = (int)((W + 1 - 3) / 2 + 1);
    a.M = (int64_t)a.N * a.Ho * a.Wo;
    return conv_launch<CV_POOL_DOWN>(a, stream);
}

// CogVideoXUpsample3D in one launch: the 3x3 padding-1 convolution over N * T' frames of 2H x 2W whose loader reads the source at half the index (CV_UP2X)
int32_t vgpa_vae_upsample_f32(const float* x, const float* w_packed, const float* bias, float* out, int64_t N, int64_t T, int64_t H, int64_t W,
                              int64_t C, int64_t Cout, int32_t compress_time, hipStream_t stream) {
    ConvArgs a = {};
    if (frames_args(a, x, w_packed, bias, out, N, T, H, W, C, Cout, 1, 1 << 29) != VGPA_OK || (compress_time != 0 && compress_time != 1)) return VGPA_ERR_INVALID;
    a.Tin = (int)T;
    a.T = (int)(!compress_time || T == 1 ? T : (T & 1) ? 2 * T - 1 : 2 * T);   // an odd count keeps frame 0 single
    a.N = (int)(N * a.T); a.Ho = (int)(2 * H); a.Wo = (int)(2 * W); a.stride = 1; a.pad = 1;
    a.M = (int64_t)a.N * a.Ho * a.Wo;
    return conv_launch<CV_UP2X>(a, stream);
}

}  // extern "C"
