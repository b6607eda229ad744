// What Depth Anything 3's DINOv2 backbone does between its blocks (depth_anything_3/model/dinov2/vision_transformer.py:300-398,
// reference_view_selector.py:29-222) and behind its camera decoder (model/utils/transform.py:41-65, utils/geometry.py:55-59), forward only, fp32:
//   ref_view     class tokens -> three metrics per view, the selection score and the reference view of every batch element, as a DEVICE int32 [B]
//   view_gather  views reordered to [ref, 0, .., ref-1, ref+1, ..] (or back), whole [N][C] slabs, one or two tensors per launch
//   cam_token    token 0 of every view <- the camera token (ref / src rule, or one row per view from the caller)
//   tap          one out layer: features [B,S,N-1,2C] = [local | LayerNorm(x)], camera token [B,S,2C] = [local | x] of token 0, the original view order
//                restored through the row's source index -- instead of cat, norm, slice and gather passes over [B,S,N,2C]
//   pose_decode  pose encoding [M,9] -> world-to-camera [M,3,4] and intrinsics [M,3,3]
// Every kernel after ref_view takes the index buffer as an argument: the selection never reaches the host.  All of them are HBM- or latency-bound row
// kernels (csrc/dino_stream.hip is the model): coalesced 16-byte accesses, wave-level reductions in a fixed order, no atomics.
#include "common.h"

#define DA3_THREADS 256
#define DA3_MAX_VIEWS 64

// position j of the reordered sequence holds view order(ref, j); restored view t comes from position inverse(ref, t)
__device__ __forceinline__ int da3_order(int ref, int j) { return j == 0 ? ref : (j <= ref ? j - 1 : j); }
__device__ __forceinline__ int da3_inverse(int ref, int t) { return t == ref ? 0 : (t < ref ? t + 1 : t); }
__device__ __forceinline__ int da3_ref_of(const int32_t* ref_idx, int b, int S) { return min(max(ref_idx[b], 0), S - 1); }

// ---------------------------------------------------------------------------------------------- reference-view selection
// One workgroup per batch element.  The S class tokens (S * C floats, L2-resident after the first pass) are reduced in fp64: the min-max normalisation
// behind the metrics divides by their spread over the views, so the choice between two views amplifies rounding; in fp64 the kernel's own arithmetic adds
// nothing to what the tokens carry.  Each wave owns whole dot products (lanes stride C, butterfly sum): the S x S Gram matrix lands in LDS.
__global__ __launch_bounds__(DA3_THREADS) void da3_ref_view_kernel(const float* __restrict__ x, int S, int64_t view_stride, int C, int strategy,
                                                                   double* __restrict__ metrics, int32_t* __restrict__ ref_idx) {
    __shared__ double gram[DA3_MAX_VIEWS][DA3_MAX_VIEWS + 1];
    __shared__ double m_sim[DA3_MAX_VIEWS], m_norm[DA3_MAX_VIEWS], m_var[DA3_MAX_VIEWS], m_score[DA3_MAX_VIEWS];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = DA3_THREADS >> 6;
    const float* xb = x + (size_t)b * S * view_stride;
    for (int s = wid; s < S; s += nw) {                        // norm and the variance of the normalised token
        const float* t = xb + (size_t)s * view_stride;
        double sum = 0.0, sq = 0.0;
        for (int c = lane; c < C; c += 64) { const double v = t[c]; sum += v; sq += v * v; }
        sum = wave_sum(sum); sq = wave_sum(sq);
        const double mean = sum / C;
        double dev = 0.0;
        for (int c = lane; c < C; c += 64) { const double d = (double)t[c] - mean; dev += d * d; }
        dev = wave_sum(dev);
        if (lane == 0) {
            gram[s][s] = sq;
            m_norm[s] = sqrt(sq);
            m_var[s] = C > 1 ? dev / sq / (double)(C - 1) : 0.0;      // var(x / |x|), unbiased as torch.var
        }
    }
    for (int p = wid; p < S * S; p += nw) {                    // the pairs i < j
        const int i = p / S, j = p % S;
        if (i >= j) continue;
        const float *ti = xb + (size_t)i * view_stride, *tj = xb + (size_t)j * view_stride;
        double dot = 0.0;
        for (int c = lane; c < C; c += 64) dot += (double)ti[c] * (double)tj[c];
        dot = wave_sum(dot);
        if (lane == 0) { gram[i][j] = dot; gram[j][i] = dot; }
    }
    __syncthreads();
    const int s = threadIdx.x;
    double range = 0.0;
    if (s < S) {                                               // cosine similarities without the diagonal's 1: mean over the other views, and the row's range
        double sum = 0.0, mx = 0.0, mn = 0.0;
        for (int j = 0; j < S; ++j) {
            const double v = gram[s][j] / (m_norm[s] * m_norm[j]) - (j == s ? 1.0 : 0.0);
            sum += v;
            mx = j == 0 ? v : fmax(mx, v);
            mn = j == 0 ? v : fmin(mn, v);
        }
        m_sim[s] = S > 1 ? sum / (double)(S - 1) : 0.0;
        range = mx - mn;
    }
    __syncthreads();
    if (s < S) {
        double score = 0.0;
        const double* ms[3] = {m_sim, m_norm, m_var};
        for (int k = 0; k < 3; ++k) {
            double mn = ms[k][0], mx = ms[k][0];
            for (int j = 1; j < S; ++j) { mn = fmin(mn, ms[k][j]); mx = fmax(mx, ms[k][j]); }
            score += fabs((ms[k][s] - mn) / (mx - mn + 1e-8) - 0.5);
        }
        m_score[s] = strategy == 3 ? range : score;
        if (metrics) {
            double* o = metrics + ((size_t)b * S + s) * 4;
            o[0] = m_sim[s]; o[1] = m_norm[s]; o[2] = m_var[s]; o[3] = m_score[s];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0;
        if (strategy == 1) best = S / 2;
        else if (strategy >= 2 && S > 1) {                      // argmin of the balance score | argmax of the range; a tie keeps the lowest index
            for (int j = 1; j < S; ++j)
                if (strategy == 2 ? m_score[j] < m_score[best] : m_score[j] > m_score[best]) best = j;
        }
        ref_idx[b] = S > 1 ? best : 0;
    }
}

// ---------------------------------------------------------------------------------------------- view gather / restore
// grid (chunks of a slab, B * S, tensors); a slab is L floats, L a multiple of 4
__global__ __launch_bounds__(DA3_THREADS) void da3_view_gather_kernel(const float* __restrict__ a_in, float* __restrict__ a_out, const float* __restrict__ b_in,
                                                                      float* __restrict__ b_out, const int32_t* __restrict__ ref_idx, int inverse, int S,
                                                                      int64_t L4) {
    const int bs = blockIdx.y, b = bs / S, j = bs % S;
    const int ref = da3_ref_of(ref_idx, b, S);
    const int src = inverse ? da3_inverse(ref, j) : da3_order(ref, j);
    const float4* in = reinterpret_cast<const float4*>(blockIdx.z ? b_in : a_in) + ((size_t)b * S + src) * L4;
    float4* out = reinterpret_cast<float4*>(blockIdx.z ? b_out : a_out) + (size_t)bs * L4;
    for (int64_t i = (int64_t)blockIdx.x * DA3_THREADS + threadIdx.x; i < L4; i += (int64_t)gridDim.x * DA3_THREADS) out[i] = in[i];
}

// ---------------------------------------------------------------------------------------------- camera token
// one workgroup per view: x[b, s, 0, :] = per_view ? cam[b, s, :] : camera_token[s == 0 ? 0 : 1, :]
__global__ __launch_bounds__(DA3_THREADS) void da3_cam_token_kernel(float* __restrict__ x, const float* __restrict__ cam, int per_view, int S, int64_t view_stride,
                                                                    int C) {
    const int bs = blockIdx.x, s = bs % S;
    const float* src = cam + (size_t)(per_view ? bs : (s == 0 ? 0 : 1)) * C;
    float* dst = x + (size_t)bs * view_stride;
    for (int c = threadIdx.x; c < C; c += DA3_THREADS) dst[c] = src[c];
}

// ---------------------------------------------------------------------------------------------- tap
// one workgroup per output token row (b, view, n); C a multiple of 4
__global__ __launch_bounds__(DA3_THREADS) void da3_tap_kernel(const float* __restrict__ local_x, const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float eps, const int32_t* __restrict__ ref_idx, int S, int N, int C,
                                                              float* __restrict__ feats, float* __restrict__ cam) {
    __shared__ float red[16];
    const int n = blockIdx.x % N, bs = blockIdx.x / N, b = bs / S, t = bs % S;
    const int src_view = ref_idx ? da3_inverse(da3_ref_of(ref_idx, b, S), t) : t;
    const size_t src = (((size_t)b * S + src_view) * N + n) * C;
    const int C4 = C >> 2;
    const float4* lp = reinterpret_cast<const float4*>(local_x + src);
    const float4* xp = reinterpret_cast<const float4*>(x + src);
    float* dst = n == 0 ? cam + (size_t)bs * 2 * C : feats + ((size_t)bs * (N - 1) + (n - 1)) * 2 * C;
    float4* d_local = reinterpret_cast<float4*>(dst);
    float4* d_x = reinterpret_cast<float4*>(dst + C);
    for (int c = threadIdx.x; c < C4; c += DA3_THREADS) d_local[c] = lp[c];
    if (n == 0) {                                              // the camera token leaves un-normalised (the whole workgroup takes this branch)
        for (int c = threadIdx.x; c < C4; c += DA3_THREADS) d_x[c] = xp[c];
        return;
    }
    float s = 0.f;
    for (int c = threadIdx.x; c < C4; c += DA3_THREADS) { const float4 v = xp[c]; s += (v.x + v.y) + (v.z + v.w); }
    const float mean = block_sum(s, red) / (float)C;
    float q = 0.f;
    for (int c = threadIdx.x; c < C4; c += DA3_THREADS) {
        const float4 v = xp[c];
        const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
        q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    }
    const float rstd = rsqrtf(block_sum(q, red) / (float)C + eps);
    const float4* wp = reinterpret_cast<const float4*>(w);
    const float4* bp = reinterpret_cast<const float4*>(bias);
    for (int c = threadIdx.x; c < C4; c += DA3_THREADS) {
        const float4 v = xp[c], ww = wp[c], bb = bp[c];
        d_x[c] = make_float4((v.x - mean) * rstd * ww.x + bb.x, (v.y - mean) * rstd * ww.y + bb.y, (v.z - mean) * rstd * ww.z + bb.z,
                             (v.w - mean) * rstd * ww.w + bb.w);
    }
}

// ---------------------------------------------------------------------------------------------- pose encoding -> world-to-camera, intrinsics
// [R | T] of the encoding is camera-to-world (scalar-last quaternion, csrc/scorer2.hip has the same matrix); its inverse is [R^T | -R^T T].  One thread per
// camera and a handful of cameras per call: the arithmetic is fp64 (free at this size), so every output is the fp32 rounding of the exact value.
__global__ void da3_pose_decode_kernel(const float* __restrict__ pe, int64_t n, double img_h, double img_w, float* __restrict__ ext, float* __restrict__ intr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = pe + i * 9;
    const double qi = p[3], qj = p[4], qk = p[5], qr = p[6], t0 = p[0], t1 = p[1], t2 = p[2];
    const double two_s = 2.0 / (((qi * qi + qj * qj) + qk * qk) + qr * qr);
    double R[9];
    R[0] = 1.0 - two_s * (qj * qj + qk * qk); R[1] = two_s * (qi * qj - qk * qr); R[2] = two_s * (qi * qk + qj * qr);
    R[3] = two_s * (qi * qj + qk * qr); R[4] = 1.0 - two_s * (qi * qi + qk * qk); R[5] = two_s * (qj * qk - qi * qr);
    R[6] = two_s * (qi * qk - qj * qr); R[7] = two_s * (qj * qk + qi * qr); R[8] = 1.0 - two_s * (qi * qi + qj * qj);
    float* e = ext + i * 12;
    for (int r = 0; r < 3; ++r) {
        e[r * 4] = (float)R[r]; e[r * 4 + 1] = (float)R[3 + r]; e[r * 4 + 2] = (float)R[6 + r];
        e[r * 4 + 3] = (float)(-((R[r] * t0 + R[3 + r] * t1) + R[6 + r] * t2));
    }
    float* k = intr + i * 9;
    for (int r = 0; r < 9; ++r) k[r] = 0.f;
    k[4] = (float)((img_h / 2.0) / fmax(tan((double)p[7] / 2.0), 1e-6));
    k[0] = (float)((img_w / 2.0) / fmax(tan((double)p[8] / 2.0), 1e-6));
    k[2] = (float)(img_w / 2.0);
    k[5] = (float)(img_h / 2.0);
    k[8] = 1.0f;
}

static bool da3_shape_ok(int64_t B, int64_t S, int64_t N, int64_t C) {
    return B > 0 && S > 0 && N > 0 && C > 0 && C <= (1 << 20) && N <= (1 << 24) && B * S <= 0x7fffffffLL / N && B * S <= 65535;
}
static bool da3_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

extern "C" {

int32_t vgpa_da3_ref_view(const float* x, int64_t B, int64_t S, int64_t N, int64_t C, int32_t strategy, double* metrics, int32_t* ref_idx,
                          hipStream_t stream) {
    if (!x || !ref_idx || !da3_shape_ok(B, S, N, C) || S > DA3_MAX_VIEWS || strategy < 0 || strategy > 3) return VGPA_ERR_INVALID;
    VGPA_LAUNCH(da3_ref_view_kernel, dim3((unsigned)B), dim3(DA3_THREADS), 0, stream, x, (int)S, N * C, (int)C, (int)strategy, metrics, ref_idx);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_da3_view_gather(const float* a_in, float* a_out, const float* b_in, float* b_out, const int32_t* ref_idx, int32_t inverse, int64_t B,
                             int64_t S, int64_t N, int64_t C, hipStream_t stream) {
    if (!a_in || !a_out || !ref_idx || (b_in != nullptr) != (b_out != nullptr) || !da3_shape_ok(B, S, N, C) || (N * C) % 4) return VGPA_ERR_INVALID;
    if (a_in == a_out || (b_in && (b_in == b_out || b_out == a_out || b_out == a_in || a_out == b_in))) return VGPA_ERR_INVALID;     // never in place
    if (!da3_aligned16(a_in) || !da3_aligned16(a_out) || !da3_aligned16(b_in) || !da3_aligned16(b_out)) return VGPA_ERR_INVALID;
    const int64_t L4 = N * C / 4;
    const unsigned chunks = (unsigned)((L4 + DA3_THREADS * 4 - 1) / (DA3_THREADS * 4) < 1024 ? (L4 + DA3_THREADS * 4 - 1) / (DA3_THREADS * 4) : 1024);
    VGPA_LAUNCH(da3_view_gather_kernel, dim3(chunks, (unsigned)(B * S), b_in ? 2 : 1), dim3(DA3_THREADS), 0, stream, a_in, a_out, b_in, b_out, ref_idx,
                (int)(inverse != 0), (int)S, L4);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_da3_cam_token(float* x, const float* cam, int32_t per_view, int64_t B, int64_t S, int64_t N, int64_t C, hipStream_t stream) {
    if (!x || !cam || !da3_shape_ok(B, S, N, C)) return VGPA_ERR_INVALID;
    VGPA_LAUNCH(da3_cam_token_kernel, dim3((unsigned)(B * S)), dim3(DA3_THREADS), 0, stream, x, cam, (int)(per_view != 0), (int)S, N * C, (int)C);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_da3_tap(const float* local_x, const float* x, const float* ln_w, const float* ln_b, float eps, const int32_t* ref_idx, float* feats,
                     float* cam, int64_t B, int64_t S, int64_t N, int64_t C, hipStream_t stream) {
    if (!local_x || !x || !ln_w || !ln_b || !cam || !da3_shape_ok(B, S, N, C) || C % 4 || (N > 1 && !feats)) return VGPA_ERR_INVALID;
    if (!da3_aligned16(local_x) || !da3_aligned16(x) || !da3_aligned16(ln_w) || !da3_aligned16(ln_b) || !da3_aligned16(feats) || !da3_aligned16(cam))
        return VGPA_ERR_INVALID;
    VGPA_LAUNCH(da3_tap_kernel, dim3((unsigned)(B * S * N)), dim3(DA3_THREADS), 0, stream, local_x, x, ln_w, ln_b, eps, ref_idx, (int)S, (int)N, (int)C, feats,
                cam);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_da3_pose_decode(const float* pose_enc, int64_t n, float image_h, float image_w, float* ext, float* intr, hipStream_t stream) {
    if (!pose_enc || !ext || !intr || n <= 0 || n > 0x7fffffffLL * 64) return VGPA_ERR_INVALID;
    VGPA_LAUNCH(da3_pose_decode_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, pose_enc, n, (double)image_h, (double)image_w, ext, intr);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

}  // extern "C"
