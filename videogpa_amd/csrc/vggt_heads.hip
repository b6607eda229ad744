// VGGT prediction heads (vggt/heads/dpt_head.py, camera_head.py), the part that is not torch plumbing.  Everything fp32 in, fp32 out,
// channels-last (NHWC), forward only:
//   conv_kernel<.., TAIL = false>   3x3 (stride 1 | 2, pad 1) or 1x1 convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32:
//                                   a k-ordered fmaf chain, only the summation order differs from torch's conv2d), with the fused pieces a
//                                   ResidualConvUnit / FeatureFusionBlock needs: out = conv(relu?(x)) + bias? + relu?(res)? + res2?
//   conv_kernel<.., TAIL = true>    the end of DPTHead._forward_impl (dpt_head.py:229-247) in one launch on the same core: the loader samples the
//                                   [N,h,w,C] map bilinearly (align_corners=True) at the (H,W) grid and adds the 0.1-scaled UV positional
//                                   embedding from two separable tables; the epilogue is bias + ReLU, the 1x1 conv 32 -> output_dim, activate_head.
//                                   The [N,H,W,C] tensor never exists.
//   upsample_kernel                 NHWC align_corners=True bilinear resize (+ the same separable embedding)
//   attn_small_kernel               fp32 softmax attention of the camera trunk, S <= 128 tokens, one workgroup per (batch, head)
//
// GEMM view of the convolution: M = N * Ho * Wo output pixels (flat, so H and W are arbitrary), N = Cout, K = taps * Cin walked tap-major in
// chunks of 16 channels.  A workgroup (4 waves) owns 128 pixels x BN channels; every thread owns ONE pixel of the A tile for the whole K loop
// (its (n, y, x) is decoded once) and fetches 2 x 16 bytes of it per chunk, the next chunk's global loads are in flight while the MFMAs of
// the current one run from LDS.  Both LDS tiles are k-major with a row stride = 32 (mod 64) dwords: lane l reads [k = l >> 5][l & 31], so
// the two k rows of one ds_read fall into disjoint bank halves.
#include "common.h"

#define CV_THREADS 256
#define CV_BM 128
#define CV_KC 16
#define CV_AS (CV_BM + 32)
#define CV_RELU_IN 1
#define CV_RELU_RES 2

struct ConvArgs {
    const float* x;      // [N,H,W,Cin]  (TAIL: the low-resolution map [N,h,w,Cin])
    const float* w;      // [taps][Cin][Cout]
    const float* bias;   // [Cout] | NULL
    const float* res;    // [N,Ho,Wo,Cout] | NULL
    const float* res2;   // [N,Ho,Wo,Cout] | NULL
    float* out;          // [N,Ho,Wo,Cout]
    int N, H, W, Ho, Wo, Cin, Cout, ksize, stride, flags;
    int64_t M;
    // TAIL only
    const float* xtab;   // [Wo, Cin/2] | NULL
    const float* ytab;   // [Ho, Cin/2] | NULL
    const float* w2;     // [od][32]
    const float* b2;     // [od]
    float* preds;        // [N,Ho,Wo,od-1]
    float* conf;         // [N,Ho,Wo]
    int od, act;         // act 0: exp, 1: inv_log
    float sy, sx;        // (h-1)/(Ho-1), (w-1)/(Wo-1)
};

__device__ __forceinline__ float4 f4_fma(float s, float4 a, float4 acc) {
    return make_float4(s * a.x + acc.x, s * a.y + acc.y, s * a.z + acc.z, s * a.w + acc.w);
}
__device__ __forceinline__ float4 f4_scale(float s, float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
__device__ __forceinline__ float4 f4_relu(float4 a) { return make_float4(fmaxf(a.x, 0.f), fmaxf(a.y, 0.f), fmaxf(a.z, 0.f), fmaxf(a.w, 0.f)); }

// torch's upsample_bilinear2d, align_corners=True: src = dst * (in - 1) / (out - 1); i1 = i0 + (i0 < in - 1); weights (1 - l, l)
struct Lerp {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Lerp lerp_of(int dst, float scale, int in) {
    const float src = scale * (float)dst;
    int i0 = (int)src;
    i0 = i0 > in - 1 ? in - 1 : i0;
    Lerp r;
    r.i0 = i0;
    r.i1 = i0 + (i0 < in - 1 ? 1 : 0);
    r.l1 = src - (float)i0;
    r.l0 = 1.0f - r.l1;
    return r;
}
// four channels of the interpolated (+ embedded) map at output pixel (oy, ox); base = frame n of the [h,w,C] source
__device__ __forceinline__ float4 sample4(const float* __restrict__ base, int h, int w, int C, float sy, float sx, int oy, int ox, int c,
                                          const float* __restrict__ xtab, const float* __restrict__ ytab) {
    const Lerp ly = lerp_of(oy, sy, h), lx = lerp_of(ox, sx, w);
    const float* r0 = base + (size_t)ly.i0 * w * C + c;
    const float* r1 = base + (size_t)ly.i1 * w * C + c;
    const float4 v00 = *reinterpret_cast<const float4*>(r0 + (size_t)lx.i0 * C), v01 = *reinterpret_cast<const float4*>(r0 + (size_t)lx.i1 * C);
    const float4 v10 = *reinterpret_cast<const float4*>(r1 + (size_t)lx.i0 * C), v11 = *reinterpret_cast<const float4*>(r1 + (size_t)lx.i1 * C);
    const float4 top = f4_fma(lx.l0, v00, f4_scale(lx.l1, v01)), bot = f4_fma(lx.l0, v10, f4_scale(lx.l1, v11));
    float4 v = f4_fma(ly.l0, top, f4_scale(ly.l1, bot));
    if (xtab) {
        const int half = C >> 1;
        const float4 e = c < half ? *reinterpret_cast<const float4*>(xtab + (size_t)ox * half + c)
                                  : *reinterpret_cast<const float4*>(ytab + (size_t)oy * half + (c - half));
        v = make_float4(v.x + e.x, v.y + e.y, v.z + e.z, v.w + e.w);
    }
    return v;
}

template <int WM, int WN, int TM, int TN, bool TAIL>
__global__ __launch_bounds__(CV_THREADS) void conv_kernel(const ConvArgs a) {
    constexpr int BN = WN * TN * 32;
    constexpr int BS = (BN % 64 == 0) ? BN + 32 : BN + 64;
    constexpr int NB = (CV_KC * BN / 4 + CV_THREADS - 1) / CV_THREADS;      // float4 of the weight tile per thread
    static_assert(WM * WN == 4 && WM * TM * 32 == CV_BM, "4 waves, 128 pixels");
    static_assert(!TAIL || BN == 32, "the tail's hidden width is 32");
    constexpr int LDS_AB = CV_KC * CV_AS + CV_KC * BS;
    constexpr int LDS_N = TAIL ? (LDS_AB > CV_BM * 33 ? LDS_AB : CV_BM * 33) : LDS_AB;
    __shared__ __attribute__((aligned(16))) float lds[LDS_N];
    float* As = lds;
    float* Bs = lds + CV_KC * CV_AS;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int64_t p0 = (int64_t)blockIdx.x * CV_BM;
    const int n0 = blockIdx.y * BN;

    // this thread's pixel of the A tile
    const int pl = tid & (CV_BM - 1), jq = tid >> 7;                         // float4 slots jq and jq + 2 of the 16-channel chunk
    const int64_t p = p0 + pl;
    const bool pvalid = p < a.M;
    int pn = 0, py = 0, px = 0;
    if (pvalid) {
        px = (int)(p % a.Wo);
        py = (int)((p / a.Wo) % a.Ho);
        pn = (int)(p / ((int64_t)a.Wo * a.Ho));
    }
    const float* xn = a.x + (size_t)pn * a.H * a.W * a.Cin;
    const int pad = a.ksize >> 1;
    const int cchunks = a.Cin / CV_KC, iters = a.ksize * a.ksize * cchunks;

    float4 ra[2], rb[NB];
    auto fetch = [&](int it) {
        const int tap = it / cchunks, c0 = (it - tap * cchunks) * CV_KC;
        const int dy = tap / a.ksize - pad, dx = tap % a.ksize - pad;
        if constexpr (TAIL) {
            const int iy = py + dy, ix = px + dx;
            const bool in = pvalid && iy >= 0 && iy < a.Ho && ix >= 0 && ix < a.Wo;
#pragma unroll
            for (int i = 0; i < 2; ++i)
                ra[i] = in ? sample4(xn, a.H, a.W, a.Cin, a.sy, a.sx, iy, ix, c0 + 4 * (jq + 2 * i), a.xtab, a.ytab) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            const int iy = py * a.stride + dy, ix = px * a.stride + dx;
            const bool in = pvalid && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const float* src = xn + ((size_t)iy * a.W + ix) * a.Cin + c0;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float4 v = in ? *reinterpret_cast<const float4*>(src + 4 * (jq + 2 * i)) : make_float4(0.f, 0.f, 0.f, 0.f);
                ra[i] = (a.flags & CV_RELU_IN) ? f4_relu(v) : v;
            }
        }
        const float* wk = a.w + ((size_t)tap * a.Cin + c0) * a.Cout;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + i * CV_THREADS, row = idx / (BN / 4), col = (idx % (BN / 4)) * 4;
            const bool in = idx < CV_KC * BN / 4 && n0 + col < a.Cout;          // Cout is a multiple of 16: a float4 is inside or outside as a whole
            rb[i] = in ? *reinterpret_cast<const float4*>(wk + (size_t)row * a.Cout + n0 + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float* d = As + (4 * (jq + 2 * i)) * CV_AS + pl;
            d[0] = ra[i].x;
            d[CV_AS] = ra[i].y;
            d[2 * CV_AS] = ra[i].z;
            d[3 * CV_AS] = ra[i].w;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + i * CV_THREADS, row = idx / (BN / 4), col = (idx % (BN / 4)) * 4;
            if (idx < CV_KC * BN / 4) *reinterpret_cast<float4*>(Bs + row * BS + col) = rb[i];
        }
    };

    f32x16_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    fetch(0);
    stash();
    __syncthreads();
    const int l31 = lane & 31, lh = lane >> 5;
    for (int it = 0; it < iters; ++it) {
        if (it + 1 < iters) fetch(it + 1);
#pragma unroll
        for (int ks = 0; ks < CV_KC / 2; ++ks) {
            const int k = 2 * ks + lh;
            float fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = As[k * CV_AS + (wm * TM + i) * 32 + l31];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = Bs[k * BS + (wn * TN + j) * 32 + l31];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (it + 1 < iters) {
            stash();
            __syncthreads();
        }
    }

    // accumulator element r of lane l: channel column l & 31, pixel row (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)
    if constexpr (!TAIL) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int co = n0 + (wn * TN + j) * 32 + l31;
            if (co >= a.Cout) continue;
            const float bv = a.bias ? a.bias[co] : 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t q = p0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (q >= a.M) continue;
                    const size_t o = (size_t)q * a.Cout + co;
                    float v = acc[i][j][r] + bv;
                    if (a.res) {
                        const float rv = a.res[o];
                        v += (a.flags & CV_RELU_RES) ? fmaxf(rv, 0.f) : rv;
                    }
                    if (a.res2) v += a.res2[o];
                    a.out[o] = v;
                }
            }
        }
    } else {
        // hidden = relu(conv + b1) -> LDS [pixel][33]; then one thread per pixel: the 1x1 conv 32 -> od and activate_head
        float* Hs = lds;
        const float bv = a.bias[l31];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            Hs[row * 33 + l31] = fmaxf(acc[0][0][r] + bv, 0.f);
        }
        __syncthreads();
        if (tid < CV_BM && p0 + tid < a.M) {
            const int64_t q = p0 + tid;
            for (int o = 0; o < a.od; ++o) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < 32; ++c) s = fmaf(a.w2[o * 32 + c], Hs[tid * 33 + c], s);
                s += a.b2[o];
                if (o == a.od - 1) a.conf[q] = 1.0f + expf(s);
                else a.preds[(size_t)q * (a.od - 1) + o] = a.act == 0 ? expf(s) : copysignf(expm1f(fabsf(s)), s);
            }
        }
    }
}

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

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool TAIL>
static int32_t conv_launch(const ConvArgs& a, hipStream_t stream) {
    const int64_t mb = (a.M + CV_BM - 1) / CV_BM;
    if (mb <= 0 || mb > 0x7fffffffLL) return VGPA_ERR_INVALID;
    if constexpr (TAIL) {
        VGPA_LAUNCH((conv_kernel<4, 1, 1, 1, true>), dim3((unsigned)mb, 1), dim3(CV_THREADS), 0, stream, a);
    } else if (a.Cout >= 128) {
        VGPA_LAUNCH((conv_kernel<2, 2, 2, 2, false>), dim3((unsigned)mb, (unsigned)((a.Cout + 127) / 128)), dim3(CV_THREADS), 0, stream, a);
    } else if (a.Cout > 32) {
        VGPA_LAUNCH((conv_kernel<2, 2, 2, 1, false>), dim3((unsigned)mb, (unsigned)((a.Cout + 63) / 64)), dim3(CV_THREADS), 0, stream, a);
    } else {
        VGPA_LAUNCH((conv_kernel<4, 1, 1, 1, false>), dim3((unsigned)mb, 1), dim3(CV_THREADS), 0, stream, a);
    }
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

static int32_t conv_entry(const float* x, const float* w, const float* bias, const float* res, const float* res2, float* out, int64_t N, int64_t H,
                          int64_t W, int64_t Cin, int64_t Cout, int ksize, int64_t stride, int32_t flags, hipStream_t stream) {
    if (!x || !w || !out || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 15) || (Cout & 15)) return VGPA_ERR_INVALID;
    if ((stride != 1 && stride != 2) || (flags & ~(CV_RELU_IN | CV_RELU_RES)) || H > (1 << 30) || W > (1 << 30) || Cin > (1 << 20) || Cout > (1 << 20))
        return VGPA_ERR_INVALID;
    if (!aligned16(x) || !aligned16(w)) return VGPA_ERR_INVALID;
    ConvArgs a = {};
    a.x = x; a.w = w; a.bias = bias; a.res = res; a.res2 = res2; a.out = out;
    a.N = (int)N; a.H = (int)H; a.W = (int)W; a.Cin = (int)Cin; a.Cout = (int)Cout; a.ksize = ksize; a.stride = (int)stride; a.flags = flags;
    a.Ho = ksize == 3 ? (int)((H - 1) / stride + 1) : (int)H;
    a.Wo = ksize == 3 ? (int)((W - 1) / stride + 1) : (int)W;
    a.M = N * a.Ho * a.Wo;
    return conv_launch<false>(a, stream);
}

extern "C" {

int32_t vgpa_conv3x3_f32(const float* x, const float* w_packed, const float* bias, const float* res, const float* res2, float* out, int64_t N,
                         int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t stride, int32_t flags, hipStream_t stream) {
    return conv_entry(x, w_packed, bias, res, res2, out, N, H, W, Cin, Cout, 3, stride, flags, stream);
}

int32_t vgpa_conv1x1_f32(const float* x, const float* w_packed, const float* bias, float* out, int64_t M, int64_t Cin, int64_t Cout,
                         hipStream_t stream) {
    return conv_entry(x, w_packed, bias, nullptr, nullptr, out, 1, 1, M, Cin, Cout, 1, 1, 0, stream);
}

int32_t vgpa_dpt_tail_f32(const float* x, const float* xtab, const float* ytab, const float* w1_packed, const float* b1, const float* w2,
                          const float* b2, float* preds, float* conf, int64_t N, int64_t h, int64_t w, int64_t C, int64_t H, int64_t W,
                          int32_t output_dim, int32_t activation, hipStream_t stream) {
    if (!x || !w1_packed || !b1 || !w2 || !b2 || !preds || !conf || N <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 15))
        return VGPA_ERR_INVALID;
    if ((xtab == nullptr) != (ytab == nullptr) || output_dim < 2 || output_dim > 8 || (activation != 0 && activation != 1)) return VGPA_ERR_INVALID;
    if (h > (1 << 20) || w > (1 << 20) || H > (1 << 20) || W > (1 << 20) || C > (1 << 20)) return VGPA_ERR_INVALID;
    if (!aligned16(x) || !aligned16(w1_packed) || !aligned16(xtab) || !aligned16(ytab)) return VGPA_ERR_INVALID;
    ConvArgs a = {};
    a.x = x; a.w = w1_packed; a.bias = b1; a.xtab = xtab; a.ytab = ytab; a.w2 = w2; a.b2 = b2; a.preds = preds; a.conf = conf;
    a.N = (int)N; a.H = (int)h; a.W = (int)w; a.Ho = (int)H; a.Wo = (int)W; a.Cin = (int)C; a.Cout = 32; a.ksize = 3; a.stride = 1;
    a.od = output_dim; a.act = activation;
    a.sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    a.sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    a.M = N * H * W;
    return conv_launch<true>(a, stream);
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
