// The exact-fp32 MFMA convolution core: conv_kernel<.., MODE>, its launcher and the argument checks the entry points share.  Instantiated by
// csrc/vggt_heads.hip (CV_CONV, CV_TAIL), csrc/dualdpt.hip (CV_AUX_TAIL) and csrc/vae_conv.hip (the four chunked modes of the CogVideoX VAE).
//   CV_CONV      3x3 (stride 1 | 2; pad 1, or one-sided: ConvArgs.pad) or 1x1 convolution with the fused ReLU / bias / residual adds
//   CV_CONV_CHUNKED  the same convolution with its K sum cut into runs of CV_CHUNK_ITERS * 16 products: every run starts from zero and is added to a
//                second accumulator when it ends.  One chain of n fp32 additions carries a rounding error that grows like sqrt(n) times the size of the
//                partial sums; n / T short chains plus one chain over their n / T results grow like sqrt(T + n / T) instead -- at the VAE encoder's
//                9 * 512 products a sixth of the single chain's error, for one vector add per accumulator register every CV_CHUNK_ITERS iterations
//   CV_CONV3D    the causal 3x3x3 convolution of the CogVideoX VAE encoder over frames (vgpa_conv3x3x3_causal_f32): x [N,T,H,W,Cin], flat
//                M = N * T * H * W, the pixel decoded once to (n, t, y, x), K = 27 * Cin walked tap-major (kt, ky, kx) with the K sum in the runs of
//                CV_CONV_CHUNKED.  Temporal tap kt of output frame t reads frame t + kt - 2; a frame in front of frame 0 comes from
//                ConvArgs.prev [N,2,H,W,Cin] (the last two frames of the chunk before) or, without one, is frame 0 again.  Only the loader's
//                source address depends on N, T and prev: an output sums the same products in the same order wherever its frames lie
//   CV_POOL_DOWN CogVideoXDownsample3D with its temporal pooling (vgpa_vae_downsample_f32): CV_CONV_CHUNKED on [N * T',H,W,C] whose loader reads
//                frame t' as (a + b) * 0.5 of two frames of x [N,Tin,H,W,C] (or one frame as it is), so the pooled tensor is never written
//   CV_UP2X      CogVideoXUpsample3D (vgpa_vae_upsample_f32): CV_CONV_CHUNKED, 3x3 with padding 1, over the nearest-neighbour x2 map of x
//                [N,Tin,H,W,C] that is never written: tap (y, x) of output frame t reads source pixel (y >> 1, x >> 1) of source frame f(t), zero
//                outside [0,2H) x [0,2W); f(t) = t (T = Tin), t >> 1 (T = 2 Tin) or 0, 1 + ((t - 1) >> 1) (T = 2 Tin - 1: frame 0 is not doubled)
//   CV_TAIL      the end of vggt's DPTHead: bilinear loader (+ embedding), epilogue bias + ReLU, 1x1 conv 32 -> od, activate_head
//   CV_AUX_TAIL  the end of DA3's auxiliary branch (dualdpt.py:250-258): the loader reads the map as it is (+ embedding, zero padding), the epilogue
//                is bias, LayerNorm over the 32 hidden channels of the pixel, ReLU, 1x1 conv 32 -> od, linear preds and conf = 1 + exp
//
// GEMM view of the convolution: M = N * Ho * Wo output pixels (flat, so H and W are arbitrary), N = Cout, K = taps * Cin walked tap-major in
// chunks of 16 channels.  A workgroup (4 waves) owns 128 pixels x BN channels; every thread owns ONE pixel of the A tile for the whole K loop
// (its (n, y, x) is decoded once) and fetches 2 x 16 bytes of it per chunk, the next chunk's global loads are in flight while the MFMAs of
// the current one run from LDS.  Both LDS tiles are k-major with a row stride = 32 (mod 64) dwords: lane l reads [k = l >> 5][l & 31], so
// the two k rows of one ds_read fall into disjoint bank halves.  Both tails reuse the tiles' LDS for their 128 x 32 hidden values, [pixel][33].
#pragma once
#include "common.h"

#define CV_CONV 0
#define CV_TAIL 1
#define CV_AUX_TAIL 2
#define CV_CONV_CHUNKED 3
#define CV_CONV3D 4
#define CV_POOL_DOWN 5
#define CV_UP2X 6
#define CV_CHUNK_ITERS 4
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
    int pad;             // zero padding in front of row / column 0 (ksize / 2 for the centred window); past the last one the bounds test pads as far as the window reaches
    int64_t M;
    // CV_TAIL and CV_AUX_TAIL only
    const float* xtab;   // [Wo, Cin/2] | NULL
    const float* ytab;   // [Ho, Cin/2] | NULL
    const float* w2;     // [od][32]
    const float* b2;     // [od]
    float* preds;        // [N,Ho,Wo,od-1]
    float* conf;         // [N,Ho,Wo]
    int od, act;         // act 0: exp, 1: inv_log
    float sy, sx;        // (h-1)/(Ho-1), (w-1)/(Wo-1)
    // CV_AUX_TAIL only
    const float* ln_w;   // [32]
    const float* ln_b;   // [32]
    float eps;
    // CV_CONV3D, CV_POOL_DOWN and CV_UP2X only
    const float* prev;   // CV_CONV3D: [N,2,H,W,Cin] | NULL
    int T;               // frames of the output
    int Tin;             // CV_POOL_DOWN: frames of x (T = (Tin + 1) / 2); CV_UP2X: frames of x (T = Tin, 2 Tin or 2 Tin - 1)
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
// v + the 0.1-scaled UV embedding of pixel (y, x), channels c .. c + 3: the x half from xtab [W][half], the y half from ytab [H][half], where
// half = C / 2 is a multiple of 4, so a float4 lies in one of the two
__device__ __forceinline__ float4 embed4(float4 v, const float* __restrict__ xtab, const float* __restrict__ ytab, int half, int y, int x, int c) {
    const float4 e = c < half ? *reinterpret_cast<const float4*>(xtab + (size_t)x * half + c)
                              : *reinterpret_cast<const float4*>(ytab + (size_t)y * half + (c - half));
    return make_float4(v.x + e.x, v.y + e.y, v.z + e.z, v.w + e.w);
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
    const float4 v = f4_fma(ly.l0, top, f4_scale(ly.l1, bot));
    return xtab ? embed4(v, xtab, ytab, C >> 1, oy, ox, c) : v;
}

template <int WM, int WN, int TM, int TN, int MODE>
__global__ __launch_bounds__(CV_THREADS) void conv_kernel(const ConvArgs a) {
    constexpr bool TAIL = MODE == CV_TAIL || MODE == CV_AUX_TAIL;                               // either tail: 32 hidden channels, the epilogue goes through LDS
    constexpr bool CHUNKED = MODE == CV_CONV_CHUNKED || MODE == CV_CONV3D || MODE == CV_POOL_DOWN || MODE == CV_UP2X;  // the K sum in runs of CV_CHUNK_ITERS iterations
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
    [[maybe_unused]] int pt = 0;                                            // CV_CONV3D: the output frame; pn above is then (n, t) in one
    [[maybe_unused]] const float* xb = nullptr;                             // CV_POOL_DOWN: the second frame of the pooled pair (== xn: one frame as it is)
    if constexpr (MODE == CV_CONV3D) {
        pt = pn % a.T;
        pn /= a.T;
    }
    const float* xn = a.x + (size_t)pn * a.H * a.W * a.Cin;
    if constexpr (MODE == CV_CONV3D) xn = a.x + (size_t)pn * a.T * a.H * a.W * a.Cin;         // frame 0 of the sample
    if constexpr (MODE == CV_POOL_DOWN) {
        const int tp = pn % a.T, n = pn / a.T;
        const int f1 = (a.Tin & 1) ? 2 * tp : 2 * tp + 1, f0 = f1 > 0 ? f1 - 1 : 0;               // odd count: frame 0 alone, then (2t' - 1, 2t')
        const size_t fs = (size_t)a.H * a.W * a.Cin;
        xn = a.x + ((size_t)n * a.Tin + f0) * fs;
        xb = a.x + ((size_t)n * a.Tin + f1) * fs;
    }
    if constexpr (MODE == CV_UP2X) {                                        // a.H, a.W: the source map; a.Ho = 2 a.H, a.Wo = 2 a.W
        const int t = pn % a.T, n = pn / a.T;
        const int f = a.T == a.Tin ? t : a.T == 2 * a.Tin ? t >> 1 : t == 0 ? 0 : 1 + ((t - 1) >> 1);
        xn = a.x + ((size_t)n * a.Tin + f) * ((size_t)a.H * a.W * a.Cin);
    }
    const int pad = a.pad;
    const int cchunks = a.Cin / CV_KC, iters = (MODE == CV_CONV3D ? 27 : a.ksize * a.ksize) * cchunks;

    float4 ra[2], rb[NB];
    auto fetch = [&](int it) {
        const int tap = it / cchunks, c0 = (it - tap * cchunks) * CV_KC;
        const int dy = tap / a.ksize - pad, dx = tap % a.ksize - pad;
        if constexpr (MODE == CV_AUX_TAIL) {
            const int iy = py + dy, ix = px + dx;
            const bool in = pvalid && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const float* src = xn + ((size_t)iy * a.W + ix) * a.Cin + c0;
            const int half = a.Cin >> 1;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c = c0 + 4 * (jq + 2 * i);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (in) {
                    v = *reinterpret_cast<const float4*>(src + 4 * (jq + 2 * i));
                    if (a.xtab) v = embed4(v, a.xtab, a.ytab, half, iy, ix, c);
                }
                ra[i] = v;
            }
        } else if constexpr (MODE == CV_TAIL) {
            const int iy = py + dy, ix = px + dx;
            const bool in = pvalid && iy >= 0 && iy < a.Ho && ix >= 0 && ix < a.Wo;
#pragma unroll
            for (int i = 0; i < 2; ++i)
                ra[i] = in ? sample4(xn, a.H, a.W, a.Cin, a.sy, a.sx, iy, ix, c0 + 4 * (jq + 2 * i), a.xtab, a.ytab) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else if constexpr (MODE == CV_CONV3D) {
            const int kt = tap / 9, r9 = tap - 9 * kt;
            const int iy = py + r9 / 3 - 1, ix = px + r9 % 3 - 1, ft = pt + kt - 2;
            const bool in = pvalid && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const size_t fs = (size_t)a.H * a.W * a.Cin;
            // the frame: of x; in front of frame 0, of prev (sample pn, frame ft + 2) or frame 0 of x again
            const float* fb = ft >= 0 ? xn + (size_t)ft * fs : a.prev ? a.prev + ((size_t)pn * 2 + (ft + 2)) * fs : xn;
            const float* src = fb + ((size_t)iy * a.W + ix) * a.Cin + c0;
#pragma unroll
            for (int i = 0; i < 2; ++i) ra[i] = in ? *reinterpret_cast<const float4*>(src + 4 * (jq + 2 * i)) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else if constexpr (MODE == CV_UP2X) {
            const int iy = py + dy, ix = px + dx;                               // on the up-sampled map
            const bool in = pvalid && iy >= 0 && iy < a.Ho && ix >= 0 && ix < a.Wo;
            const float* src = xn + ((size_t)(iy >> 1) * a.W + (ix >> 1)) * a.Cin + c0;
#pragma unroll
            for (int i = 0; i < 2; ++i) ra[i] = in ? *reinterpret_cast<const float4*>(src + 4 * (jq + 2 * i)) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else if constexpr (MODE == CV_POOL_DOWN) {
            const int iy = py * a.stride + dy, ix = px * a.stride + dx;
            const bool in = pvalid && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const size_t off = ((size_t)iy * a.W + ix) * a.Cin + c0;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (in) {
                    v = *reinterpret_cast<const float4*>(xn + off + 4 * (jq + 2 * i));
                    if (xb != xn) {
                        const float4 u = *reinterpret_cast<const float4*>(xb + off + 4 * (jq + 2 * i));
                        v = make_float4((v.x + u.x) * 0.5f, (v.y + u.y) * 0.5f, (v.z + u.z) * 0.5f, (v.w + u.w) * 0.5f);
                    }
                }
                ra[i] = v;
            }
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

    [[maybe_unused]] f32x16_t tot[TM][TN];                                  // CHUNKED: the sum of the finished runs
    if constexpr (CHUNKED) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[i][j][r] = 0.f;
    }

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
        if constexpr (CHUNKED) {
            const bool last = it + 1 == iters;
            if ((it & (CV_CHUNK_ITERS - 1)) == CV_CHUNK_ITERS - 1 || last) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            tot[i][j][r] += acc[i][j][r];
                            acc[i][j][r] = last ? tot[i][j][r] : 0.f;          // the epilogue reads acc
                        }
            }
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
        // hidden = conv + b1 (CV_TAIL: its ReLU) -> LDS [pixel][33]
        float* Hs = lds;
        const float bv = a.bias[l31];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const float v = acc[0][0][r] + bv;
            Hs[row * 33 + l31] = MODE == CV_TAIL ? fmaxf(v, 0.f) : v;
        }
        __syncthreads();
        if (tid < CV_BM && p0 + tid < a.M) {                                  // one thread per pixel
            const int64_t q = p0 + tid;
            [[maybe_unused]] float h[32];                                       // CV_AUX_TAIL: the normalised hidden values; CV_TAIL projects straight from LDS
            if constexpr (MODE == CV_AUX_TAIL) {
                // LayerNorm over the pixel's 32 values (mean and the biased variance of the centred values by pairwise sums, so 32 equal
                // values give variance 0 exactly), then ReLU
                float t[32];
#pragma unroll
                for (int c = 0; c < 32; ++c) t[c] = h[c] = Hs[tid * 33 + c];
#pragma unroll
                for (int n = 16; n >= 1; n >>= 1)
#pragma unroll
                    for (int c = 0; c < n; ++c) t[c] += t[c + n];
                const float mean = t[0] * (1.0f / 32.0f);
#pragma unroll
                for (int c = 0; c < 32; ++c) {
                    h[c] -= mean;
                    t[c] = h[c] * h[c];
                }
#pragma unroll
                for (int n = 16; n >= 1; n >>= 1)
#pragma unroll
                    for (int c = 0; c < n; ++c) t[c] += t[c + n];
                const float rstd = rsqrtf(t[0] * (1.0f / 32.0f) + a.eps);
#pragma unroll
                for (int c = 0; c < 32; ++c) h[c] = fmaxf(h[c] * rstd * a.ln_w[c] + a.ln_b[c], 0.f);
            }
            // the 1x1 conv 32 -> od: the last output is conf = 1 + exp, the others are preds, written as they are (CV_AUX_TAIL) or through
            // activate_head (CV_TAIL)
            for (int o = 0; o < a.od; ++o) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < 32; ++c) {
                    if constexpr (MODE == CV_AUX_TAIL) s = fmaf(a.w2[o * 32 + c], h[c], s);
                    else s = fmaf(a.w2[o * 32 + c], Hs[tid * 33 + c], s);
                }
                s += a.b2[o];
                if (o == a.od - 1) a.conf[q] = 1.0f + expf(s);
                else if constexpr (MODE == CV_AUX_TAIL) a.preds[(size_t)q * (a.od - 1) + o] = s;
                else a.preds[(size_t)q * (a.od - 1) + o] = a.act == 0 ? expf(s) : copysignf(expm1f(fabsf(s)), s);
            }
        }
    }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The checks and the ConvArgs fill that the two tail entry points share: x [N,h,w,C] read on an [N,H,W] output grid, 32 hidden channels, od outputs.
// An entry adds its own checks and fields (activation and scales; LayerNorm parameters) and launches.
static int32_t tail_args(ConvArgs& a, const float* x, const float* xtab, const float* ytab, const float* w1_packed, const float* b1, const float* w2,
                         const float* b2, float* preds, float* conf, int64_t N, int64_t h, int64_t w, int64_t C, int64_t H, int64_t W, int32_t od) {
    if (!x || !w1_packed || !b1 || !w2 || !b2 || !preds || !conf || N <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 15))
        return VGPA_ERR_INVALID;
    if ((xtab == nullptr) != (ytab == nullptr) || od < 2 || od > 8) return VGPA_ERR_INVALID;
    if (h > (1 << 20) || w > (1 << 20) || H > (1 << 20) || W > (1 << 20) || C > (1 << 20)) return VGPA_ERR_INVALID;
    if (!aligned16(x) || !aligned16(w1_packed) || !aligned16(xtab) || !aligned16(ytab)) return VGPA_ERR_INVALID;
    a.x = x; a.w = w1_packed; a.bias = b1; a.xtab = xtab; a.ytab = ytab; a.w2 = w2; a.b2 = b2; a.preds = preds; a.conf = conf;
    a.N = (int)N; a.H = (int)h; a.W = (int)w; a.Ho = (int)H; a.Wo = (int)W; a.Cin = (int)C; a.Cout = 32; a.ksize = 3; a.stride = 1; a.pad = 1;
    a.od = od;
    a.M = N * H * W;
    return VGPA_OK;
}

template <int MODE>
static int32_t conv_launch(const ConvArgs& a, hipStream_t stream) {
    const int64_t mb = (a.M + CV_BM - 1) / CV_BM;
    if (mb <= 0 || mb > 0x7fffffffLL) return VGPA_ERR_INVALID;
    if constexpr (MODE == CV_TAIL || MODE == CV_AUX_TAIL) {
        VGPA_LAUNCH((conv_kernel<4, 1, 1, 1, MODE>), dim3((unsigned)mb, 1), dim3(CV_THREADS), 0, stream, a);
    } else if (a.Cout >= 128) {
        VGPA_LAUNCH((conv_kernel<2, 2, 2, 2, MODE>), dim3((unsigned)mb, (unsigned)((a.Cout + 127) / 128)), dim3(CV_THREADS), 0, stream, a);
    } else if (a.Cout > 32) {
        VGPA_LAUNCH((conv_kernel<2, 2, 2, 1, MODE>), dim3((unsigned)mb, (unsigned)((a.Cout + 63) / 64)), dim3(CV_THREADS), 0, stream, a);
    } else {
        VGPA_LAUNCH((conv_kernel<4, 1, 1, 1, MODE>), dim3((unsigned)mb, 1), dim3(CV_THREADS), 0, stream, a);
    }
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

// The plain 2-D entry (CV_CONV, CV_CONV_CHUNKED): the checks, the ConvArgs fill and the launch of x [N,H,W,Cin] under a ksize x ksize window with pad_lo zero
// rows / columns in front and pad_hi behind
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
