// The front of the DINOv2 backbone in one launch: DinoVisionTransformer.prepare_tokens_with_masks(x, masks=None)
// (vggt/layers/vision_transformer.py:214-226) = patch projection (Conv2d, kernel = stride = p) + class token + position table + register tokens.
//
//   out[n, 0, :]         = cls + pos[0]
//   out[n, 1..R, :]      = reg                                  (no position: the reference inserts the registers after the addition)
//   out[n, 1 + R + j, :] = W . patch_j + bias + pos[1 + j]      j = gy * (W / p) + gx
//
// The projection is an implicit GEMM, M = N * P patches (flat), N = C channels, K = 3 p p walked in chunks of 16 in the convolution weight's own
// order k = (c, ky, kx); the packed weight [Kpad][C] is zero-padded to a multiple of 16 rows and the A loader feeds zeros for k >= K.  The A tile is
// gathered straight from the NCHW image: every thread owns ONE patch for the whole K loop and half of each chunk (8 consecutive k: pieces of one or two
// patch rows, so neighbouring lanes = neighbouring patches read one contiguous image row between them), as 8-byte pairs when p is even (a patch row
// starts on an even pixel) and element by element otherwise.  No im2col tensor, no cat / add passes.
//
// The core is the exact-fp32 MFMA loop of vggt_heads.hip (v_mfma_f32_32x32x2_f32, both LDS tiles k-major with a row stride = 32 (mod 64) dwords, the
// next chunk's global loads in flight while the current one multiplies).  Every output element is summed in one fixed order (k-ordered fp32 chains over
// blocks of 64 k, the blocks added in order) that does not depend on which tile row the patch landed in: any split of the N frames over calls gives
// the same bits.  bf16 input is widened on load, bf16 output is one rounding of
// the fp32 result.
#include "common.h"

#define DE_THREADS 256
#define DE_BM 128
#define DE_KC 16
#define DE_AS (DE_BM + 32)
#define DE_BLOCK 4             // chunks per summation block (a power of two)
#define DE_SPECIAL_ROWS 8      // (frame, special row) pairs per special-row workgroup

struct EmbedArgs {
    const void* img;     // [N,3,H,W] fp32 | bf16
    const float* w;      // [Kpad][C]
    const float* bias;   // [C]
    const float* cls;    // [C]
    const float* reg;    // [R][C] | NULL when R == 0
    const float* pos;    // [1 + P][C]
    void* out;           // [N, 1 + R + P, C] fp32 | bf16
    int N, H, W, p, C, R, Kpad, P, gw, in_bf16, out_bf16, vec2;
    int64_t M;           // N * P
    unsigned mb;         // workgroups of the projection along x; the ones behind them write the special rows
};

__device__ __forceinline__ void de_store(void* out, size_t idx, float v, int out_bf16) {
    if (out_bf16) reinterpret_cast<bf16_t*>(out)[idx] = f32_to_bf16(v);
    else reinterpret_cast<float*>(out)[idx] = v;
}

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(DE_THREADS) void dino_embed_kernel(const EmbedArgs a) {
    constexpr int BN = WN * TN * 32;
    constexpr int BS = (BN % 64 == 0) ? BN + 32 : BN + 64;
    constexpr int NB = (DE_KC * BN / 4 + DE_THREADS - 1) / DE_THREADS;      // float4 of the weight tile per thread
    static_assert(WM * WN == 4 && WM * TM * 32 == DE_BM, "4 waves, 128 patches");
    __shared__ __attribute__((aligned(16))) float lds[DE_KC * DE_AS + DE_KC * BS];
    float* As = lds;
    float* Bs = lds + DE_KC * DE_AS;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.y * BN;
    const int T = 1 + a.R + a.P;

    if (blockIdx.x >= a.mb) {
        // class and register rows: 8 (frame, row) pairs per workgroup, 32 lanes across the channels of this column tile
        const int64_t pair = (int64_t)(blockIdx.x - a.mb) * DE_SPECIAL_ROWS + (tid >> 5);
        if (pair >= (int64_t)a.N * (1 + a.R)) return;
        const int n = (int)(pair / (1 + a.R)), r = (int)(pair % (1 + a.R));
        for (int co = n0 + (tid & 31); co < n0 + BN && co < a.C; co += 32) {
            const float v = r == 0 ? a.cls[co] + a.pos[co] : a.reg[(size_t)(r - 1) * a.C + co];
            de_store(a.out, ((size_t)n * T + r) * a.C + co, v, a.out_bf16);
        }
        return;
    }

    const int wm = wave / WN, wn = wave % WN;
    const int64_t p0 = (int64_t)blockIdx.x * DE_BM;

    // this thread's patch of the A tile, and its half (8 consecutive k) of every chunk
    const int pl = tid & (DE_BM - 1), jq = tid >> 7;
    const int64_t q = p0 + pl;
    const bool pvalid = q < a.M;
    int pn = 0, y0 = 0, x0 = 0;
    if (pvalid) {
        const int j = (int)(q % a.P);
        pn = (int)(q / a.P);
        y0 = (j / a.gw) * a.p;
        x0 = (j % a.gw) * a.p;
    }
    const size_t frame = (size_t)pn * 3 * a.H * a.W;
    const float* imf = reinterpret_cast<const float*>(a.img) + frame;
    const bf16_t* imh = reinterpret_cast<const bf16_t*>(a.img) + frame;
    const int pp = a.p * a.p, iters = a.Kpad / DE_KC;

    float ra[8];
    float4 rb[NB];
    auto fetch = [&](int it) {
        const int k = it * DE_KC + jq * 8;
        int c = k / pp;
        const int rem = k - c * pp;
        int ky = rem / a.p, kx = rem - ky * a.p;
        int off = (c * a.H + y0 + ky) * a.W + x0 + kx;                      // element offset inside the frame; c >= 3 is the zero padding of K
        if (a.vec2) {
#pragma unroll
            for (int i = 0; i < 8; i += 2) {
                const bool in = pvalid && c < 3;
                if (a.in_bf16) {
                    const uint32_t v = in ? *reinterpret_cast<const uint32_t*>(imh + off) : 0u;
                    ra[i] = bf16lo_to_f32(v);
                    ra[i + 1] = bf16hi_to_f32(v);
                } else {
                    const float2 v = in ? *reinterpret_cast<const float2*>(imf + off) : make_float2(0.f, 0.f);
                    ra[i] = v.x;
                    ra[i + 1] = v.y;
                }
                kx += 2;
                off += 2;
                if (kx >= a.p) {
                    kx = 0;
                    off += a.W - a.p;
                    if (++ky >= a.p) {
                        ky = 0;
                        off += (a.H - a.p) * a.W;
                        ++c;
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bool in = pvalid && c < 3;
                ra[i] = !in ? 0.f : a.in_bf16 ? bf16_to_f32(imh[off]) : imf[off];
                ++kx;
                ++off;
                if (kx >= a.p) {
                    kx = 0;
                    off += a.W - a.p;
                    if (++ky >= a.p) {
                        ky = 0;
                        off += (a.H - a.p) * a.W;
                        ++c;
                    }
                }
            }
        }
        const float* wk = a.w + (size_t)it * DE_KC * a.C;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + i * DE_THREADS, row = idx / (BN / 4), col = (idx % (BN / 4)) * 4;
            const bool in = idx < DE_KC * BN / 4 && n0 + col < a.C;          // C is a multiple of 32: a float4 is inside or outside as a whole
            rb[i] = in ? *reinterpret_cast<const float4*>(wk + (size_t)row * a.C + n0 + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i) As[(jq * 8 + i) * DE_AS + pl] = ra[i];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + i * DE_THREADS, row = idx / (BN / 4), col = (idx % (BN / 4)) * 4;
            if (idx < DE_KC * BN / 4) *reinterpret_cast<float4*>(Bs + row * BS + col) = rb[i];
        }
    };

    // blocked summation: `acc` collects DE_BLOCK chunks (64 k), then joins `tot` -- a fixed order like the plain chain, with a third of its rounding error
    // (a 588-term fp32 chain alone sits at 5-9e-7 of the largest output, ~10 x what torch's convolution leaves at some shapes)
    f32x16_t acc[TM][TN], tot[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = tot[i][j][r] = 0.f;

    fetch(0);
    stash();
    __syncthreads();
    const int l31 = lane & 31, lh = lane >> 5;
    for (int it = 0; it < iters; ++it) {
        if (it + 1 < iters) fetch(it + 1);
#pragma unroll
        for (int ks = 0; ks < DE_KC / 2; ++ks) {
            const int k = 2 * ks + lh;
            float fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = As[k * DE_AS + (wm * TM + i) * 32 + l31];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = Bs[k * BS + (wn * TN + j) * 32 + l31];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if ((it & (DE_BLOCK - 1)) == DE_BLOCK - 1 || it + 1 == iters) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    tot[i][j] += acc[i][j];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
                }
        }
        __syncthreads();
        if (it + 1 < iters) {
            stash();
            __syncthreads();
        }
    }

    // accumulator element r of lane l: channel column l & 31, patch row (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int co = n0 + (wn * TN + j) * 32 + l31;
        if (co >= a.C) continue;
        const float bv = a.bias[co];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t qo = p0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (qo >= a.M) continue;
                const int n = (int)(qo / a.P), jo = (int)(qo % a.P);
                const float v = (tot[i][j][r] + bv) + a.pos[(size_t)(1 + jo) * a.C + co];
                de_store(a.out, ((size_t)n * T + 1 + a.R + jo) * a.C + co, v, a.out_bf16);
            }
        }
    }
}

static bool de_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" {

int32_t vgpa_dino_embed(const void* images, int32_t in_dtype, const float* w_packed, int64_t k_packed, const float* bias, const float* cls_token,
                        const float* register_tokens, const float* pos, void* out, int32_t out_dtype, int64_t N, int64_t H, int64_t W,
                        int64_t patch, int64_t C, int64_t R, hipStream_t stream) {
    if (!images || !w_packed || !bias || !cls_token || !pos || !out || (R > 0 && !register_tokens)) return VGPA_ERR_INVALID;
    if ((in_dtype != VGPA_DTYPE_F32 && in_dtype != VGPA_DTYPE_BF16) || (out_dtype != VGPA_DTYPE_F32 && out_dtype != VGPA_DTYPE_BF16))
        return VGPA_ERR_INVALID;
    if (N <= 0 || H <= 0 || W <= 0 || patch <= 0 || patch > 64 || C <= 0 || R < 0 || R > 64 || H > (1 << 14) || W > (1 << 14) || C > (1 << 16) ||
        N > (1 << 20))
        return VGPA_ERR_INVALID;
    if (H % patch || W % patch || (C & 31)) return VGPA_ERR_INVALID;
    if (k_packed != (3 * patch * patch + DE_KC - 1) / DE_KC * DE_KC) return VGPA_ERR_INVALID;
    if (!de_aligned16(images) || !de_aligned16(w_packed) || !de_aligned16(pos) || !de_aligned16(out)) return VGPA_ERR_INVALID;
    EmbedArgs a = {};
    a.img = images; a.w = w_packed; a.bias = bias; a.cls = cls_token; a.reg = register_tokens; a.pos = pos; a.out = out;
    a.N = (int)N; a.H = (int)H; a.W = (int)W; a.p = (int)patch; a.C = (int)C; a.R = (int)R; a.Kpad = (int)k_packed;
    a.gw = (int)(W / patch);
    a.P = (int)(H / patch) * a.gw;
    a.in_bf16 = in_dtype == VGPA_DTYPE_BF16; a.out_bf16 = out_dtype == VGPA_DTYPE_BF16;
    a.vec2 = (patch & 1) == 0;                                              // a patch row starts on an even pixel: 8-byte (fp32) / 4-byte (bf16) pairs
    a.M = N * a.P;
    const int64_t mb = (a.M + DE_BM - 1) / DE_BM, sb = (N * (1 + R) + DE_SPECIAL_ROWS - 1) / DE_SPECIAL_ROWS;
    if (mb + sb > 0x7fffffffLL) return VGPA_ERR_INVALID;
    a.mb = (unsigned)mb;
    const dim3 block(DE_THREADS);
    if (C >= 128) {
        VGPA_LAUNCH((dino_embed_kernel<2, 2, 2, 2>), dim3((unsigned)(mb + sb), (unsigned)((C + 127) / 128)), block, 0, stream, a);
    } else if (C > 32) {
        VGPA_LAUNCH((dino_embed_kernel<2, 2, 2, 1>), dim3((unsigned)(mb + sb), (unsigned)((C + 63) / 64)), block, 0, stream, a);
    } else {
        VGPA_LAUNCH((dino_embed_kernel<4, 1, 1, 1>), dim3((unsigned)(mb + sb), 1), block, 0, stream, a);
    }
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

}  // extern "C"
