// SuperPoint (DeTone et al. 2018, as packaged by cvg/LightGlue: lightglue/superpoint.py, lightglue/utils.py), the part around the ten 3x3
// convolutions and the 1x1 descriptor head, which run on conv_kernel of vggt_heads.hip as they are.  Everything fp32, channels-last, forward only,
// no float atomics, bit-identical from run to run and for every split of the frames over calls:
//   sp_input_kernel    frames -> conv1a's pre-ReLU output [T,Ho,Wo,64] in one launch: gray conversion, g / 255 through a host-made table, the
//                      bilinear resize of Extractor.extract (F.interpolate, align_corners=False, torch's fp32 index arithmetic) and the 3x3 1 -> 64
//                      convolution with zero padding on the VALU.  A 16 x 16 tile's 18 x 18 gray patch lives in LDS; a thread owns four output
//                      channels of a pixel, a wave stores 1 KiB of consecutive output.  The layer is bound by its 256 B of output per pixel.
//   sp_head_kernel     convPa's pre-ReLU map [T,h,w,256] -> score image [T,8h,8w]: ReLU, the 1x1 convolution to 65 channels, softmax over the 65,
//                      the dustbin dropped, the 8 x 8 depth-to-space.  Lane = kept channel, a wave walks SP_HEAD_CPW cells per weight read; the dustbin
//                      logit is a wave reduction.  The logits never leave registers.
//   sp_nms_kernel      upstream's three-round simple_nms (exact comparisons only) on a 32 x 32 tile with a halo of 5 radii in LDS: five window maxima
//                      deep, each separable (row pass, column pass) and each over the shrinking part of the region that is still right.  Outside the
//                      image a window sees -inf, as max_pool2d's padding.  Then the `remove_borders` frame of -1.
//   sp_count_kernel / sp_compact_kernel    score > threshold, compacted in row-major order by block scans (integer counts only)
//   sp_select_kernel   one workgroup per frame: everything when the count fits, else the top k by a 4 x 8-bit radix select (the scheme of
//                      csrc/scorer2.hip, per frame and in LDS), ties at the cut taken in row-major order, then a bitonic sort of the k survivors by
//                      (score descending, index ascending).  torch.topk leaves the tie order open: this one is fixed.
//   sp_sample_kernel   sample_descriptors: one wave per keypoint reads its four neighbour vectors of the raw descriptor map, unit-normalises each
//                      (x / max(|x|, 1e-12)), blends them bilinearly (grid_sample, align_corners=True, zeros outside) and normalises again.
//                      The normalised map is never written.
//
// RESTATED, NOT PINNED (neither cv2 nor lightglue nor kornia is available to check against): the 8-bit RGB -> gray weights below are cv2's 15-bit
// fixed-point form written from memory.  They live in SP_GRAY_* and nowhere else.
#include "common.h"
#include <math.h>

#define SP_GRAY_R 9798
#define SP_GRAY_G 19235
#define SP_GRAY_B 3735
#define SP_GRAY_SHIFT 15

#define SP_THREADS 256
#define SP_IN_TILE 16
#define SP_IN_LD (SP_IN_TILE + 3)
#define SP_MODE_RGB8 0          // uint8 [T,H,W,3]
#define SP_MODE_GRAY_F32 1      // float [T,1,H,W]
#define SP_MODE_RGB_F32 3       // float [T,3,H,W], reduced with (0.299, 0.587, 0.114)

#define SP_HEAD_CPW 8           // cells a wave carries through one pass over the weights
#define SP_C 256                // width of convPa / convDa / the descriptor

#define SP_NMS_TILE 32
#define SP_NMS_MAXR 4

#define SP_CHUNK_PER_THREAD 8
#define SP_CHUNK (SP_THREADS * SP_CHUNK_PER_THREAD)
#define SP_SEL_THREADS 1024
#define SP_SEL_MAXK 4096

__device__ __forceinline__ int sp_gray_u8(int r, int g, int b) {
    return (SP_GRAY_R * r + SP_GRAY_G * g + SP_GRAY_B * b + (1 << (SP_GRAY_SHIFT - 1))) >> SP_GRAY_SHIFT;
}

struct SpInArgs {
    const void* src;
    const float* table;
    const float* w;          // [9][64]
    const float* bias;       // [64]
    float* out;              // [T,Ho,Wo,64]
    float* gray;             // [T,Ho,Wo] or null
    int mode, H, W, Ho, Wo;
    float sy, sx;
};

__device__ __forceinline__ float sp_src(const SpInArgs& a, int t, int y, int x) {
    const size_t HW = (size_t)a.H * a.W, p = (size_t)y * a.W + x;
    if (a.mode == SP_MODE_RGB8) {
        const uint8_t* s = (const uint8_t*)a.src + ((size_t)t * HW + p) * 3;
        return a.table[sp_gray_u8(s[0], s[1], s[2])];
    }
    const float* s = (const float*)a.src;
    if (a.mode == SP_MODE_GRAY_F32) return s[(size_t)t * HW + p];
    s += (size_t)t * 3 * HW + p;
    return s[0] * 0.299f + s[HW] * 0.587f + s[2 * HW] * 0.114f;
}

// torch's area_pixel_compute_source_index + guard for align_corners=False, fp32, no contraction
__device__ __forceinline__ void sp_axis(float scale, int dst, int in, int& i0, int& i1, float& l1) {
    float f = __fsub_rn(__fmul_rn(scale, (float)dst + 0.5f), 0.5f);
    f = f < 0.f ? 0.f : f;
    i0 = min((int)f, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(__fsub_rn(f, (float)i0), 0.f), 1.f);
}

__device__ __forceinline__ float sp_resized(const SpInArgs& a, int t, int oy, int ox) {
    int y0, y1, x0, x1;
    float ly, lx;
    sp_axis(a.sy, oy, a.H, y0, y1, ly);
    sp_axis(a.sx, ox, a.W, x0, x1, lx);
    const float ly0 = 1.f - ly, lx0 = 1.f - lx;
    const float v00 = sp_src(a, t, y0, x0), v01 = sp_src(a, t, y0, x1), v10 = sp_src(a, t, y1, x0), v11 = sp_src(a, t, y1, x1);
    return ly0 * (lx0 * v00 + lx * v01) + ly * (lx0 * v10 + lx * v11);
}

// grid (tiles x, tiles y, T)
__global__ __launch_bounds__(SP_THREADS) void sp_input_kernel(const SpInArgs a) {
    __shared__ float g[(SP_IN_TILE + 2) * SP_IN_LD];
    const int t = blockIdx.z, ty0 = blockIdx.y * SP_IN_TILE, tx0 = blockIdx.x * SP_IN_TILE;
    for (int i = threadIdx.x; i < (SP_IN_TILE + 2) * (SP_IN_TILE + 2); i += SP_THREADS) {
        const int ly = i / (SP_IN_TILE + 2), lx = i - ly * (SP_IN_TILE + 2);
        const int oy = ty0 + ly - 1, ox = tx0 + lx - 1;
        float v = 0.f;                                                   // the convolution's zero padding
        if (oy >= 0 && oy < a.Ho && ox >= 0 && ox < a.Wo) {
            v = sp_resized(a, t, oy, ox);
            if (a.gray && ly >= 1 && ly <= SP_IN_TILE && lx >= 1 && lx <= SP_IN_TILE) a.gray[((size_t)t * a.Ho + oy) * a.Wo + ox] = v;
        }
        g[ly * SP_IN_LD + lx] = v;
    }
    __syncthreads();
    const int c = (threadIdx.x & 15) * 4, px = threadIdx.x >> 4;
    float4 wk[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k] = *reinterpret_cast<const float4*>(a.w + k * 64 + c);
    const float4 b = *reinterpret_cast<const float4*>(a.bias + c);
    const int ox = tx0 + px;
    if (ox >= a.Wo) return;
    for (int py = 0; py < SP_IN_TILE; ++py) {
        const int oy = ty0 + py;
        if (oy >= a.Ho) break;
        float4 acc = b;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float v = g[(py + ky) * SP_IN_LD + px + kx];
                const float4 w4 = wk[ky * 3 + kx];
                acc.x = fmaf(v, w4.x, acc.x); acc.y = fmaf(v, w4.y, acc.y); acc.z = fmaf(v, w4.z, acc.z); acc.w = fmaf(v, w4.w, acc.w);
            }
        *reinterpret_cast<float4*>(a.out + (((size_t)t * a.Ho + oy) * a.Wo + ox) * 64 + c) = acc;
    }
}

// x [cells][256] pre-ReLU, w [256][65], bias [65] -> score [T,8h,8w]; block = 4 waves x SP_HEAD_CPW cells
__global__ __launch_bounds__(SP_THREADS) void sp_head_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                              float* __restrict__ score, int64_t cells, int h, int wd) {
    __shared__ float xs[SP_THREADS / 64][SP_HEAD_CPW][SP_C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t cell0 = ((int64_t)blockIdx.x * (SP_THREADS / 64) + wave) * SP_HEAD_CPW;
#pragma unroll
    for (int c = 0; c < SP_HEAD_CPW; ++c) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cell0 + c < cells) v = *reinterpret_cast<const float4*>(x + (size_t)(cell0 + c) * SP_C + lane * 4);
        v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
        *reinterpret_cast<float4*>(&xs[wave][c][lane * 4]) = v;
    }
    __syncthreads();
    float acc[SP_HEAD_CPW], dust[SP_HEAD_CPW];
    const float b = bias[lane];
#pragma unroll
    for (int c = 0; c < SP_HEAD_CPW; ++c) acc[c] = b;
    for (int k = 0; k < SP_C; k += 4) {
        const float w0 = w[(k + 0) * 65 + lane], w1 = w[(k + 1) * 65 + lane], w2 = w[(k + 2) * 65 + lane], w3 = w[(k + 3) * 65 + lane];
#pragma unroll
        for (int c = 0; c < SP_HEAD_CPW; ++c) {
            const float4 v = *reinterpret_cast<const float4*>(&xs[wave][c][k]);
            acc[c] = fmaf(v.w, w3, fmaf(v.z, w2, fmaf(v.y, w1, fmaf(v.x, w0, acc[c]))));
        }
    }
    const float d0 = w[(4 * lane + 0) * 65 + 64], d1 = w[(4 * lane + 1) * 65 + 64], d2 = w[(4 * lane + 2) * 65 + 64], d3 = w[(4 * lane + 3) * 65 + 64];
    const float bd = bias[64];
#pragma unroll
    for (int c = 0; c < SP_HEAD_CPW; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(&xs[wave][c][lane * 4]);
        dust[c] = wave_sum(fmaf(v.w, d3, fmaf(v.z, d2, fmaf(v.y, d1, v.x * d0)))) + bd;
    }
    const int dy = lane >> 3, dx = lane & 7;
#pragma unroll
    for (int c = 0; c < SP_HEAD_CPW; ++c) {
        const int64_t cell = cell0 + c;
        const float m = fmaxf(wave_max(acc[c]), dust[c]);
        const float e = expf(acc[c] - m);
        const float sum = wave_sum(e) + expf(dust[c] - m);
        if (cell < cells) {
            const int cx = (int)(cell % wd), cy = (int)((cell / wd) % h);
            const int64_t t = cell / ((int64_t)wd * h);
            score[((size_t)t * 8 * h + 8 * cy + dy) * (8 * (size_t)wd) + 8 * cx + dx] = e / sum;
        }
    }
}

// f(ly, lx, index) over the region inset by IY radii in y and IX radii in x
template <int RAD, int IY, int IX, typename F>
__device__ __forceinline__ void sp_region(F f) {
    constexpr int R = SP_NMS_TILE + 10 * RAD, y0 = IY * RAD, x0 = IX * RAD, h = R - 2 * y0, w = R - 2 * x0;
    for (int i = threadIdx.x; i < h * w; i += SP_THREADS) {
        const int ly = y0 + i / w, lx = x0 + i % w;
        f(ly, lx, ly * R + lx);
    }
}

// one suppression round on masks that are right from inset D (in radii) inwards; leaves M right from inset D + 2
template <int RAD, int D>
__device__ __forceinline__ void sp_nms_round(const float* S, float* B, uint8_t* M, uint8_t* Bm, uint8_t* SUPP) {
    constexpr int R = SP_NMS_TILE + 10 * RAD;
    sp_region<RAD, D, D + 1>([&](int, int, int i) {                       // supp = max_pool(max_mask) > 0: rows, then columns
        uint8_t m = 0;
#pragma unroll
        for (int d = -RAD; d <= RAD; ++d) m |= M[i + d];
        Bm[i] = m;
    });
    __syncthreads();
    sp_region<RAD, D + 1, D + 1>([&](int, int, int i) {
        uint8_t m = 0;
#pragma unroll
        for (int d = -RAD; d <= RAD; ++d) m |= Bm[i + d * R];
        SUPP[i] = (m && S[i] != -INFINITY) ? 1 : 0;
    });
    __syncthreads();
    sp_region<RAD, D + 1, D + 2>([&](int, int, int i) {                   // window maxima of where(supp, 0, s)
        float m = -INFINITY;
#pragma unroll
        for (int d = -RAD; d <= RAD; ++d) m = fmaxf(m, SUPP[i + d] ? 0.f : S[i + d]);
        B[i] = m;
    });
    __syncthreads();
    sp_region<RAD, D + 2, D + 2>([&](int, int, int i) {
        float m = -INFINITY;
#pragma unroll
        for (int d = -RAD; d <= RAD; ++d) m = fmaxf(m, B[i + d * R]);
        if (S[i] != -INFINITY && !SUPP[i] && S[i] == m) M[i] = 1;        // max_mask |= new_max_mask & ~supp_mask
    });
    __syncthreads();
}

// grid (tiles x, tiles y, T).  Region = tile + halo of 5 RAD on every side: simple_nms is five window maxima deep, and each pass computes only the
// part of the region whose inputs the pass before it got right (one radius further in per separable direction), so the tile is what is left.
// Outside the image S = -inf (max_pool2d pads with -inf), and neither mask is ever set there.
template <int RAD>
__global__ __launch_bounds__(SP_THREADS) void sp_nms_kernel(const float* __restrict__ score, float* __restrict__ out, int Hs, int Ws, int border) {
    constexpr int R = SP_NMS_TILE + 10 * RAD, halo = 5 * RAD;
    __shared__ float S[R * R], B[R * R];
    __shared__ uint8_t M[R * R], Bm[R * R], SUPP[R * R];
    const int y0 = blockIdx.y * SP_NMS_TILE - halo, x0 = blockIdx.x * SP_NMS_TILE - halo;
    const float* src = score + (size_t)blockIdx.z * Hs * Ws;
    sp_region<RAD, 0, 0>([&](int ly, int lx, int i) {
        const int gy = y0 + ly, gx = x0 + lx;
        S[i] = (gy >= 0 && gy < Hs && gx >= 0 && gx < Ws) ? src[(size_t)gy * Ws + gx] : -INFINITY;
    });
    __syncthreads();
    sp_region<RAD, 0, 1>([&](int, int, int i) {                           // max_mask = s == max_pool(s)
        float m = -INFINITY;
#pragma unroll
        for (int d = -RAD; d <= RAD; ++d) m = fmaxf(m, S[i + d]);
        B[i] = m;
    });
    __syncthreads();
    sp_region<RAD, 1, 1>([&](int, int, int i) {
        float m = -INFINITY;
#pragma unroll
        for (int d = -RAD; d <= RAD; ++d) m = fmaxf(m, B[i + d * R]);
        M[i] = (S[i] != -INFINITY && S[i] == m) ? 1 : 0;
    });
    __syncthreads();
    sp_nms_round<RAD, 1>(S, B, M, Bm, SUPP);
    sp_nms_round<RAD, 3>(S, B, M, Bm, SUPP);
    float* dst = out + (size_t)blockIdx.z * Hs * Ws;
    sp_region<RAD, 5, 5>([&](int ly, int lx, int i) {
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= Hs || gx >= Ws) return;
        float v = M[i] ? S[i] : 0.f;
        if (gy < border || gy >= Hs - border || gx < border || gx >= Ws - border) v = -1.f;
        dst[(size_t)gy * Ws + gx] = v;
    });
}

// exclusive prefix of v over the workgroup (blockDim.x a multiple of 64, at most 1024), *total = the workgroup's sum; smem holds 16 words
__device__ __forceinline__ uint32_t sp_block_exscan(uint32_t v, uint32_t* smem, uint32_t* total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) smem[wid] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int i = 0; i < nw; ++i) {
        if (i < wid) base += smem[i];
        tot += smem[i];
    }
    *total = tot;
    return base + inc - v;
}

// grid (chunks, T): chunk_count[t][chunk] = candidates among the chunk's SP_CHUNK row-major pixels
__global__ __launch_bounds__(SP_THREADS) void sp_count_kernel(const float* __restrict__ nms, int64_t HW, float thr, int nchunks,
                                                               uint32_t* __restrict__ chunk_count) {
    __shared__ uint32_t red[16];
    const float* src = nms + (size_t)blockIdx.y * HW;
    const int64_t p0 = (int64_t)blockIdx.x * SP_CHUNK + threadIdx.x * SP_CHUNK_PER_THREAD;
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < SP_CHUNK_PER_THREAD; ++j)
        if (p0 + j < HW && src[p0 + j] > thr) ++n;
    const uint32_t s = block_sum<uint32_t>(n, red);
    if (threadIdx.x == 0) chunk_count[(size_t)blockIdx.y * nchunks + blockIdx.x] = s;
}

__global__ __launch_bounds__(SP_THREADS) void sp_compact_kernel(const float* __restrict__ nms, int64_t HW, float thr, int nchunks,
                                                                 const uint32_t* __restrict__ chunk_count, int32_t* __restrict__ cand_idx,
                                                                 float* __restrict__ cand_score, uint32_t* __restrict__ ncand) {
    __shared__ uint32_t red[16];
    const int t = blockIdx.y;
    const float* src = nms + (size_t)t * HW;
    uint32_t before = 0;
    for (int i = threadIdx.x; i < (int)blockIdx.x; i += SP_THREADS) before += chunk_count[(size_t)t * nchunks + i];
    before = block_sum<uint32_t>(before, red);
    const int64_t p0 = (int64_t)blockIdx.x * SP_CHUNK + threadIdx.x * SP_CHUNK_PER_THREAD;
    float v[SP_CHUNK_PER_THREAD];
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < SP_CHUNK_PER_THREAD; ++j) {
        v[j] = p0 + j < HW ? src[p0 + j] : -INFINITY;
        if (p0 + j < HW && v[j] > thr) ++n;
    }
    uint32_t total;
    uint32_t o = before + sp_block_exscan(n, red, &total);
#pragma unroll
    for (int j = 0; j < SP_CHUNK_PER_THREAD; ++j)
        if (p0 + j < HW && v[j] > thr) {
            cand_idx[(size_t)t * HW + o] = (int32_t)(p0 + j);
            cand_score[(size_t)t * HW + o] = v[j];
            ++o;
        }
    if ((int)blockIdx.x == nchunks - 1 && threadIdx.x == 0) ncand[t] = before + total;
}

// an order-preserving map of float bits to uint32
__device__ __forceinline__ uint32_t sp_okey(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ void sp_emit(float* kp, float* sc, int64_t slot, int32_t idx, float s, int Ws) {
    kp[2 * slot] = (float)(idx % Ws);
    kp[2 * slot + 1] = (float)(idx / Ws);
    sc[slot] = s;
}

// grid T.  kp [T,kcap,2] (x, y), sc [T,kcap], counts [T] = min(candidates, kcap); rows past a frame's count are left as they are
__global__ __launch_bounds__(SP_SEL_THREADS) void sp_select_kernel(const int32_t* __restrict__ cand_idx, const float* __restrict__ cand_score,
                                                                    const uint32_t* __restrict__ ncand, int64_t HW, int Ws, int64_t kcap,
                                                                    float* __restrict__ kp, float* __restrict__ sc, int32_t* __restrict__ counts) {
    __shared__ unsigned long long keys[SP_SEL_MAXK];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t red[16];
    __shared__ uint32_t pick[2];
    const int t = blockIdx.x;
    const int32_t* ci = cand_idx + (size_t)t * HW;
    const float* cs = cand_score + (size_t)t * HW;
    float* kpo = kp + (size_t)t * kcap * 2;
    float* sco = sc + (size_t)t * kcap;
    const int64_t n = ncand[t];
    if (n <= kcap) {                                                     // nothing is cut: row-major order
        for (int64_t i = threadIdx.x; i < n; i += SP_SEL_THREADS) sp_emit(kpo, sco, i, ci[i], cs[i], Ws);
        if (threadIdx.x == 0) counts[t] = (int32_t)n;
        return;
    }
    const uint32_t k = (uint32_t)kcap;                                   // <= SP_SEL_MAXK, checked on the host
    uint32_t prefix = 0, mask = 0, remaining = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        for (int64_t i = threadIdx.x; i < n; i += SP_SEL_THREADS) {
            const uint32_t key = sp_okey(cs[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);      // integer counts: the order of the adds cannot show
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t above = 0;
            int b = 255;
            for (; b > 0; --b) {
                if (above + hist[b] >= remaining) break;
                above += hist[b];
            }
            pick[0] = (uint32_t)b;
            pick[1] = above;
        }
        __syncthreads();
        prefix |= pick[0] << shift;
        mask |= 255u << shift;
        remaining -= pick[1];
        __syncthreads();
    }
    // prefix = the k-th largest key; `remaining` (>= 1) of the candidates that carry it are kept, the first in row-major order
    const uint32_t n_gt = k - remaining;
    uint32_t done_gt = 0, done_eq = 0;
    for (int64_t i0 = 0; i0 < n; i0 += SP_SEL_THREADS) {
        const int64_t i = i0 + threadIdx.x;
        uint32_t key = 0;
        float s = 0.f;
        int32_t idx = 0;
        if (i < n) {
            s = cs[i];
            idx = ci[i];
            key = sp_okey(s);
        }
        const uint32_t gt = (i < n && key > prefix) ? 1u : 0u, eq = (i < n && key == prefix) ? 1u : 0u;
        uint32_t total;
        const uint32_t ex = sp_block_exscan(gt | (eq << 16), red, &total);
        const uint32_t rg = done_gt + (ex & 0xffffu), re = done_eq + (ex >> 16);
        const unsigned long long v = ((unsigned long long)(~key) << 32) | (uint32_t)idx;
        if (gt) keys[rg] = v;
        if (eq && re < remaining) keys[n_gt + re] = v;
        done_gt += total & 0xffffu;
        done_eq += total >> 16;
    }
    uint32_t n2 = 1;
    while (n2 < k) n2 <<= 1;
    for (uint32_t i = k + threadIdx.x; i < n2; i += SP_SEL_THREADS) keys[i] = ~0ull;
    for (uint32_t size = 2; size <= n2; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < (n2 >> 1); i += SP_SEL_THREADS) {
                const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool asc = (lo & size) == 0;
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a > b) == asc) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
        }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < k; i += SP_SEL_THREADS) {
        const unsigned long long v = keys[i];
        const uint32_t key = ~(uint32_t)(v >> 32);
        const uint32_t u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
        sp_emit(kpo, sco, i, (int32_t)(uint32_t)v, __uint_as_float(u), Ws);
    }
    if (threadIdx.x == 0) counts[t] = (int32_t)k;
}

__device__ __forceinline__ float4 sp_unit4(const float* p, int lane) {
    float4 v = *reinterpret_cast<const float4*>(p + lane * 4);
    const float n = fmaxf(sqrtf(wave_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w)), 1e-12f);
    return make_float4(v.x / n, v.y / n, v.z / n, v.w / n);
}

// one wave per (frame, slot); dmap [T,h,w,256] raw, kp [T,kcap,2], out [T,kcap,256]
__global__ __launch_bounds__(SP_THREADS) void sp_sample_kernel(const float* __restrict__ dmap, const float* __restrict__ kp,
                                                                const int32_t* __restrict__ counts, float* __restrict__ out, int h, int w,
                                                                int64_t kcap, int64_t total, float divx, float divy) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (SP_THREADS / 64) + (threadIdx.x >> 6);
    if (g >= total) return;
    const int64_t t = g / kcap;
    if (g - t * kcap >= counts[t]) return;
    // sample_descriptors with s = 8: kp - s/2 + 0.5, over (w s - s/2 - 0.5, h s - s/2 - 0.5), to [-1, 1]; grid_sample(align_corners=True) back to pixels
    const float gx = (kp[2 * g] - 4.f + 0.5f) / divx * 2.f - 1.f, gy = (kp[2 * g + 1] - 4.f + 0.5f) / divy * 2.f - 1.f;
    const float ix = (gx + 1.f) / 2.f * (float)(w - 1), iy = (gy + 1.f) / 2.f * (float)(h - 1);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float wx1 = ix - fx, wy1 = iy - fy, wx0 = (fx + 1.f) - ix, wy0 = (fy + 1.f) - iy;
    const float* base = dmap + (size_t)t * h * w * SP_C;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                        // nw, ne, sw, se: grid_sample's order
        const int xx = x0 + (j & 1), yy = y0 + (j >> 1);
        const float wt = ((j & 1) ? wx1 : wx0) * ((j >> 1) ? wy1 : wy0);
        if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;           // zeros outside; uniform over the wave
        const float4 u = sp_unit4(base + ((size_t)yy * w + xx) * SP_C, lane);
        acc.x = fmaf(u.x, wt, acc.x); acc.y = fmaf(u.y, wt, acc.y); acc.z = fmaf(u.z, wt, acc.z); acc.w = fmaf(u.w, wt, acc.w);
    }
    const float n = fmaxf(sqrtf(wave_sum(acc.x * acc.x + acc.y * acc.y + acc.z * acc.z + acc.w * acc.w)), 1e-12f);
    *reinterpret_cast<float4*>(out + (size_t)g * SP_C + lane * 4) = make_float4(acc.x / n, acc.y / n, acc.z / n, acc.w / n);
}

static bool sp_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool sp_dims_ok(int64_t T, int64_t H, int64_t W) { return T > 0 && T <= 65535 && H > 0 && W > 0 && H <= (1 << 15) && W <= (1 << 15); }
static int64_t sp_chunks(int64_t HW) { return (HW + SP_CHUNK - 1) / SP_CHUNK; }

struct SpSelLayout {
    size_t chunk_count, ncand, cand_idx, cand_score, bytes;
};
static SpSelLayout sp_sel_layout(int64_t T, int64_t HW) {
    SpSelLayout l;
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += (b + 255) & ~(size_t)255; return at; };
    l.chunk_count = take((size_t)T * sp_chunks(HW) * 4);
    l.ncand = take((size_t)T * 4);
    l.cand_idx = take((size_t)T * HW * 4);
    l.cand_score = take((size_t)T * HW * 4);
    l.bytes = o;
    return l;
}

extern "C" {

int32_t vgpa_sp_input_conv1a(const void* src, int32_t mode, const float* table, const float* w, const float* bias, float* out, float* gray, int64_t T,
                             int64_t H, int64_t W, int64_t Ho, int64_t Wo, hipStream_t stream) {
    if (!src || !w || !bias || !out || !sp_dims_ok(T, H, W) || !sp_dims_ok(T, Ho, Wo)) return VGPA_ERR_INVALID;
    if (mode != SP_MODE_RGB8 && mode != SP_MODE_GRAY_F32 && mode != SP_MODE_RGB_F32) return VGPA_ERR_INVALID;
    if ((mode == SP_MODE_RGB8) != (table != nullptr)) return VGPA_ERR_INVALID;
    if (mode != SP_MODE_RGB8 && ((uintptr_t)src & 3)) return VGPA_ERR_INVALID;
    if (!sp_aligned16(w) || !sp_aligned16(bias) || !sp_aligned16(out) || ((uintptr_t)gray & 3) || ((uintptr_t)table & 3)) return VGPA_ERR_INVALID;
    SpInArgs a = {src, table, w, bias, out, gray, mode, (int)H, (int)W, (int)Ho, (int)Wo, (float)H / (float)Ho, (float)W / (float)Wo};
    const dim3 grid((unsigned)((Wo + SP_IN_TILE - 1) / SP_IN_TILE), (unsigned)((Ho + SP_IN_TILE - 1) / SP_IN_TILE), (unsigned)T);
    VGPA_LAUNCH(sp_input_kernel, grid, dim3(SP_THREADS), 0, stream, a);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_sp_head_f32(const float* x, const float* w, const float* bias, float* score, int64_t T, int64_t h, int64_t wd, hipStream_t stream) {
    if (!x || !w || !bias || !score || !sp_dims_ok(T, h, wd) || h > 4096 || wd > 4096) return VGPA_ERR_INVALID;
    if (!sp_aligned16(x) || ((uintptr_t)w & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)score & 3)) return VGPA_ERR_INVALID;
    const int64_t cells = T * h * wd, per = (SP_THREADS / 64) * SP_HEAD_CPW, blocks = (cells + per - 1) / per;
    if (blocks > 0x7fffffffLL) return VGPA_ERR_INVALID;
    VGPA_LAUNCH(sp_head_kernel, dim3((unsigned)blocks), dim3(SP_THREADS), 0, stream, x, w, bias, score, cells, (int)h, (int)wd);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_sp_nms_f32(const float* score, float* out, int64_t T, int64_t Hs, int64_t Ws, int32_t radius, int32_t border, hipStream_t stream) {
    if (!score || !out || score == out || !sp_dims_ok(T, Hs, Ws) || radius < 1 || radius > SP_NMS_MAXR || border < 0) return VGPA_ERR_INVALID;
    if (((uintptr_t)score & 3) || ((uintptr_t)out & 3)) return VGPA_ERR_INVALID;
    const dim3 grid((unsigned)((Ws + SP_NMS_TILE - 1) / SP_NMS_TILE), (unsigned)((Hs + SP_NMS_TILE - 1) / SP_NMS_TILE), (unsigned)T);
#define SP_NMS_CASE(RAD)                                                                                             \
    case RAD:                                                                                                        \
        VGPA_LAUNCH(sp_nms_kernel<RAD>, grid, dim3(SP_THREADS), 0, stream, score, out, (int)Hs, (int)Ws, (int)border); \
        break;
    switch (radius) {
        SP_NMS_CASE(1) SP_NMS_CASE(2) SP_NMS_CASE(3) SP_NMS_CASE(4)
        default: return VGPA_ERR_INVALID;
    }
#undef SP_NMS_CASE
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

size_t vgpa_sp_select_workspace_bytes(int64_t T, int64_t Hs, int64_t Ws) {
    if (!sp_dims_ok(T, Hs, Ws)) return 0;
    return sp_sel_layout(T, Hs * Ws).bytes;
}

int32_t vgpa_sp_select(const float* nms, float threshold, int64_t T, int64_t Hs, int64_t Ws, int64_t kcap, float* kp, float* sc, int32_t* counts,
                       void* workspace, size_t ws_bytes, hipStream_t stream) {
    if (!nms || !kp || !sc || !counts || !workspace || !sp_dims_ok(T, Hs, Ws) || kcap < 1) return VGPA_ERR_INVALID;
    const int64_t HW = Hs * Ws;
    if (kcap > SP_SEL_MAXK && kcap < HW) return VGPA_ERR_INVALID;          // a cut sorts its survivors in LDS
    if (((uintptr_t)nms & 3) || ((uintptr_t)kp & 3) || ((uintptr_t)sc & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)workspace & 255)) return VGPA_ERR_INVALID;
    const SpSelLayout l = sp_sel_layout(T, HW);
    if (ws_bytes < l.bytes) return VGPA_ERR_WORKSPACE;
    char* ws = (char*)workspace;
    uint32_t* chunk_count = (uint32_t*)(ws + l.chunk_count);
    uint32_t* ncand = (uint32_t*)(ws + l.ncand);
    int32_t* cand_idx = (int32_t*)(ws + l.cand_idx);
    float* cand_score = (float*)(ws + l.cand_score);
    const int nchunks = (int)sp_chunks(HW);
    const dim3 grid((unsigned)nchunks, (unsigned)T);
    VGPA_LAUNCH(sp_count_kernel, grid, dim3(SP_THREADS), 0, stream, nms, HW, threshold, nchunks, chunk_count);
    VGPA_CHECK_LAUNCH();
    VGPA_LAUNCH(sp_compact_kernel, grid, dim3(SP_THREADS), 0, stream, nms, HW, threshold, nchunks, chunk_count, cand_idx, cand_score, ncand);
    VGPA_CHECK_LAUNCH();
    VGPA_LAUNCH(sp_select_kernel, dim3((unsigned)T), dim3(SP_SEL_THREADS), 0, stream, cand_idx, cand_score, ncand, HW, (int)Ws, kcap, kp, sc, counts);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_sp_sample_desc_f32(const float* dmap, const float* kp, const int32_t* counts, float* out, int64_t T, int64_t h, int64_t wd, int64_t kcap,
                                hipStream_t stream) {
    if (!dmap || !kp || !counts || !out || !sp_dims_ok(T, h, wd) || kcap < 1) return VGPA_ERR_INVALID;
    if (!sp_aligned16(dmap) || !sp_aligned16(out) || ((uintptr_t)kp & 3) || ((uintptr_t)counts & 3)) return VGPA_ERR_INVALID;
    const int64_t total = T * kcap, blocks = (total + SP_THREADS / 64 - 1) / (SP_THREADS / 64);
    if (blocks > 0x7fffffffLL) return VGPA_ERR_INVALID;
    const float divx = (float)((double)wd * 8 - 4 - 0.5), divy = (float)((double)h * 8 - 4 - 0.5);
    VGPA_LAUNCH(sp_sample_kernel, dim3((unsigned)blocks), dim3(SP_THREADS), 0, stream, dmap, kp, counts, out, (int)h, (int)wd, kcap, total, divx, divy);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

}  // extern "C"
