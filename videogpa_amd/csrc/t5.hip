// T5 encoder (transformers' T5EncoderModel, the CogVideoX text encoder) between its GEMMs, forward only, gfx950: videogpa_amd/t5.py.
//  * t5_attn_kernel       o = softmax(q k^T + bias[h][j - i] + mask[b][j]) v at head_dim 64: no 1/sqrt(d) scale, a learned per-head bias that depends on j - i
//                         only (a Toeplitz table, never an [H,S,S] tensor) and an optional key-padding mask.  S <= 512.
//  * t5_rms_kernel        the fp32 residual stream: x_new = x + y (or the embedding row), n = w * x_new * rsqrt(mean(x_new^2) + eps); one wave per row over row_ln.h
//  * t5_gated_gelu_kernel g = bf16(gelu_tanh(a) * b) of the two halves of the fused wi_0 | wi_1 GEMM output
#include "attn_common.h"
#include "row_ln.h"

#define T5_MAX_S 512
#define T5_LOG2E 1.4426950408889634f

// ======================================================================================================================================================
// Attention.  Conventions of attention.hip: 256 threads = 4 waves, a wave owns 32 query rows, every product is computed transposed (S^T = K Q^T,
// O^T = V^T P^T) so that the softmax row a lane works on is the MFMA column lane & 31 and the packed scores are the B operand of the PV product as they
// stand; K / V tiles of 64 rows go HBM -> registers -> LDS with the row index clamped to S - 1.
// The softmax is the exact two-pass one: a first sweep over the key tiles finds the TRUE maximum of every row (scores + bias, valid keys only), a second
// sweep forms the same scores again (the same instructions on the same operands: the same bits), p = bf16(exp(s - max)), and accumulates sum p and p v.
// No running maximum, no rescaling, no redo.  At S <= 512 the second QK^T costs 8 tiles of MFMAs at most; holding the 512 scores of a row block
// instead would take 256 accumulator registers per lane.  The row sum adds the ROUNDED weights, the ones the PV product multiplies: o is an exact convex
// combination of v rows (tests/attn_tol.py, "normalised by the rounded sum").
// Scores, the bias add and the softmax are fp32.  A masked key, and a key of the ragged last tile, gets the score -inf by selection (not by addition:
// whatever k holds there, NaN included, does not reach the row) and so the weight exactly 0.  PRECONDITION: every sample keeps at least one key (the
// tokenizer always emits EOS); a sample without one has no row maximum and its rows come out NaN.
// ======================================================================================================================================================
__device__ __forceinline__ void t5_scores(const bf16_t* kl, int kb, int lane, int hi, const bf16x8_t (&qf)[4], const float* biasq, const float* keep,
                                          int key0, int S, f32x16_t& s) {
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) s = mfma32(frag_row(kl, kb * 32, ks, lane), qf[ks], s);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int j = key0 + kb * 32 + acc_row(r, hi);          // < 64 * ceil(S / 64) <= T5_MAX_S: inside `keep`
        const float t = s[r] + biasq[j < S ? j : S - 1];        // one fp32 addition per score
        s[r] = keep[j] != 0.f ? t : -INFINITY;
    }
}

__global__ __launch_bounds__(256) void t5_attn_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
                                                      const float* __restrict__ bias_delta, const uint8_t* __restrict__ mask, bf16_t* __restrict__ O,
                                                      TStride sq, TStride sk, TStride sv, TStride so, int S, int H, int n_qt) {
    __shared__ __attribute__((aligned(16))) bf16_t lds[2 * TILE_ELEMS];   // one K tile, one V tile
    __shared__ float bias_l[2 * T5_MAX_S];                                // bias_delta[h]: 2 S - 1 entries, index j - i + S - 1
    __shared__ float keep[T5_MAX_S];                                      // 1 for a key that takes part, 0 for a masked one or one past S
    const int bh = blockIdx.x / n_qt, qt = blockIdx.x % n_qt;
    const int b = bh / H, h = bh % H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5;
    const int q0 = (qt * 4 + wave) * 32;
    const int nt = (S + TILE - 1) / TILE;

    const bf16_t* Qb = Q + ((size_t)b * sq.b + (size_t)h * sq.h);
    const bf16_t* Kb = K + ((size_t)b * sk.b + (size_t)h * sk.h);
    const bf16_t* Vb = V + ((size_t)b * sv.b + (size_t)h * sv.h);
    bf16_t* const kl = lds;
    bf16_t* const vl = lds + TILE_ELEMS;

    for (int i = threadIdx.x; i < 2 * S - 1; i += 256) bias_l[i] = bias_delta[(size_t)h * (2 * S - 1) + i];
    for (int j = threadIdx.x; j < nt * TILE; j += 256) keep[j] = (j < S && (!mask || mask[(size_t)b * S + j] != 0)) ? 1.f : 0.f;

    bf16x8_t qf[4];
    load_row_frags(Qb, sq.s, q0, S, lane, qf);                  // rows past S - 1 read row S - 1 and are not stored
    const int q = q0 + (lane & 31);
    const float* biasq = bias_l + (S - 1 - (q < S ? q : S - 1));   // biasq[j] = bias[h][j - q + S - 1], j in [0, S)

    u32x4_t kr[2], vr[2];
    f32x16_t s;
    // pass 1: the row maximum
    float mx = -INFINITY;
    for (int t = 0; t < nt; ++t) {
        tile_load(Kb, sk.s, t * TILE, S, kr);
        __syncthreads();                                        // the tile before has been read by every wave (t = 0: nothing to wait for)
        tile_store(kl, kr);
        __syncthreads();                                        // also behind the bias_l / keep staging
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            t5_scores(kl, kb, lane, hi, qf, biasq, keep, t * TILE, S, s);
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[r]);
        }
    }
    mx = fmaxf(mx, other_half(mx));

    // pass 2: weights against the true maximum, their sum, and P V
    f32x16_t o[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) { o[0][i] = 0.f; o[1][i] = 0.f; }
    float l = 0.f;
    for (int t = 0; t < nt; ++t) {
        tile_load(Kb, sk.s, t * TILE, S, kr);
        tile_load(Vb, sv.s, t * TILE, S, vr);
        __syncthreads();
        tile_store(kl, kr);
        tile_store(vl, vr);
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            t5_scores(kl, kb, lane, hi, qf, biasq, keep, t * TILE, S, s);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = round_bf16(__builtin_amdgcn_exp2f((s[r] - mx) * T5_LOG2E));      // exp2(-inf) = 0: a masked key weighs nothing
                l += s[r];
            }
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const bf16x8_t pf = pack_frag(s, 8 * cc);       // exact: the values are bf16 already
#pragma unroll
                for (int db = 0; db < 2; ++db) o[db] = mfma32(frag_tr(vl, kb * 32 + 16 * cc, db * 32, lane), pf, o[db]);
            }
        }
    }
    const float inv = 1.f / (l + other_half(l));
    if (q < S) {
        bf16_t* op = O + ((size_t)b * so.b + (size_t)h * so.h + (size_t)q * so.s);
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                u32x2_t w;
                w[0] = pack_bf16x2(o[db][4 * g] * inv, o[db][4 * g + 1] * inv);
                w[1] = pack_bf16x2(o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv);
                *reinterpret_cast<u32x2_t*>(op + db * 32 + 8 * g + 4 * hi) = w;
            }
    }
}

// ======================================================================================================================================================
// The residual stream, one wave per row (row_ln.h: chunk c of lane l holds elements (c * 64 + l) * 8 .. + 7), rows taken grid-stride.
//   MODE 0   x_new = x                          (nothing written for it)
//   MODE 1   x_new = x + y                      y bf16, the GEMM output in front; written when x_new is given (never in place)
//   MODE 2   x_new = float(table[ids[row]])     the embedding gather; an id outside [0, V) gives a row of NaN and reads nothing
//   n = w * x_new * rsqrt(mean(x_new^2) + eps)  T5LayerNorm: no mean subtraction, no bias; stored as bf16 or fp32, rounded once
// ======================================================================================================================================================
#define T5_ROW_WAVES 4
#define T5_ROW_MAX_BLOCKS 2048

template <int NV, int MODE>
__global__ __launch_bounds__(64 * T5_ROW_WAVES) void t5_rms_kernel(const float* __restrict__ x, const bf16_t* __restrict__ y, const int64_t* __restrict__ ids,
                                                                   const bf16_t* __restrict__ table, int64_t V, const float* __restrict__ w, float eps, int D,
                                                                   int64_t M, float* x_new, void* __restrict__ n, int n_bf16) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * T5_ROW_WAVES + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * T5_ROW_WAVES) {
        float v[NV][8];
        if (MODE == 2) {
            const int64_t id = ids[row];
            const bool ok = id >= 0 && id < V;
            Raw8<VGPA_DTYPE_BF16> tr[NV];                       // the row's loads first (common.h Raw8)
#pragma unroll
            for (int c = 0; c < NV; ++c) tr[c].load(table, (size_t)(ok ? id : 0) * D + (c * 64 + lane) * 8, ok && (c * 64 + lane) * 8 < D);
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                tr[c].get(v[c]);
                if (!ok) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[c][j] = __builtin_nanf("");
                }
            }
        } else {
            Raw8<VGPA_DTYPE_F32> xr[NV];
            Raw8<VGPA_DTYPE_BF16> yr[MODE == 1 ? NV : 1];
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const int i0 = (c * 64 + lane) * 8;
                xr[c].load(x, (size_t)row * D + i0, i0 < D);
                if (MODE == 1) yr[c].load(y, (size_t)row * D + i0, i0 < D);
            }
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                xr[c].get(v[c]);
                if (MODE == 1) {
                    float yv[8];
                    yr[c].get(yv);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[c][j] += yv[j];
                }
            }
        }
        float sq = 0.f;
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const int i0 = (c * 64 + lane) * 8;
            if (i0 < D) {
                if (MODE != 0 && x_new) store8<VGPA_DTYPE_F32>(x_new, (size_t)row * D + i0, v[c]);
#pragma unroll
                for (int j = 0; j < 8; ++j) sq += v[c][j] * v[c][j];
            }
        }
        const float rs = rsqrtf(wave_sum(sq) / (float)D + eps);
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const int i0 = (c * 64 + lane) * 8;
            if (i0 < D) {
                float wv[8], o[8];
                load8<VGPA_DTYPE_F32>(w, (size_t)i0, wv);       // an L2 hit, shared by every row
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (v[c][j] * rs) * wv[j];
                if (n_bf16) store8<VGPA_DTYPE_BF16>(n, (size_t)row * D + i0, o);
                else store8<VGPA_DTYPE_F32>(n, (size_t)row * D + i0, o);
            }
        }
    }
}

template <int NV>
static void t5_rms_launch(int mode, dim3 grid, hipStream_t stream, const float* x, const bf16_t* y, const int64_t* ids, const bf16_t* table, int64_t V,
                          const float* w, float eps, int D, int64_t M, float* x_new, void* n, int n_bf16) {
    if (mode == 0) VGPA_LAUNCH((t5_rms_kernel<NV, 0>), grid, dim3(64 * T5_ROW_WAVES), 0, stream, x, y, ids, table, V, w, eps, D, M, x_new, n, n_bf16);
    else if (mode == 1) VGPA_LAUNCH((t5_rms_kernel<NV, 1>), grid, dim3(64 * T5_ROW_WAVES), 0, stream, x, y, ids, table, V, w, eps, D, M, x_new, n, n_bf16);
    else VGPA_LAUNCH((t5_rms_kernel<NV, 2>), grid, dim3(64 * T5_ROW_WAVES), 0, stream, x, y, ids, table, V, w, eps, D, M, x_new, n, n_bf16);
}

// ======================================================================================================================================================
// T5DenseGatedActDense between its GEMMs: u [M, 2F] = n (wi_0 | wi_1)^T, g[m, f] = bf16(gelu_new(u[m, f]) * u[m, F + f]).  gelu_new is the tanh form
// (common.h gelu_sig); the product is formed in fp32 from the two bf16 values and rounded once.  Eight elements per thread, grid-stride.
// ======================================================================================================================================================
__global__ __launch_bounds__(256) void t5_gated_gelu_kernel(const bf16_t* __restrict__ u, bf16_t* __restrict__ g, int64_t total /* M * F / 8 */, int F8) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t m = i / F8;
        const int c = (int)(i - m * F8);
        const size_t ia = ((size_t)m * 2 * F8 + c) * 8;
        float a[8], bb[8], o[8];
        load8<VGPA_DTYPE_BF16>(u, ia, a);
        load8<VGPA_DTYPE_BF16>(u, ia + (size_t)F8 * 8, bb);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = gelu_tanh_value(a[j]) * bb[j];
        store8<VGPA_DTYPE_BF16>(g, (size_t)i * 8, o);
    }
}

extern "C" {

int32_t vgpa_t5_attn_fwd(const void* q, const void* k, const void* v, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                         const float* bias_delta, const uint8_t* mask, void* o, int64_t B, int64_t H, int64_t S, hipStream_t stream) {
    if (!q || !k || !v || !bias_delta || !o || B <= 0 || H <= 0 || S <= 0 || S > T5_MAX_S) return VGPA_ERR_INVALID;
    if (!view_ok(q_strides, B, H, S, HD) || !view_ok(k_strides, B, H, S, HD) || !view_ok(v_strides, B, H, S, HD) || !al16(q) || !al16(k) || !al16(v) || !al16(o))
        return VGPA_ERR_INVALID;
    const int64_t o_strides[3] = {S * H * HD, HD, H * HD};                   // o [B, S, H * 64] contiguous
    const int n_qt = (int)((S + WG_ROWS - 1) / WG_ROWS);
    if (!range_ok(o_strides, B, H, S, HD) || B * H * n_qt > 0x7fffffff) return VGPA_ERR_INVALID;
    VGPA_LAUNCH(t5_attn_kernel, dim3((unsigned)(B * H * n_qt)), dim3(256), 0, stream, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, bias_delta, mask,
                (bf16_t*)o, mk(q_strides), mk(k_strides), mk(v_strides), mk(o_strides), (int)S, (int)H, n_qt);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_t5_rms(const float* x, const void* y, const int64_t* ids, const void* table, int64_t V, const float* w, float* x_new, void* n, int32_t n_dtype,
                    int64_t M, int64_t D, float eps, hipStream_t stream) {
    if (!w || !n || M <= 0 || D <= 0 || D > 4096 || D % 64 || (n_dtype != VGPA_DTYPE_F32 && n_dtype != VGPA_DTYPE_BF16)) return VGPA_ERR_INVALID;
    int mode;
    if (ids) {                                                               // the embedding gather writes the stream
        if (!table || V <= 0 || x || y || !x_new) return VGPA_ERR_INVALID;
        mode = 2;
    } else {
        if (!x || table) return VGPA_ERR_INVALID;
        if (!y && x_new) return VGPA_ERR_INVALID;                            // nothing to write without the add
        mode = y ? 1 : 0;
    }
    if ((const void*)x_new == (const void*)n || (const void*)x == (const void*)n || (x && x_new == x)) return VGPA_ERR_INVALID;
    const int64_t blocks = (M + T5_ROW_WAVES - 1) / T5_ROW_WAVES;
    const dim3 grid((unsigned)(blocks < T5_ROW_MAX_BLOCKS ? blocks : T5_ROW_MAX_BLOCKS));
    ROW_DISPATCH_NV(D, (t5_rms_launch<NV>(mode, grid, stream, x, (const bf16_t*)y, ids, (const bf16_t*)table, V, w, eps, (int)D, M, x_new, n,
                                          n_dtype == VGPA_DTYPE_BF16)));
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_t5_gated_gelu(const void* u, void* g, int64_t M, int64_t d_ff, hipStream_t stream) {
    if (!u || !g || u == g || M <= 0 || d_ff <= 0 || d_ff % 8 || d_ff > (1 << 24) || !al16(u) || !al16(g)) return VGPA_ERR_INVALID;
    const int64_t total = M * (d_ff / 8);
    const int64_t blocks = (total + 255) / 256;
    VGPA_LAUNCH(t5_gated_gelu_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, stream, (const bf16_t*)u, (bf16_t*)g, total, (int)(d_ff / 8));
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

}  // extern "C"
