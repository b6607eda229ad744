// LightGlue (cvg/LightGlue, features="superpoint") between its GEMMs, forward only, gfx950: videogpa_amd/lightglue.py.
//  * lg_attn_kernel        softmax(q k^T / 8) v at head_dim 64, separate query and key lengths per sample, fp32 operands read in place by element
//                          strides, rotary and scale in the loader, fp16 MFMA with fp32 accumulators, fp32 online softmax; two directions per launch
//  * lg_posenc_kernel      keypoint normalisation and the cos / sin tables of the learnable Fourier encoding
//  * lg_ln_gelu_kernel     LayerNorm(512) -> erf GELU between the two ffn GEMMs (row_ln.h), and the last ffn bias added to the residual stream
//  * lg_confidence_kernel  sigmoid(w . x + b) per row (token confidence, matchability) and the per-sample count of rows below a threshold
//  * lg_prune_kernel       keep mask, ordered compaction of descriptors, rotary tables and the index vector, prune[ind] += 1, the new counts
//  * lg_assign_*           log-sum-exps of sim by row and column, argmax of the combined log score, mutual check, threshold, ordered match list
// Variable-length form: a sample owns R rows of every activation; rows [0, S0) are image 0 with count c0[b], rows [S0, R) image 1 with count c1[b]
// (c1 == NULL: one segment, S0 == R).  Rows at or past a count are never read as keys and never written.  Every per-sample result is a function of that
// sample's rows and counts alone: no reduction crosses samples, no order depends on B or R, no float atomics (the only atomics add integers).
#include "attn_common.h"
#include "row_ln.h"

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;

#define LG_MAX_N 4096
#define LG_D 256
#define LG_LOG2E 1.4426950408889634f

__device__ __forceinline__ uint32_t lg_pack_f16x2(float lo, float hi) {          // round-to-nearest-even, as torch's float -> half cast
    const f16x2_t h = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(uint32_t, h);
}
__device__ __forceinline__ float lg_round_f16(float f) { return (float)(_Float16)f; }
__device__ __forceinline__ f32x16_t lg_mfma(bf16x8_t a, f16x8_t b, f32x16_t c) {  // the LDS helpers of mfma_tiles.h move 16-bit words: the bits are fp16 here
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), b, c, 0, 0, 0);
}
__device__ __forceinline__ int lg_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// segment of row r of sample b: its index inside the segment and whether it is below the segment's count
__device__ __forceinline__ bool lg_row_valid(int b, int r, int S0, int R, const int32_t* c0, const int32_t* c1) {
    if (r < S0) return r < lg_clampi(c0[b], 0, S0);
    return c1 && (r - S0) < lg_clampi(c1[b], 0, R - S0);
}

// ======================================================================================================================================================
// Attention.  Conventions of t5.hip / attention.hip: 256 threads = 4 waves, a wave owns 32 query rows, both products are computed transposed
// (S^T = K Q^T, O^T = V^T P^T) so that a lane's softmax row is the MFMA column lane & 31 and the packed weights are the B operand of the PV product as
// they stand.  K / V tiles of 64 keys go HBM (fp32, strided) -> registers -> LDS (fp16); the loader applies the rotary rotation of adjacent pairs
// (x0, x1) -> (x0 c - x1 s, x1 c + x0 s) and q_premul in fp32 and rounds once.  Key rows are clamped to nk - 1 on load and a key at or past nk gets the
// score -inf by selection, so whatever the padding holds never reaches a row.  Online softmax in fp32 (base 2): every tile holds at least one valid key,
// so the running maximum is finite from the first tile on; the weights are rounded to fp16, and the row sum adds the ROUNDED weights, the ones the PV
// product multiplies.  blockIdx.z is the direction: the two directions of the cross block, or the two images of the self block, are one launch.
// ======================================================================================================================================================
struct LgDir {
    const float *q, *k, *v;
    float* o;
    const int32_t *nq, *nk;
    const float *qcos, *qsin, *kcos, *ksin;      // [B][rows][32] by batch stride, or NULL
    int64_t q_b, q_h, q_t, k_b, k_h, k_t, v_b, v_h, v_t, o_b, o_t, rq_b, rk_b;
    int32_t nq_max, nk_max;
};
struct LgAttnArgs {
    LgDir d[2];
    float q_premul;
    int H;
};

__device__ __forceinline__ void lg_rope8(float* x, const float* c, const float* s) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a = x[2 * i], b = x[2 * i + 1];
        x[2 * i] = a * c[i] - b * s[i];
        x[2 * i + 1] = b * c[i] + a * s[i];
    }
}

// one thread's share of a 64-key tile: key row tid >> 2, dims (tid & 3) * 16 .. + 15 of k and v, and the row's rotary entries for those dims
template <int DS>
struct LgTileRegs {
    float k[16], v[16], c[8], s[8];
    __device__ __forceinline__ void load(const float* Kb, const float* Vb, const float* cosb, const float* sinb, int64_t k_t, int64_t v_t, int key0, int nk) {
        int row = key0 + (int)(threadIdx.x >> 2);
        row = row < nk ? row : nk - 1;
        const int d0 = (threadIdx.x & 3) * 16;
        const float* kp = Kb + (int64_t)row * k_t + (int64_t)d0 * DS;
        const float* vp = Vb + (int64_t)row * v_t + (int64_t)d0 * DS;
#pragma unroll
        for (int j = 0; j < 16; ++j) { k[j] = kp[j * DS]; v[j] = vp[j * DS]; }
        if (cosb) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { c[j] = cosb[(int64_t)row * 32 + d0 / 2 + j]; s[j] = sinb[(int64_t)row * 32 + d0 / 2 + j]; }
        }
    }
    __device__ __forceinline__ void store(uint16_t* kl, uint16_t* vl, bool rope, float premul) {
        if (rope) { lg_rope8(k, c, s); lg_rope8(k + 8, c + 4, s + 4); }
        const int off = (int)(threadIdx.x >> 2) * PITCH + (int)(threadIdx.x & 3) * 16;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            u32x4_t kw, vw;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                kw[j] = lg_pack_f16x2(k[8 * g + 2 * j] * premul, k[8 * g + 2 * j + 1] * premul);
                vw[j] = lg_pack_f16x2(v[8 * g + 2 * j], v[8 * g + 2 * j + 1]);
            }
            *reinterpret_cast<u32x4_t*>(kl + off + 8 * g) = kw;
            *reinterpret_cast<u32x4_t*>(vl + off + 8 * g) = vw;
        }
    }
};

template <int DS>
__global__ __launch_bounds__(256) void lg_attn_kernel(LgAttnArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * TILE_ELEMS];   // one K tile, one V tile (fp16 bits)
    const LgDir& d = a.d[blockIdx.z];
    const int b = blockIdx.y / a.H, h = blockIdx.y % a.H;
    const int nq = lg_clampi(d.nq[b], 0, d.nq_max), nk = lg_clampi(d.nk[b], 0, d.nk_max);
    if ((int)blockIdx.x * WG_ROWS >= nq) return;                             // uniform: the whole workgroup leaves
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5;
    const int q0 = (blockIdx.x * 4 + wave) * 32;
    const int q = q0 + (lane & 31);
    float* op = d.o + ((int64_t)b * d.o_b + (int64_t)q * d.o_t + h * HD);
    if (nk == 0) {                                                           // no key: the rows are defined as 0
        if (q < nq) {
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4_t*>(op + db * 32 + 8 * g + 4 * hi) = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        return;
    }
    const float* Kb = d.k + ((int64_t)b * d.k_b + (int64_t)h * d.k_h);
    const float* Vb = d.v + ((int64_t)b * d.v_b + (int64_t)h * d.v_h);
    const float* kcos = d.kcos ? d.kcos + (int64_t)b * d.rk_b : nullptr;
    const float* ksin = d.kcos ? d.ksin + (int64_t)b * d.rk_b : nullptr;
    uint16_t* const kl = lds;
    uint16_t* const vl = lds + TILE_ELEMS;
    const int nt = (nk + TILE - 1) / TILE;

    LgTileRegs<DS> tr;
    tr.load(Kb, Vb, kcos, ksin, d.k_t, d.v_t, 0, nk);

    // the wave's query fragments: lane (row = lane & 31, hi) holds dims ks * 16 + 8 hi .. + 7 of its row for the four k-steps
    f16x8_t qf[4];
    {
        const int qr = q < nq ? q : nq - 1;
        const float* qp = d.q + ((int64_t)b * d.q_b + (int64_t)h * d.q_h + (int64_t)qr * d.q_t);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int d0 = ks * 16 + hi * 8;
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = qp[(int64_t)(d0 + j) * DS];
            if (d.qcos) {
                float c[4], s[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    c[j] = d.qcos[(int64_t)b * d.rq_b + (int64_t)qr * 32 + d0 / 2 + j];
                    s[j] = d.qsin[(int64_t)b * d.rq_b + (int64_t)qr * 32 + d0 / 2 + j];
                }
                lg_rope8(x, c, s);
            }
            u32x4_t w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = lg_pack_f16x2(x[2 * j] * a.q_premul, x[2 * j + 1] * a.q_premul);
            qf[ks] = __builtin_bit_cast(f16x8_t, w);
        }
    }

    f32x16_t o[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) { o[0][i] = 0.f; o[1][i] = 0.f; }
    float mx = -INFINITY, l = 0.f;
    const float sc = 0.125f * LG_LOG2E;                                      // 1 / sqrt(64), scores kept in base 2
    for (int t = 0; t < nt; ++t) {
        __syncthreads();                                                     // the tile before has been read by every wave
        tr.store(kl, vl, kcos != nullptr, a.q_premul);
        __syncthreads();
        if (t + 1 < nt) tr.load(Kb, Vb, kcos, ksin, d.k_t, d.v_t, (t + 1) * TILE, nk);
        f32x16_t s[2];
        float tmax = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[kb][i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) s[kb] = lg_mfma(frag_row(kl, kb * 32, ks, lane), qf[ks], s[kb]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = t * TILE + kb * 32 + acc_row(r, hi);
                s[kb][r] = j < nk ? s[kb][r] * sc : -INFINITY;
                tmax = fmaxf(tmax, s[kb][r]);
            }
        }
        tmax = fmaxf(tmax, other_half(tmax));                                // both lanes of a pair hold the same query row: one maximum
        const float mnew = fmaxf(mx, tmax);                                  // finite: key t * 64 of the tile is valid
        const float alpha = __builtin_amdgcn_exp2f(mx - mnew);               // exp2(-inf) = 0 at the first tile
        mx = mnew;
        l *= alpha;
#pragma unroll
        for (int i = 0; i < 16; ++i) { o[0][i] *= alpha; o[1][i] *= alpha; }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[kb][r] = lg_round_f16(__builtin_amdgcn_exp2f(s[kb][r] - mx));   // a masked key weighs exactly 0
                l += s[kb][r];
            }
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                u32x4_t w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = lg_pack_f16x2(s[kb][8 * cc + 2 * j], s[kb][8 * cc + 2 * j + 1]);   // exact: fp16 values already
                const f16x8_t pf = __builtin_bit_cast(f16x8_t, w);
#pragma unroll
                for (int db = 0; db < 2; ++db) o[db] = lg_mfma(frag_tr(reinterpret_cast<const bf16_t*>(vl), kb * 32 + 16 * cc, db * 32, lane), pf, o[db]);
            }
        }
    }
    const float inv = 1.f / (l + other_half(l));
    if (q < nq) {
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<f32x4_t*>(op + db * 32 + 8 * g + 4 * hi) =
                    f32x4_t{o[db][4 * g] * inv, o[db][4 * g + 1] * inv, o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv};
    }
}

// ======================================================================================================================================================
// Positional encoding.  grid (ceil(N / 64), B): every block forms the sample's normalisation again (image_size, or 1 + max - min over the sample's own
// keypoints: min and max do not depend on the order), then 64 rows x 32 frequencies: p = Wr[f][0] x + Wr[f][1] y, cosf / sinf at full precision.
// ======================================================================================================================================================
__global__ __launch_bounds__(256) void lg_posenc_kernel(const float* __restrict__ kp, const int32_t* __restrict__ counts, const float* __restrict__ image_size,
                                                        const float* __restrict__ Wr, float* __restrict__ cs, float* __restrict__ sn, int N, int64_t out_b) {
    __shared__ float red[4][4];
    const int b = blockIdx.y;
    const int n = lg_clampi(counts[b], 0, N);
    if ((int)blockIdx.x * 64 >= n) return;
    const float* kb = kp + (int64_t)b * N * 2;
    float sx, sy;
    if (image_size) {
        sx = image_size[2 * b];
        sy = image_size[2 * b + 1];
    } else {
        float lox = INFINITY, loy = INFINITY, hix = -INFINITY, hiy = -INFINITY;
        for (int i = threadIdx.x; i < n; i += 256) {
            const float x = kb[2 * i], y = kb[2 * i + 1];
            lox = fminf(lox, x); hix = fmaxf(hix, x); loy = fminf(loy, y); hiy = fmaxf(hiy, y);
        }
        lox = -wave_max(-lox); loy = -wave_max(-loy); hix = wave_max(hix); hiy = wave_max(hiy);
        const int wid = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { red[wid][0] = lox; red[wid][1] = loy; red[wid][2] = hix; red[wid][3] = hiy; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) { lox = fminf(lox, red[w][0]); loy = fminf(loy, red[w][1]); hix = fmaxf(hix, red[w][2]); hiy = fmaxf(hiy, red[w][3]); }
        sx = 1.f + hix - lox;
        sy = 1.f + hiy - loy;
    }
    const float shx = sx / 2.f, shy = sy / 2.f, scale = fmaxf(sx, sy) / 2.f;
    const int f = threadIdx.x & 31;
    const float w0 = Wr[2 * f], w1 = Wr[2 * f + 1];
    for (int rr = threadIdx.x >> 5; rr < 64; rr += 8) {
        const int i = blockIdx.x * 64 + rr;
        if (i >= n) break;
        const float x = (kb[2 * i] - shx) / scale, y = (kb[2 * i + 1] - shy) / scale;
        const float p = x * w0 + y * w1;
        cs[(int64_t)b * out_b + (int64_t)i * 32 + f] = cosf(p);
        sn[(int64_t)b * out_b + (int64_t)i * 32 + f] = sinf(p);
    }
}

// ======================================================================================================================================================
// Row kernels, one wave per row, rows taken grid-stride over B * R.
// ======================================================================================================================================================
#define LG_ROW_WAVES 4
#define LG_ROW_MAX_BLOCKS 2048

// h = gelu_erf(LayerNorm_512(u)) (two-pass variance: row_ln.h), and, when resid is given, resid[row][0..255] += rbias: the bias of the GEMM that follows,
// which then accumulates into the residual stream in place
__global__ __launch_bounds__(64 * LG_ROW_WAVES) void lg_ln_gelu_kernel(const float* __restrict__ u, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                       float eps, float* __restrict__ hout, float* resid, int64_t resid_stride,
                                                                       const float* __restrict__ rbias, int B, int R, int S0, const int32_t* __restrict__ c0,
                                                                       const int32_t* __restrict__ c1) {
    const int lane = threadIdx.x & 63;
    const int64_t M = (int64_t)B * R;
    for (int64_t row = (int64_t)blockIdx.x * LG_ROW_WAVES + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * LG_ROW_WAVES) {
        if (!lg_row_valid((int)(row / R), (int)(row % R), S0, R, c0, c1)) continue;
        float v[8], g[8], bt[8], o[8];
        load8<VGPA_DTYPE_F32>(u, (size_t)row * 512 + lane * 8, v);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += v[j];
        const float mean = wave_sum(sum) / 512.f;
        float sq = 0.f;
        ln_sqdev_acc8(v, mean, sq);
        const float rstd = rsqrtf(wave_sum(sq) / 512.f + eps);
        load8<VGPA_DTYPE_F32>(gamma, (size_t)lane * 8, g);
        load8<VGPA_DTYPE_F32>(beta, (size_t)lane * 8, bt);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float y = (v[j] - mean) * rstd * g[j] + bt[j];
            o[j] = 0.5f * y * (1.f + erff(y * 0.70710678118654752440f));
        }
        store8<VGPA_DTYPE_F32>(hout, (size_t)row * 512 + lane * 8, o);
        if (resid) {
            f32x4_t* rp = reinterpret_cast<f32x4_t*>(resid + (size_t)row * resid_stride + lane * 4);
            const f32x4_t bb = *reinterpret_cast<const f32x4_t*>(rbias + lane * 4);
            f32x4_t x = *rp;
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] += bb[j];
            *rp = x;
        }
    }
}

__device__ __forceinline__ float lg_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// z = w . x + b over 256 features, conf = sigmoid(z); below[b] += (conf < thr), the comparison in double (thr is what the reference compares against)
__global__ __launch_bounds__(64 * LG_ROW_WAVES) void lg_confidence_kernel(const float* __restrict__ x, int64_t x_stride, const float* __restrict__ w, float bias,
                                                                          float* __restrict__ conf, float* __restrict__ z_out, double thr,
                                                                          int32_t* __restrict__ below, int B, int R, int S0, const int32_t* __restrict__ c0,
                                                                          const int32_t* __restrict__ c1) {
    const int lane = threadIdx.x & 63;
    const int64_t M = (int64_t)B * R;
    const f32x4_t wv = *reinterpret_cast<const f32x4_t*>(w + lane * 4);
    for (int64_t row = (int64_t)blockIdx.x * LG_ROW_WAVES + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * LG_ROW_WAVES) {
        const int b = (int)(row / R);
        if (!lg_row_valid(b, (int)(row % R), S0, R, c0, c1)) continue;
        const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(x + (size_t)row * x_stride + lane * 4);
        float acc = xv[0] * wv[0];
        acc += xv[1] * wv[1];
        acc += xv[2] * wv[2];
        acc += xv[3] * wv[3];
        const float z = wave_sum(acc) + bias;
        const float c = lg_sigmoid(z);
        if (lane == 0) {
            if (conf) conf[row] = c;
            if (z_out) z_out[row] = z;
            if (below && (double)c < thr) atomicAdd(below + b, 1);           // an integer count: exact in any order
        }
    }
}

// block-wide exclusive scan of one count per thread (256 threads); *total = the block's sum
__device__ __forceinline__ uint32_t lg_block_exscan(uint32_t v, uint32_t* smem /* >= 4 */, uint32_t* total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
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
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < wid) base += smem[i];
        tot += smem[i];
    }
    *total = tot;
    return base + inc - v;
}

// ======================================================================================================================================================
// Pruning.  grid (B, segments): one workgroup walks its segment in chunks of 256 rows, in order.  A segment with more than prune_min rows keeps row i iff
// match[i] > thr_keep or conf[i] <= thr_conf (doubles); one with fewer keeps everything and leaves `prune` alone.  Kept rows go, in order, to the front of
// the segment in the OUTPUT buffers (never in place): x (256 of a row), the rotary tables, ind; prune[b][ind] += 1 for the kept rows of a pruned segment
// (ind is injective: a plain add); counts_out = the number kept.
// ======================================================================================================================================================
__global__ __launch_bounds__(256) void lg_prune_kernel(const float* __restrict__ conf, const float* __restrict__ match, double thr_conf, double thr_keep,
                                                       int prune_min, const float* __restrict__ x_in, float* __restrict__ x_out, int64_t x_stride,
                                                       const float* __restrict__ cos_in, const float* __restrict__ sin_in, float* __restrict__ cos_out,
                                                       float* __restrict__ sin_out, const int32_t* __restrict__ ind_in, int32_t* __restrict__ ind_out,
                                                       int32_t* __restrict__ prune0, int32_t* __restrict__ prune1, int P0, int P1, int R, int S0,
                                                       const int32_t* __restrict__ c0, const int32_t* __restrict__ c1, int32_t* __restrict__ c0_out,
                                                       int32_t* __restrict__ c1_out, uint8_t* __restrict__ keep_out) {
    __shared__ uint32_t red[4];
    __shared__ int32_t src_of[256];
    const int b = blockIdx.x, seg = blockIdx.y;
    const int r0 = seg ? S0 : 0, cap = seg ? R - S0 : S0;
    const int n = lg_clampi((seg ? c1 : c0)[b], 0, cap);
    const bool pruning = n > prune_min;
    int32_t* prune = seg ? prune1 : prune0;
    const int P = seg ? P1 : P0;
    const int64_t base = (int64_t)b * R + r0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t done = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        bool keep = false;
        if (i < n) keep = !pruning || (double)match[base + i] > thr_keep || (double)conf[base + i] <= thr_conf;
        uint32_t total;
        const uint32_t off = lg_block_exscan(keep ? 1u : 0u, red, &total);
        if (i < n && keep_out) keep_out[base + i] = keep ? 1 : 0;
        if (keep) {
            src_of[off] = i;
            const int32_t id = ind_in[base + i];
            ind_out[base + done + off] = id;
            if (pruning && id >= 0 && id < P) prune[(int64_t)b * P + id] += 1;
        }
        __syncthreads();
        for (uint32_t k = wave; k < total; k += 4) {
            const int64_t s = base + src_of[k], dd = base + done + k;
            *reinterpret_cast<f32x4_t*>(x_out + dd * x_stride + lane * 4) = *reinterpret_cast<const f32x4_t*>(x_in + s * x_stride + lane * 4);
            if (lane < 8) *reinterpret_cast<f32x4_t*>(cos_out + dd * 32 + lane * 4) = *reinterpret_cast<const f32x4_t*>(cos_in + s * 32 + lane * 4);
            else if (lane < 16) *reinterpret_cast<f32x4_t*>(sin_out + dd * 32 + (lane - 8) * 4) = *reinterpret_cast<const f32x4_t*>(sin_in + s * 32 + (lane - 8) * 4);
        }
        done += total;
        __syncthreads();                                                     // src_of is rewritten by the next chunk
    }
    if (threadIdx.x == 0) (seg ? c1_out : c0_out)[b] = (int32_t)done;
}

// ======================================================================================================================================================
// Assignment.  sim [B][Mmax][Nmax] (the vendor GEMM's md0 md1^T), z0 [B][Mmax], z1 [B][Nmax] the matchability logits, counts m[b], n[b].
//   log score  S[i][j] = ((sim - rmax_i) - rlog_i) + ((sim - cmax_j) - clog_j) + (logsigmoid(z0_i) + logsigmoid(z1_j)),  log_softmax as torch forms it
//   stage 1: rmax / rlog by row (one wave per row) and cmax / clog by column (64 columns x 4 row groups per workgroup, the groups combined in order)
//   stage 2: the maximum of S and its index by row and by column.  TIES GO TO THE LOWEST INDEX, as torch.max does on the CPU.
//   stage 3: mutual check, exp, the threshold (double), matches0 / matches1 / matching_scores0 / matching_scores1 (scattered through ind0 / ind1 when
//            pruning ran) and the ordered list of valid (i, j) with its count.
// ======================================================================================================================================================
__device__ __forceinline__ float lg_logsigmoid(float z) { return fminf(z, 0.f) - log1pf(expf(-fabsf(z))); }

__device__ __forceinline__ void lg_argmax_merge(float& v, int& idx, float ov, int oidx) {
    if (ov > v || (ov == v && oidx < idx)) { v = ov; idx = oidx; }
}

// MODE 0: log-sum-exp (out_a = max, out_b = log sum exp(. - max)).  MODE 1: max / argmax of S (out_a = max, out_i = index).
template <int MODE>
__global__ __launch_bounds__(256) void lg_assign_rows_kernel(const float* __restrict__ sim, const float* __restrict__ z0, const float* __restrict__ z1,
                                                             const int32_t* __restrict__ mc, const int32_t* __restrict__ nc, int B, int Mmax, int Nmax,
                                                             float* __restrict__ rmax, float* __restrict__ rlog, const float* __restrict__ cmax,
                                                             const float* __restrict__ clog, float* __restrict__ best, int32_t* __restrict__ arg) {
    const int lane = threadIdx.x & 63;
    const int64_t rows = (int64_t)B * Mmax;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        const int b = (int)(row / Mmax), i = (int)(row % Mmax);
        const int m = lg_clampi(mc[b], 0, Mmax), n = lg_clampi(nc[b], 0, Nmax);
        if (i >= m || n == 0) continue;
        const float* sr = sim + row * Nmax;
        if (MODE == 0) {
            float mx = -INFINITY;
            for (int j = lane; j < n; j += 64) mx = fmaxf(mx, sr[j]);
            mx = wave_max(mx);
            float sum = 0.f;
            for (int j = lane; j < n; j += 64) sum += expf(sr[j] - mx);
            sum = wave_sum(sum);
            if (lane == 0) { rmax[row] = mx; rlog[row] = logf(sum); }
        } else {
            const float rm = rmax[row], rl = rlog[row], l0 = lg_logsigmoid(z0[row]);
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int j = lane; j < n; j += 64) {
                const float s = sr[j];
                const float v = (((s - rm) - rl) + ((s - cmax[(int64_t)b * Nmax + j]) - clog[(int64_t)b * Nmax + j])) + (l0 + lg_logsigmoid(z1[(int64_t)b * Nmax + j]));
                if (v > bv) { bv = v; bi = j; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) lg_argmax_merge(bv, bi, __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
            if (lane == 0) { best[row] = bv; arg[row] = bi == 0x7fffffff ? 0 : bi; }
        }
    }
}

// grid (ceil(Nmax / 64), B): thread (column = tid & 63, group = tid >> 6) walks rows group, group + 4, ...
template <int MODE>
__global__ __launch_bounds__(256) void lg_assign_cols_kernel(const float* __restrict__ sim, const float* __restrict__ z0, const float* __restrict__ z1,
                                                             const int32_t* __restrict__ mc, const int32_t* __restrict__ nc, int Mmax, int Nmax,
                                                             const float* __restrict__ rmax, const float* __restrict__ rlog, float* __restrict__ cmax,
                                                             float* __restrict__ clog, float* __restrict__ best, int32_t* __restrict__ arg) {
    __shared__ float sv[4][64];
    __shared__ int si[4][64];
    const int b = blockIdx.y, c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int m = lg_clampi(mc[b], 0, Mmax), n = lg_clampi(nc[b], 0, Nmax);
    const int j = blockIdx.x * 64 + c;
    if ((int)blockIdx.x * 64 >= n || m == 0) return;
    const bool on = j < n;
    const float* sb = sim + (int64_t)b * Mmax * Nmax + j;
    const int64_t col = (int64_t)b * Nmax + j;
    if (MODE == 0) {
        float mx = -INFINITY;
        if (on) for (int i = g; i < m; i += 4) mx = fmaxf(mx, sb[(int64_t)i * Nmax]);
        sv[g][c] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(sv[0][c], sv[1][c]), fmaxf(sv[2][c], sv[3][c]));
        float sum = 0.f;
        if (on) for (int i = g; i < m; i += 4) sum += expf(sb[(int64_t)i * Nmax] - mx);
        __syncthreads();
        sv[g][c] = sum;
        __syncthreads();
        if (g == 0 && on) { cmax[col] = mx; clog[col] = logf(((sv[0][c] + sv[1][c]) + sv[2][c]) + sv[3][c]); }
    } else {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        if (on) {
            const float cm = cmax[col], cl = clog[col], l1 = lg_logsigmoid(z1[col]);
            for (int i = g; i < m; i += 4) {
                const float s = sb[(int64_t)i * Nmax];
                const int64_t row = (int64_t)b * Mmax + i;
                const float v = (((s - rmax[row]) - rlog[row]) + ((s - cm) - cl)) + (lg_logsigmoid(z0[row]) + l1);
                if (v > bv) { bv = v; bi = i; }
            }
        }
        sv[g][c] = bv;
        si[g][c] = bi;
        __syncthreads();
        if (g == 0 && on) {
#pragma unroll
            for (int k = 1; k < 4; ++k) lg_argmax_merge(bv, bi, sv[k][c], si[k][c]);
            best[col] = bv;
            arg[col] = bi == 0x7fffffff ? 0 : bi;
        }
    }
}

// grid (B): one workgroup per sample
__global__ __launch_bounds__(256) void lg_assign_finish_kernel(const float* __restrict__ rbest, const int32_t* __restrict__ rarg, const int32_t* __restrict__ carg,
                                                               const int32_t* __restrict__ mc, const int32_t* __restrict__ nc, int Mmax, int Nmax, double thr,
                                                               const int32_t* __restrict__ ind0, const int32_t* __restrict__ ind1, int M0, int N0,
                                                               int32_t* __restrict__ matches0, int32_t* __restrict__ matches1, float* __restrict__ ms0,
                                                               float* __restrict__ ms1, int32_t* __restrict__ matches, float* __restrict__ mscores,
                                                               int32_t* __restrict__ nmatch) {
    __shared__ uint32_t red[4];
    const int b = blockIdx.x;
    const int m = lg_clampi(mc[b], 0, Mmax), n = lg_clampi(nc[b], 0, Nmax);
    const int64_t rb = (int64_t)b * Mmax, cb = (int64_t)b * Nmax;
    uint32_t done = 0;
    if (n > 0) {
        for (int i0 = 0; i0 < m; i0 += 256) {
            const int i = i0 + threadIdx.x;
            bool valid = false;
            int oi = 0, oj = 0;
            float sc = 0.f;
            if (i < m) {
                const int j = lg_clampi(rarg[rb + i], 0, n - 1);
                const bool mutual = carg[cb + j] == i;
                sc = mutual ? expf(rbest[rb + i]) : 0.f;
                valid = mutual && (double)sc > thr;
                oi = ind0 ? ind0[rb + i] : i;
                oj = ind1 ? ind1[cb + j] : j;
                if (oi >= 0 && oi < M0) {
                    matches0[(int64_t)b * M0 + oi] = valid ? oj : -1;
                    ms0[(int64_t)b * M0 + oi] = sc;
                }
            }
            uint32_t total;
            const uint32_t off = lg_block_exscan(valid ? 1u : 0u, red, &total);
            if (valid) {
                matches[((int64_t)b * M0 + done + off) * 2] = oi;
                matches[((int64_t)b * M0 + done + off) * 2 + 1] = oj;
                mscores[(int64_t)b * M0 + done + off] = sc;
            }
            done += total;
        }
        for (int j = threadIdx.x; j < n; j += 256) {
            const int i = lg_clampi(carg[cb + j], 0, m > 0 ? m - 1 : 0);
            bool mutual = false, valid = false;
            float sc = 0.f;
            if (m > 0) {
                mutual = rarg[rb + i] == j;
                if (mutual) {                                                // then row i is mutual too and its score is the same exp
                    sc = expf(rbest[rb + i]);
                    valid = (double)sc > thr;
                }
            }
            const int oj = ind1 ? ind1[cb + j] : j, oi = ind0 && m > 0 ? ind0[rb + i] : i;
            if (oj >= 0 && oj < N0) {
                matches1[(int64_t)b * N0 + oj] = valid ? oi : -1;
                ms1[(int64_t)b * N0 + oj] = sc;
            }
        }
    }
    if (threadIdx.x == 0) nmatch[b] = (int32_t)done;
}

// the full (m + 1) x (n + 1) log assignment of a sample inside scores [B][Mmax + 1][Nmax + 1]: the dustbin row at m, the dustbin column at n, the corner 0
__global__ __launch_bounds__(256) void lg_assign_scores_kernel(const float* __restrict__ sim, const float* __restrict__ z0, const float* __restrict__ z1,
                                                               const int32_t* __restrict__ mc, const int32_t* __restrict__ nc, int Mmax, int Nmax,
                                                               const float* __restrict__ rmax, const float* __restrict__ rlog, const float* __restrict__ cmax,
                                                               const float* __restrict__ clog, float* __restrict__ scores) {
    const int b = blockIdx.y;
    const int m = lg_clampi(mc[b], 0, Mmax), n = lg_clampi(nc[b], 0, Nmax);
    const int64_t total = (int64_t)(m + 1) * (n + 1);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int i = (int)(e / (n + 1)), j = (int)(e % (n + 1));
        const int64_t row = (int64_t)b * Mmax + i, col = (int64_t)b * Nmax + j;
        float v;
        if (i < m && j < n) {
            const float s = sim[row * Nmax + j];
            v = (((s - rmax[row]) - rlog[row]) + ((s - cmax[col]) - clog[col])) + (lg_logsigmoid(z0[row]) + lg_logsigmoid(z1[col]));
        } else if (i < m) v = lg_logsigmoid(-z0[row]);
        else if (j < n) v = lg_logsigmoid(-z1[col]);
        else v = 0.f;
        scores[((int64_t)b * (Mmax + 1) + i) * (Nmax + 1) + j] = v;
    }
}

// ======================================================================================================================================================
// The Linears and sim: C[b, r, n] (+)= alpha * sum_k A[b, r, k] Bm[b, n, k] (+ bias[n]) in exact fp32 on v_mfma_f32_32x32x2_f32, the core of
// dino_embed.hip (128 x 128 tile, 4 waves of 64 x 64, chunks of 16 k, both LDS tiles k-major with a row stride = 32 (mod 64) dwords, the next chunk's
// loads in flight while the current one multiplies).  Both operands are row-major over k: A is an activation view, Bm an nn.Linear weight as torch
// keeps it ([N][K], batch stride 0) or a second activation (sim: md1).  Every output element is one fixed sum (k-ordered fp32 chains over blocks of 64 k,
// the blocks added in order) whatever tile row it lands in, which a vendor GEMM does not promise when the row count changes: a batched pair equals its
// B = 1 call bit for bit through this kernel.  Tiles with no row below the counts (or no column below cn) do no work, rows and columns past them are
// not written.
#define LG_GM_THREADS 256
#define LG_GM_BM 128
#define LG_GM_KC 16
#define LG_GM_LS (LG_GM_BM + 32)
#define LG_GM_BLOCK 4

struct LgGemmArgs {
    const float* a;
    const float* bm;
    const float* bias;
    float* c;
    int64_t a_bs, lda, b_bs, ldb, c_bs, ldc;
    int R, N, K, S0, accumulate;
    float alpha;
    const int32_t* c0;
    const int32_t* c1;
    const int32_t* cn;
};

__global__ __launch_bounds__(LG_GM_THREADS) void lg_gemm_kernel(const LgGemmArgs g) {
    __shared__ __attribute__((aligned(16))) float lds[2 * LG_GM_KC * LG_GM_LS];
    float* As = lds;
    float* Bs = lds + LG_GM_KC * LG_GM_LS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int b = blockIdx.z, r0 = blockIdx.x * LG_GM_BM, n0 = blockIdx.y * LG_GM_BM;

    // the sample's valid rows [0, m0) and [s0, s0 + m1), valid columns [0, nn): uniform over the workgroup
    int s0 = g.R, m0 = g.R, m1 = 0, nn = g.N;
    if (g.c0) {
        s0 = g.S0;
        m0 = lg_clampi(g.c0[b], 0, s0);
        m1 = g.c1 ? lg_clampi(g.c1[b], 0, g.R - s0) : 0;
    }
    if (g.cn) nn = lg_clampi(g.cn[b], 0, g.N);
    {
        const int lo = r0 > s0 ? r0 : s0, hi = r0 + LG_GM_BM < s0 + m1 ? r0 + LG_GM_BM : s0 + m1;
        if (!(r0 < m0 || lo < hi) || n0 >= nn) return;
    }

    // loader: a thread owns one row of each tile and 8 consecutive k of every chunk
    const int pl = tid & (LG_GM_BM - 1), jq = tid >> 7;
    const bool av = r0 + pl < g.R, bv = n0 + pl < g.N;
    const float* ap = g.a + (int64_t)b * g.a_bs + (int64_t)(av ? r0 + pl : 0) * g.lda + jq * 8;
    const float* bp = g.bm + (int64_t)b * g.b_bs + (int64_t)(bv ? n0 + pl : 0) * g.ldb + jq * 8;
    const int iters = g.K / LG_GM_KC;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ra[2], rb[2];
    auto fetch = [&](int it) {
        const int k = it * LG_GM_KC;
        ra[0] = av ? *reinterpret_cast<const float4*>(ap + k) : zero4;
        ra[1] = av ? *reinterpret_cast<const float4*>(ap + k + 4) : zero4;
        rb[0] = bv ? *reinterpret_cast<const float4*>(bp + k) : zero4;
        rb[1] = bv ? *reinterpret_cast<const float4*>(bp + k + 4) : zero4;
    };
    auto stash = [&]() {
        float* pa = As + (jq * 8) * LG_GM_LS + pl;
        float* pb = Bs + (jq * 8) * LG_GM_LS + pl;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            pa[(4 * h + 0) * LG_GM_LS] = ra[h].x;
            pa[(4 * h + 1) * LG_GM_LS] = ra[h].y;
            pa[(4 * h + 2) * LG_GM_LS] = ra[h].z;
            pa[(4 * h + 3) * LG_GM_LS] = ra[h].w;
            pb[(4 * h + 0) * LG_GM_LS] = rb[h].x;
            pb[(4 * h + 1) * LG_GM_LS] = rb[h].y;
            pb[(4 * h + 2) * LG_GM_LS] = rb[h].z;
            pb[(4 * h + 3) * LG_GM_LS] = rb[h].w;
        }
    };

    f32x16_t acc[2][2], tot[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = tot[i][j][r] = 0.f;

    fetch(0);
    stash();
    __syncthreads();
    const int l31 = lane & 31, lh = lane >> 5;
    for (int it = 0; it < iters; ++it) {
        if (it + 1 < iters) fetch(it + 1);
#pragma unroll
        for (int ks = 0; ks < LG_GM_KC / 2; ++ks) {
            const int k = 2 * ks + lh;
            float fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = As[k * LG_GM_LS + (wm * 2 + i) * 32 + l31];
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = Bs[k * LG_GM_LS + (wn * 2 + j) * 32 + l31];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if ((it & (LG_GM_BLOCK - 1)) == LG_GM_BLOCK - 1 || it + 1 == iters) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
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

    // accumulator element r of lane l: column l & 31, row (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)
    float* cb = g.c + (int64_t)b * g.c_bs;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + (wn * 2 + j) * 32 + l31;
        if (n >= nn) continue;
        const float bias = g.bias ? g.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = r0 + (wm * 2 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (!(row < m0 || (row >= s0 && row < s0 + m1))) continue;
                float* p = cb + (int64_t)row * g.ldc + n;
                const float v = g.alpha * tot[i][j][r];
                *p = g.accumulate ? *p + v : v + bias;
            }
        }
    }
}

static inline bool lg_seg_ok(int64_t B, int64_t R, int64_t S0, const void* c0, const void* c1) {
    return B > 0 && R > 0 && S0 > 0 && S0 <= R && c0 && (c1 ? S0 < R : S0 == R) && S0 <= LG_MAX_N && R - S0 <= LG_MAX_N && B * R <= 0x7fffffff;
}
static inline dim3 lg_row_grid(int64_t rows) {
    const int64_t blocks = (rows + LG_ROW_WAVES - 1) / LG_ROW_WAVES;
    return dim3((unsigned)(blocks < LG_ROW_MAX_BLOCKS ? blocks : LG_ROW_MAX_BLOCKS));
}

extern "C" {

int32_t vgpa_lg_gemm(const float* a, int64_t a_batch_stride, int64_t lda, const float* bm, int64_t b_batch_stride, int64_t ldb, const float* bias, float* c,
                     int64_t c_batch_stride, int64_t ldc, int64_t B, int64_t R, int64_t N, int64_t K, float alpha, int32_t accumulate, int64_t S0,
                     const int32_t* c0, const int32_t* c1, const int32_t* cn, hipStream_t stream) {
    if (!a || !bm || !c || !al16(a) || !al16(bm) || (accumulate && bias)) return VGPA_ERR_INVALID;
    if (B <= 0 || B > 65535 || R <= 0 || R > 2 * LG_MAX_N || N <= 0 || N > (1 << 20) || K <= 0 || K > (1 << 20) || K % LG_GM_KC) return VGPA_ERR_INVALID;
    if (lda < K || ldb < K || ldc < N || lda % 4 || ldb % 4 || a_batch_stride % 4 || b_batch_stride % 4 || a_batch_stride < 0 || b_batch_stride < 0 ||
        c_batch_stride < 0)
        return VGPA_ERR_INVALID;
    if (c0 ? !lg_seg_ok(B, R, S0, c0, c1) : c1 != nullptr) return VGPA_ERR_INVALID;
    LgGemmArgs g = {};
    g.a = a; g.bm = bm; g.bias = bias; g.c = c;
    g.a_bs = a_batch_stride; g.lda = lda; g.b_bs = b_batch_stride; g.ldb = ldb; g.c_bs = c_batch_stride; g.ldc = ldc;
    g.R = (int)R; g.N = (int)N; g.K = (int)K; g.S0 = (int)S0; g.accumulate = accumulate != 0; g.alpha = alpha;
    g.c0 = c0; g.c1 = c1; g.cn = cn;
    const dim3 grid((unsigned)((R + LG_GM_BM - 1) / LG_GM_BM), (unsigned)((N + LG_GM_BM - 1) / LG_GM_BM), (unsigned)B);
    VGPA_LAUNCH(lg_gemm_kernel, grid, dim3(LG_GM_THREADS), 0, stream, g);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_lg_attn_fwd(const void* const* ptrs, const int64_t* strides, int64_t B, int64_t H, int64_t ndir, int64_t dim_stride, float q_premul,
                         hipStream_t stream) {
    if (!ptrs || !strides || B <= 0 || H <= 0 || (ndir != 1 && ndir != 2) || (dim_stride != 1 && dim_stride != 3) || B * H > 65535) return VGPA_ERR_INVALID;
    LgAttnArgs a;
    a.q_premul = q_premul;
    a.H = (int)H;
    int64_t nq_all = 0;
    for (int i = 0; i < 2; ++i) {
        const void* const* p = ptrs + 10 * (i < ndir ? i : 0);
        const int64_t* s = strides + 16 * (i < ndir ? i : 0);
        LgDir& d = a.d[i];
        d.q = (const float*)p[0]; d.k = (const float*)p[1]; d.v = (const float*)p[2]; d.o = (float*)p[3];
        d.nq = (const int32_t*)p[4]; d.nk = (const int32_t*)p[5];
        d.qcos = (const float*)p[6]; d.qsin = (const float*)p[7]; d.kcos = (const float*)p[8]; d.ksin = (const float*)p[9];
        d.q_b = s[0]; d.q_h = s[1]; d.q_t = s[2]; d.k_b = s[3]; d.k_h = s[4]; d.k_t = s[5]; d.v_b = s[6]; d.v_h = s[7]; d.v_t = s[8];
        d.o_b = s[9]; d.o_t = s[10]; d.rq_b = s[11]; d.rk_b = s[12];
        d.nq_max = (int32_t)s[13]; d.nk_max = (int32_t)s[14];
        if (!d.q || !d.k || !d.v || !d.o || !d.nq || !d.nk || !d.qcos != !d.qsin || !d.kcos != !d.ksin) return VGPA_ERR_INVALID;
        if (s[13] < 1 || s[13] > LG_MAX_N || s[14] < 0 || s[14] > LG_MAX_N) return VGPA_ERR_INVALID;
        for (int j = 0; j < 13; ++j)
            if (s[j] < 0) return VGPA_ERR_INVALID;
        if (!al16(d.o) || d.o_b % 4 || d.o_t % 4 || d.o_t < H * HD) return VGPA_ERR_INVALID;          // 16-byte stores of the context
        if (s[13] > nq_all) nq_all = s[13];
    }
    const dim3 grid((unsigned)((nq_all + WG_ROWS - 1) / WG_ROWS), (unsigned)(B * H), (unsigned)ndir);
    if (dim_stride == 1) VGPA_LAUNCH(lg_attn_kernel<1>, grid, dim3(256), 0, stream, a);
    else VGPA_LAUNCH(lg_attn_kernel<3>, grid, dim3(256), 0, stream, a);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_lg_posenc(const float* kpts, const int32_t* counts, const float* image_size, const float* Wr, float* cos_out, float* sin_out, int64_t B, int64_t N,
                       int64_t out_batch_stride, hipStream_t stream) {
    if (!kpts || !counts || !Wr || !cos_out || !sin_out || B <= 0 || B > 65535 || N <= 0 || N > LG_MAX_N || out_batch_stride < N * 32) return VGPA_ERR_INVALID;
    VGPA_LAUNCH(lg_posenc_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)B), dim3(256), 0, stream, kpts, counts, image_size, Wr, cos_out, sin_out, (int)N,
                out_batch_stride);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_lg_ln_gelu(const float* u, const float* gamma, const float* beta, float eps, float* h, float* resid, int64_t resid_stride, const float* resid_bias,
                        int64_t B, int64_t R, int64_t S0, const int32_t* c0, const int32_t* c1, hipStream_t stream) {
    if (!u || !gamma || !beta || !h || u == h || !lg_seg_ok(B, R, S0, c0, c1) || !al16(u) || !al16(h) || !al16(gamma) || !al16(beta)) return VGPA_ERR_INVALID;
    if (resid && (!resid_bias || resid_stride < LG_D || resid_stride % 4 || !al16(resid) || !al16(resid_bias))) return VGPA_ERR_INVALID;
    VGPA_LAUNCH(lg_ln_gelu_kernel, lg_row_grid(B * R), dim3(64 * LG_ROW_WAVES), 0, stream, u, gamma, beta, eps, h, resid, resid_stride, resid_bias, (int)B, (int)R,
                (int)S0, c0, c1);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_lg_confidence(const float* x, int64_t x_stride, const float* w, float bias, float* conf, float* z, double thr, int32_t* below, int64_t B, int64_t R,
                           int64_t S0, const int32_t* c0, const int32_t* c1, hipStream_t stream) {
    if (!x || !w || (!conf && !z) || x_stride < LG_D || x_stride % 4 || !al16(x) || !al16(w) || !lg_seg_ok(B, R, S0, c0, c1)) return VGPA_ERR_INVALID;
    VGPA_LAUNCH(lg_confidence_kernel, lg_row_grid(B * R), dim3(64 * LG_ROW_WAVES), 0, stream, x, x_stride, w, bias, conf, z, thr, below, (int)B, (int)R, (int)S0, c0,
                c1);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_lg_prune(const float* conf, const float* match, double thr_conf, double thr_keep, int64_t prune_min, const float* x_in, float* x_out, int64_t x_stride,
                      const float* cos_in, const float* sin_in, float* cos_out, float* sin_out, const int32_t* ind_in, int32_t* ind_out, int32_t* prune0,
                      int32_t* prune1, int64_t P0, int64_t P1, int64_t B, int64_t R, int64_t S0, const int32_t* c0, const int32_t* c1, int32_t* c0_out,
                      int32_t* c1_out, uint8_t* keep_out, hipStream_t stream) {
    if (!conf || !match || !x_in || !x_out || x_in == x_out || !cos_in || !sin_in || !cos_out || !sin_out || cos_in == cos_out || sin_in == sin_out || !ind_in ||
        !ind_out || ind_in == ind_out || !prune0 || !c0_out || P0 <= 0)
        return VGPA_ERR_INVALID;
    if (!lg_seg_ok(B, R, S0, c0, c1) || B > 65535 || (c1 && (!prune1 || !c1_out || P1 <= 0)) || x_stride < LG_D || x_stride % 4) return VGPA_ERR_INVALID;
    if (!al16(x_in) || !al16(x_out) || !al16(cos_in) || !al16(sin_in) || !al16(cos_out) || !al16(sin_out)) return VGPA_ERR_INVALID;
    VGPA_LAUNCH(lg_prune_kernel, dim3((unsigned)B, c1 ? 2u : 1u), dim3(256), 0, stream, conf, match, thr_conf, thr_keep, (int)prune_min, x_in, x_out, x_stride, cos_in,
                sin_in, cos_out, sin_out, ind_in, ind_out, prune0, prune1, (int)P0, (int)P1, (int)R, (int)S0, c0, c1, c0_out, c1_out, keep_out);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

size_t vgpa_lg_assign_workspace_bytes(int64_t B, int64_t Mmax, int64_t Nmax) {
    if (B <= 0 || Mmax <= 0 || Nmax <= 0) return 0;
    return (size_t)B * (size_t)(Mmax + Nmax) * 4 * sizeof(float);            // max, log-sum, best, arg by row and by column
}

int32_t vgpa_lg_assign(const float* sim, const float* z0, const float* z1, const int32_t* m, const int32_t* n, int64_t B, int64_t Mmax, int64_t Nmax, double thr,
                       const int32_t* ind0, const int32_t* ind1, int64_t M0, int64_t N0, int32_t* matches0, int32_t* matches1, float* mscores0, float* mscores1,
                       int32_t* matches, float* mscores, int32_t* nmatch, float* scores, int32_t stages, void* workspace, size_t ws_bytes, hipStream_t stream) {
    if (!m || !n || B <= 0 || B > 65535 || Mmax <= 0 || Nmax <= 0 || Mmax > LG_MAX_N || Nmax > LG_MAX_N || !workspace || stages <= 0 || stages > 7)
        return VGPA_ERR_INVALID;
    if (ws_bytes < vgpa_lg_assign_workspace_bytes(B, Mmax, Nmax)) return VGPA_ERR_WORKSPACE;
    if ((stages & 3) && (!sim || !z0 || !z1)) return VGPA_ERR_INVALID;
    if ((stages & 4) && (!matches0 || !matches1 || !mscores0 || !mscores1 || !matches || !mscores || !nmatch || M0 < Mmax || N0 < Nmax || !ind0 != !ind1))
        return VGPA_ERR_INVALID;
    float* w = (float*)workspace;
    const int64_t nr = B * Mmax, ncol = B * Nmax;
    float *rmax = w, *rlog = w + nr, *rbest = w + 2 * nr, *cmax = w + 4 * nr, *clog = cmax + ncol, *cbest = cmax + 2 * ncol;
    int32_t *rarg = (int32_t*)(w + 3 * nr), *carg = (int32_t*)(cmax + 3 * ncol);
    const dim3 rgrid = lg_row_grid(nr), cgrid((unsigned)((Nmax + 63) / 64), (unsigned)B);
    if (stages & 1) {
        VGPA_LAUNCH(lg_assign_rows_kernel<0>, rgrid, dim3(256), 0, stream, sim, z0, z1, m, n, (int)B, (int)Mmax, (int)Nmax, rmax, rlog, cmax, clog, rbest, rarg);
        VGPA_LAUNCH(lg_assign_cols_kernel<0>, cgrid, dim3(256), 0, stream, sim, z0, z1, m, n, (int)Mmax, (int)Nmax, rmax, rlog, cmax, clog, cbest, carg);
    }
    if (stages & 2) {
        VGPA_LAUNCH(lg_assign_rows_kernel<1>, rgrid, dim3(256), 0, stream, sim, z0, z1, m, n, (int)B, (int)Mmax, (int)Nmax, rmax, rlog, cmax, clog, rbest, rarg);
        VGPA_LAUNCH(lg_assign_cols_kernel<1>, cgrid, dim3(256), 0, stream, sim, z0, z1, m, n, (int)Mmax, (int)Nmax, rmax, rlog, cmax, clog, cbest, carg);
        if (scores)
            VGPA_LAUNCH(lg_assign_scores_kernel, dim3(1024, (unsigned)B), dim3(256), 0, stream, sim, z0, z1, m, n, (int)Mmax, (int)Nmax, rmax, rlog, cmax, clog, scores);
    }
    if (stages & 4)
        VGPA_LAUNCH(lg_assign_finish_kernel, dim3((unsigned)B), dim3(256), 0, stream, rbest, rarg, carg, m, n, (int)Mmax, (int)Nmax, thr, ind0, ind1, (int)M0,
                    (int)N0, matches0, matches1, mscores0, mscores1, matches, mscores, nmatch);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

}  // extern "C"
