// Online-softmax (running-maximum) forward of the 3D full attention (all T*H*W + text tokens, non-causal, head_dim 64) for gfx950,
// plus the backward's delta.  The product forward and backward are the one-wave-per-SIMD "w1" kernels of attention_w1.hip; this
// file holds what stands behind them:
//  * attn_fwd_pipe_kernel: the flash-style forward with a running row maximum, hand-written around v_mfma_f32_32x32x16_bf16.
//    vgpa_internal_attn_fwd_redo launches it over the 256-row strips the w1 forward flagged (its bound-shifted softmax could not
//    represent them) and over every strip for vgpa_attn_fwd_online_res and for sequences too short for the w1 kernel.
//  * attn_delta_kernel (vgpa_attn_bwd_delta_res): delta = rowsum(dO o O) on its own, without the w1 statistics planes.
// Oracle: oracle/cogvideox.py::block_forward (softmax(QK^T/8)V), the F.scaled_dot_product_attention of diffusers'
// CogVideoXAttnProcessor2_0 as reached from train/CogVideoX-5B/03_train.py:134-151.
//
// Conventions (shared with attention_w1.hip):
//  * 256-thread workgroup = 4 waves; a wave owns 2 x 32 query rows and keeps its operand fragments and accumulators in registers
//    for the whole sweep over the keys (2 waves per SIMD).
//  * Every product is computed TRANSPOSED (S^T = K Q^T, O^T = V^T P^T) so the softmax row a lane works on
//    is the MFMA column lane&31: running max / sum / LSE are lane-local scalars, and the fp32
//    accumulator registers of one product are, after a bf16 pack, directly the B operand of the next one
//    (the k-slot permutation this implies is applied to the A-side LDS reads instead of shuffling P).
//  * K/V tiles of 64 rows are staged HBM -> registers -> LDS, one barrier per tile;
//    row pitch 144 B makes the 16-byte fragment reads bank-conflict free.  Operands that are contracted over
//    their row index are read with the gfx950 hardware transpose read (ds_read_b64_tr_b16), so every tensor
//    stays row-major [tokens, 64] in HBM and no transposed copy is ever written.
//  * Loads clamp the row index to S-1 and the tail is masked, so S needs no padding (17 776 = 277*64 + 48).
//  * blockIdx is remapped so that the workgroups an XCD runs concurrently share (batch, head) and hit K/V in
//    that XCD's private L2.
#include "attn_common.h"

// =====================================================================================================
// Forward:  O = softmax(scale * Q K^T) V ;  lse2 = log2 sum_k exp2(scale*log2e * q.k)
// =====================================================================================================
#define PSUM_TRIGGER 1024.0f   // a half-lane tile sum above this (or inf/NaN) means some score outgrew the running max by > ~2^5

// =====================================================================================================
// Forward, software-pipelined.  The tile loop body is ONE basic block in which independent work of
// neighbouring half-tiles (32 keys) can overlap inside a wave:
//     sB = QK^T(t, keys 32..63)   ||  pA = exp2(sA)            sA = scores of (t, keys 0..31), made one step earlier
//     O += V^T pA^T               ||  pB = exp2(sB)
//     sA = QK^T(t+1, keys 0..31)  ||  O += V^T pB^T
// with the same 64 score registers (exp in place; a half is overwritten right after its PV consumed it).  To make that
// legal the softmax check moves BEHIND the PV product: P is formed against the running max m, the tile is accumulated
// unconditionally, and only then is the tile's partial sum looked at.  A sum above PSUM_TRIGGER means some score
// outgrew m; O and l are still exactly consistent (everything is scaled by 2^-m), so the repair is "raise m to the true
// max, rescale O, l and the already-made sA" -- nothing is recomputed.  What cannot be repaired is an overflow inside a
// single tile (a score > m + 64 in log2 units; impossible for LayerNorm-ed q, k with sane weights): it sets a workgroup
// flag and the q-strip is redone by the plain online-softmax loop (safe_tile for every tile), which also handles the
// first tile (establishes m) and the ragged last tile.  K tiles: 3-slot LDS ring, V tiles: 2-slot ring.
// =====================================================================================================
#define PSUM_OVERFLOW 1.8446744e19f   // 2^64: a half-lane tile sum above this (or NaN) -> redo the strip in safe mode

template <int QB>
__device__ __forceinline__ void qk_half(const bf16_t* kl, int kb, int lane, const bf16x8_t& kx, const bf16x8_t (&qx)[QB],
                                        const bf16x8_t (&qf)[QB][4], f32x16_t (&s)[QB]) {
#pragma unroll
    for (int j = 0; j < QB; ++j) {
#pragma unroll
        for (int i = 0; i < 16; ++i) s[j][i] = 0.f;
        s[j] = mfma32(kx, qx[j], s[j]);
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const bf16x8_t kf = frag_row(kl, kb * 32, ks, lane);
#pragma unroll
        for (int j = 0; j < QB; ++j) s[j] = mfma32(kf, qf[j][ks], s[j]);
    }
}

template <int QB>
__device__ __forceinline__ void exp_half(f32x16_t (&s)[QB], f32x2_t (&ps2)[QB]) {
#pragma unroll
    for (int j = 0; j < QB; ++j)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            s[j][r] = __builtin_amdgcn_exp2f(s[j][r]);
            s[j][r + 1] = __builtin_amdgcn_exp2f(s[j][r + 1]);
            ps2[j][0] = nopack_add(ps2[j][0], s[j][r]);
            ps2[j][1] = nopack_add(ps2[j][1], s[j][r + 1]);
        }
}

template <int QB>
__device__ __forceinline__ void pv_half(const bf16_t* vl, int kb, int lane, const f32x16_t (&s)[QB], f32x16_t (&o)[QB][2]) {
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        bf16x8_t pf[QB];
#pragma unroll
        for (int j = 0; j < QB; ++j) pf[j] = pack_frag(s[j], 8 * cc);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            const bf16x8_t vf = frag_tr(vl, kb * 32 + 16 * cc, db * 32, lane);
#pragma unroll
            for (int j = 0; j < QB; ++j) o[j][db] = mfma32(vf, pf[j], o[j][db]);
        }
    }
}

// exact row max of tile (kl) over the valid keys, both halves; raises m and rescales O, l (and `carry`, scores that were
// already made against the old m).  Returns with qx holding the new shift and s0 / s1 the raw scores.
template <int QB, bool HAS_CARRY>
__device__ __forceinline__ void raise_max(const bf16_t* kl, int key0, int S, bool tail, int lane, int hi, const bf16x8_t (&qf)[QB][4],
                                          bf16x8_t (&qx)[QB], float (&m)[QB], float (&l)[QB], f32x16_t (&o)[QB][2],
                                          f32x16_t (&carry)[QB], f32x16_t (&s0)[QB], f32x16_t (&s1)[QB]) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        f32x16_t(&s)[QB] = kb ? s1 : s0;
#pragma unroll
        for (int j = 0; j < QB; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) s[j][i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8_t kf = frag_row(kl, kb * 32, ks, lane);
#pragma unroll
            for (int j = 0; j < QB; ++j) s[j] = mfma32(kf, qf[j][ks], s[j]);
        }
        if (tail) {
#pragma unroll
            for (int j = 0; j < QB; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (key0 + kb * 32 + acc_row(r, hi) >= S) s[j][r] = -INFINITY;
        }
    }
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        float mx = s0[j][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s0[j][r]);
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s1[j][r]);
        mx = fmaxf(mx, other_half(mx));
        const float m_new = fmaxf(m[j], mx);
        const float alpha = __builtin_amdgcn_exp2f(m[j] - m_new);   // m = -inf on the first tile: alpha = 0, O = l = 0 stay 0
        if (HAS_CARRY) {
            const float d = m[j] - m_new;
#pragma unroll
            for (int i = 0; i < 16; ++i) carry[j][i] += d;
        }
        m[j] = m_new;
        qx[j] = shift_frag(m_new, hi);
        l[j] *= alpha;
#pragma unroll
        for (int i = 0; i < 16; ++i) { o[j][0][i] *= alpha; o[j][1][i] *= alpha; }
    }
}

// plain online-softmax step for one tile (first tile, ragged last tile, and every tile of the safe-mode redo)
template <int QB>
__device__ __forceinline__ void safe_tile(const bf16_t* kl, const bf16_t* vl, int key0, int S, bool tail, int lane, int hi,
                                          const bf16x8_t (&qf)[QB][4], bf16x8_t (&qx)[QB], float (&m)[QB], float (&l)[QB],
                                          f32x16_t (&o)[QB][2]) {
    f32x16_t s0[QB], s1[QB];
    raise_max<QB, false>(kl, key0, S, tail, lane, hi, qf, qx, m, l, o, s0, s0, s1);
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p0 = __builtin_amdgcn_exp2f(s0[j][r] - m[j]), p1 = __builtin_amdgcn_exp2f(s1[j][r] - m[j]);
            s0[j][r] = p0;
            s1[j][r] = p1;
            ps += p0 + p1;
        }
        l[j] += ps;
    }
    pv_half<QB>(vl, 0, lane, s0, o);
    pv_half<QB>(vl, 1, lane, s1, o);
}

// workgroup = task (one 256-row query strip of one head) task0 + remapped blockIdx, all key tiles; with only_flagged, only the strips
// whose flag is set.  task0 (the launcher passes 0) and the two unnamed arguments behind it are what is left of a key-range split this
// kernel once had: they keep the kernel-argument layout, and with it the compiled kernel, exactly what it was with the split.
__global__ __launch_bounds__(256, 2) void attn_fwd_pipe_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
                                                               bf16_t* __restrict__ O, float* __restrict__ LSE2, TStride sq, TStride sk, TStride sv,
                                                               TStride so, int S, int H, int n_qt, int task0, int /* unused */, float* /* unused */,
                                                               const int* __restrict__ only_flagged, void* __restrict__ ORES, TStride sor, int res_kind) {
    constexpr int QB = 2, NW = 4;   // 32-row query blocks per wave, waves per workgroup
    __shared__ __attribute__((aligned(16))) bf16_t lds[5 * TILE_ELEMS];  // K ring [3], V ring [2]
    __shared__ int redo_flag;
    const int vid = task0 + xcd_remap(blockIdx.x, gridDim.x);
    if (only_flagged && only_flagged[vid] == 0) return;   // redo pass behind the w1 forward: only the strips it flagged
    const int bh = vid / n_qt, qt = vid % n_qt;
    const int b = bh / H, h = bh % H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5;
    const int q0 = (qt * NW + wave) * (32 * QB);

    const bf16_t* Qb = Q + ((size_t)b * sq.b + (size_t)h * sq.h);
    const bf16_t* Kb = K + ((size_t)b * sk.b + (size_t)h * sk.h);
    const bf16_t* Vb = V + ((size_t)b * sv.b + (size_t)h * sv.h);
    bf16_t* const kring = lds;
    bf16_t* const vring = lds + 3 * TILE_ELEMS;

    bf16x8_t qf[QB][4], qx[QB];
    f32x16_t o[QB][2];
    float m[QB], l[QB];
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        load_row_frags(Qb, sq.s, q0 + 32 * j, S, lane, qf[j]);
#pragma unroll
        for (int i = 0; i < 16; ++i) { o[j][0][i] = 0.f; o[j][1][i] = 0.f; }
        m[j] = -INFINITY;
        l[j] = 0.f;
        qx[j] = shift_frag(0.f, hi);
    }
    bf16x8_t kx;   // K-side of the shift k-step: ones in k-slots 0..2 of the lower half-lanes
    {
        float o8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (hi == 0) { o8[0] = 1.f; o8[1] = 1.f; o8[2] = 1.f; }
        kx = f32_to_frag(o8);
    }

    const int nt = (S + TILE - 1) / TILE;
    const bool ragged = (S & (TILE - 1)) != 0;   // the ragged tile, if any, is the last one
    const rsrc_t krs = tile_rsrc(Kb, sk.s, S), vrs = tile_rsrc(Vb, sv.s, S);
    const uint32_t koff = tile_lane_byte_offset(sk.s), voff = tile_lane_byte_offset(sv.s);
    u32x4_t kr[8 / NW], vr[8 / NW];
    if (threadIdx.x == 0) redo_flag = 0;
    // prologue: K(0..2), V(0..1) -> LDS (rows past S read as zeros; their scores are masked or unused)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        tile_load_buf(krs, sk.s, i * TILE, koff, kr);
        tile_store(kring + i * TILE_ELEMS, kr);
        if (i < 2) {
            tile_load_buf(vrs, sv.s, i * TILE, voff, vr);
            tile_store(vring + i * TILE_ELEMS, vr);
        }
    }
#pragma unroll
    for (int j = 0; j < QB; ++j) frags_arrived(qf[j]);
    __syncthreads();

    // first tile: establishes m (also the ragged tile when it is the only one)
    safe_tile<QB>(kring, vring, 0, S, ragged && nt == 1, lane, hi, qf, qx, m, l, o);

    f32x16_t sA[QB], sB[QB];
    if (nt > 2) qk_half<QB>(kring + TILE_ELEMS, 0, lane, kx, qx, qf, sA);
    int kslot = 1, vslot = 1;   // ring slots of tile t
    for (int t = 1; t < nt - 1; ++t) {
        const bf16_t* kl = kring + kslot * TILE_ELEMS;
        const int kslot1 = kslot == 2 ? 0 : kslot + 1, kslot2 = kslot1 == 2 ? 0 : kslot1 + 1;
        const bf16_t* kl1 = kring + kslot1 * TILE_ELEMS;
        const bf16_t* vl = vring + vslot * TILE_ELEMS;
        tile_load_buf(krs, sk.s, (t + 2) * TILE, koff, kr);   // one staging register set, used for K then for V
        f32x2_t ps2[QB];
#pragma unroll
        for (int j = 0; j < QB; ++j) ps2[j] = (f32x2_t){0.f, 0.f};
        qk_half<QB>(kl, 1, lane, kx, qx, qf, sB);
        exp_half<QB>(sA, ps2);
        pv_half<QB>(vl, 0, lane, sA, o);
        tile_store(kring + kslot2 * TILE_ELEMS, kr);
        tile_load_buf(vrs, sv.s, (t + 1) * TILE, voff, kr);
#ifndef PIPE_NO_SB
        // nothing crosses: everything that reads the old sA is done before the next half-tile's scores are started, so
        // they are written into the same registers (otherwise the rotation costs 32 register copies per tile)
        __builtin_amdgcn_sched_barrier(0);
#endif
        exp_half<QB>(sB, ps2);
        qk_half<QB>(kl1, 0, lane, kx, qx, qf, sA);
        pv_half<QB>(vl, 1, lane, sB, o);
        bool grew = false, over = false;
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            const float psum = ps2[j][0] + ps2[j][1];
            l[j] += psum;
            grew = grew || !(psum <= PSUM_TRIGGER);
            over = over || !(psum <= PSUM_OVERFLOW);
        }
        if (__any(grew)) {
            if (__any(over)) redo_flag = 1;
            raise_max<QB, true>(kl, t * TILE, S, false, lane, hi, qf, qx, m, l, o, sA, sB, sB);
        }
        tile_store(vring + (vslot ^ 1) * TILE_ELEMS, kr);
        kslot = kslot1;
        vslot ^= 1;
        __syncthreads();
    }
    if (nt > 1) safe_tile<QB>(kring + kslot * TILE_ELEMS, vring + vslot * TILE_ELEMS, (nt - 1) * TILE, S, ragged, lane, hi, qf, qx, m, l, o);

    if (redo_flag) {   // workgroup-uniform (written before the loop's last barrier); essentially never taken
#pragma unroll
        for (int j = 0; j < QB; ++j) {
#pragma unroll
            for (int i = 0; i < 16; ++i) { o[j][0][i] = 0.f; o[j][1][i] = 0.f; }
            m[j] = -INFINITY;
            l[j] = 0.f;
        }
        for (int t = 0; t < nt; ++t) {
            __syncthreads();
            tile_load_buf(krs, sk.s, t * TILE, koff, kr);
            tile_load_buf(vrs, sv.s, t * TILE, voff, vr);
            tile_store(kring, kr);
            tile_store(vring, vr);
            __syncthreads();
            safe_tile<QB>(kring, vring, t * TILE, S, ragged && t == nt - 1, lane, hi, qf, qx, m, l, o);
        }
    }

#pragma unroll
    for (int j = 0; j < QB; ++j) {
        const float lt = l[j] + other_half(l[j]);
        const float inv = 1.f / lt;
        const int q = q0 + 32 * j + (lane & 31);
        if (q < S) {
            bf16_t* op = O + ((size_t)b * so.b + (size_t)h * so.h + (size_t)q * so.s);
            const size_t ro = (size_t)b * sor.b + (size_t)h * sor.h + (size_t)q * sor.s;   // the output's residual for the backward's delta (attention_w1.hip)
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float x[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) x[i] = o[j][db][4 * g + i] * inv;
                    u32x2_t w;
                    w[0] = pack_bf16x2(x[0], x[1]);
                    w[1] = pack_bf16x2(x[2], x[3]);
                    *reinterpret_cast<u32x2_t*>(op + db * 32 + 8 * g + 4 * hi) = w;
                    if (res_kind == VGPA_RES_8) {
                        *reinterpret_cast<uint32_t*>((uint8_t*)ORES + ro + db * 32 + 8 * g + 4 * hi) = res8_pack4(x, w);
                    } else if (res_kind == VGPA_RES_BF16) {
                        u32x2_t r;
                        r[0] = pack_bf16x2(x[0] - __uint_as_float(w[0] << 16), x[1] - __uint_as_float(w[0] & 0xffff0000u));
                        r[1] = pack_bf16x2(x[2] - __uint_as_float(w[1] << 16), x[3] - __uint_as_float(w[1] & 0xffff0000u));
                        *reinterpret_cast<u32x2_t*>((bf16_t*)ORES + ro + db * 32 + 8 * g + 4 * hi) = r;
                    }
                }
            if (hi == 0) LSE2[(int64_t)bh * S + q] = m[j] + __builtin_amdgcn_logf(lt);  // v_log_f32 is log2
        }
    }
}

// =====================================================================================================
// delta[b,h,q] = sum_d dO[q,d] * O[q,d]
// =====================================================================================================
__global__ __launch_bounds__(256) void attn_delta_kernel(const bf16_t* __restrict__ dO, const bf16_t* __restrict__ O, TStride sdo,
                                                           TStride so, int S, int H, int64_t total /* B*H*S */, float* __restrict__ delta,
                                                           const void* __restrict__ ORES = nullptr, TStride sor = TStride{0, 0, 0},
                                                           int res_kind = VGPA_RES_NONE) {
    // 8 lanes per (b,h,q) row, 16 B each
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid >> 3;
    const int c8 = (int)(gid & 7);
    float acc = 0.f;
    if (row < total) {
        const int q = (int)(row % S);
        const int64_t bh = row / S;
        const int h = (int)(bh % H), b = (int)(bh / H);
        float a[8], o[8];
        unpack8(*reinterpret_cast<const u32x4_t*>(dO + ((size_t)b * sdo.b + (size_t)h * sdo.h + (size_t)q * sdo.s + c8 * 8)), a);
        const u32x4_t ob = *reinterpret_cast<const u32x4_t*>(O + ((size_t)b * so.b + (size_t)h * so.h + (size_t)q * so.s + c8 * 8));
        const size_t ro = (size_t)b * sor.b + (size_t)h * sor.h + (size_t)q * sor.s + c8 * 8;
        if (res_kind == VGPA_RES_8) {   // the forward's 8 further mantissa bits (common.h res8)
            unpack8_res8(ob, *reinterpret_cast<const u32x2_t*>((const uint8_t*)ORES + ro), o);
        } else {
            unpack8(ob, o);
            if (res_kind == VGPA_RES_BF16) {   // the forward's rounding residual (attention_w1.hip, w1_residual4)
                float r[8];
                unpack8(*reinterpret_cast<const u32x4_t*>((const bf16_t*)ORES + ro), r);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] += r[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += a[j] * o[j];
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if (row < total && c8 == 0) delta[row] = acc;
}

// Redo pass behind the w1 forward (attention_w1.hip): the online-softmax kernel over every 256-row strip whose flag is set.
int32_t vgpa_internal_attn_fwd_redo(const void* q, const void* k, const void* v, void* o, float* lse2, TStride sq, TStride sk, TStride sv, TStride so,
                                    int S, int H, int n_qt, int64_t tasks, const int* flags, hipStream_t stream, void* o_res, TStride sor, int res_kind) {
    VGPA_LAUNCH(attn_fwd_pipe_kernel, dim3((unsigned)tasks), dim3(256), 0, stream, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, lse2, sq,
                sk, sv, so, S, H, n_qt, 0, 1, (float*)nullptr, flags, o_res, sor, o_res ? res_kind : VGPA_RES_NONE);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

static inline bool bwd_common_ok(int64_t B, int64_t H, int64_t S, int64_t head_dim) {
    return head_dim == HD && B > 0 && H > 0 && S > 0 && S <= (1 << 24) && (int64_t)((S + WG_ROWS - 1) / WG_ROWS) * B * H <= 0x7fffffff;
}

extern "C" {

// Tensors are bf16 views [B, H, S, 64] given by element strides {batch, head, token} (last dim contiguous, strides multiples of 8,
// base pointers 16-byte aligned); delta is fp32 [B, H, S] contiguous.

// step 1 of the backward: delta[b,h,q] = sum_d dO * O  -- of the output as the forward's residual tensor completes it when o_res is given
// (vgpa_attn_fwd_w1_res, res_kind VGPA_RES_BF16 / VGPA_RES_8); o_res may be NULL
int32_t vgpa_attn_bwd_delta_res(const void* o, const void* o_res, int32_t res_kind, const void* d_o, const int64_t* o_strides, const int64_t* ores_strides,
                                const int64_t* do_strides, float* delta, int64_t B, int64_t H, int64_t S, int64_t head_dim, hipStream_t stream) {
    if (!o || !d_o || !delta || !bwd_common_ok(B, H, S, head_dim) || !view_ok(o_strides, B, H, S, HD) || !view_ok(do_strides, B, H, S, HD) || !al16(o) ||
        !al16(d_o))
        return VGPA_ERR_INVALID;
    if (o_res && (!view_ok(ores_strides, B, H, S, HD) || !al16(o_res) || (res_kind != VGPA_RES_BF16 && res_kind != VGPA_RES_8))) return VGPA_ERR_INVALID;
    const int64_t total = B * H * S;
    VGPA_LAUNCH(attn_delta_kernel, dim3((unsigned)((total * 8 + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)d_o, (const bf16_t*)o,
                       mk(do_strides), mk(o_strides), (int)S, (int)H, total, delta, o_res, o_res ? mk(ores_strides) : mk(o_strides),
                       o_res ? (int)res_kind : VGPA_RES_NONE);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

}  // extern "C"
