// Shared pieces of the "w1" attention kernels (attention_w1.hip): one wave per SIMD, the whole 512-register file per
// wave, streamed tiles brought in by LDS-DMA (buffer_load_dwordx4 ... lds) into an unpadded, chunk-swizzled ring.
//
// LDS image of one streamed [64 rows x 64 bf16] tile: 8 KiB, row pitch 128 B (no padding: the LDS-DMA destination is
// wave-uniform base + lane * 16 B, so the image must be lane-linear), the eight 16-B chunks of row r stored at chunk
// position c ^ f(r), f(r) = (r1 << 2) | (r2 << 1) | r3 (r_i = bit i of r).  The permutation is applied on the SOURCE side
// (each lane's global address) and again on every read.  With it
//   * the 16-byte row-fragment reads (ds_read_b128: 16-lane groups of 16 different rows mod 16, one logical chunk) hit
//     16 different 16-B slots of the 256-B bank row, and
//   * the transpose reads (ds_read_b64_tr_b16: 32 lanes = 4 rows x 4 chunks x 2 halves) hit all 16 slots twice 8 B,
// i.e. both read kinds are bank-conflict free, which no padded pitch achieves for the two at once.
//
// The head_dim-128 image (attention_hd128.hip) is the same with 256-byte rows and sixteen chunks per row, f(r) = w1h_swz(r).
//
// This header is also the one home of the C++ shell around the generated main loops (w1_*_loop.inc): ring priming, the
// per-lane DMA and read offsets, the split ranges, the epilogue row stores and the redo-flag thresholds, for both head dims.
// The asm operand lists stay in the kernels: the register map is each loop's own contract.
#pragma once
#include "attn_common.h"

#define W1_TILE_BYTES 8192                  // one [64][64] bf16 tile
#define W1_SLOT_BYTES (2 * W1_TILE_BYTES)   // a ring slot = the two streamed operands of one step (K|V or Q|dO)
#define W1_SLOTS 4                          // ring depth: LDS-DMA runs two tiles ahead of the first reader
#define W1_RING_BYTES (W1_SLOTS * W1_SLOT_BYTES)
#define W1_STAT_BYTES 1024                  // dK/dV kernels, per ring slot behind the ring: 4 waves x (16 x -lse2 | 16 x -delta | 128 B unused)

typedef __attribute__((address_space(3))) bf16x4_t* w1_lds_b64_t;
typedef __attribute__((ext_vector_type(16))) uint32_t u32x16_t;
typedef __attribute__((ext_vector_type(8))) uint32_t u32x8_t;

__device__ __forceinline__ uint32_t w1_swz(uint32_t r) { return (((r >> 1) & 1u) << 2) | (((r >> 2) & 1u) << 1) | ((r >> 3) & 1u); }
__device__ __forceinline__ uint32_t w1h_swz(uint32_t r) { return ((r & 3u) << 2) | ((r >> 2) & 3u); }   // head_dim 128: sixteen chunks per row

// Geometry of a streamed [64 rows x D bf16] tile, D = 64 or 128: a wave's LDS-DMA piece is 1 KiB = 64 lanes x 16 B.
template <int D>
struct W1Tile {
    static constexpr uint32_t ROW_BYTES = 2 * D;                      // 128 / 256
    static constexpr uint32_t TILE_BYTES = 64 * ROW_BYTES;            // 8 / 16 KiB
    static constexpr uint32_t SLOT_BYTES = 2 * TILE_BYTES;
    static constexpr uint32_t RING_BYTES = W1_SLOTS * SLOT_BYTES;
    static constexpr int PW = TILE_BYTES / 1024 / 4;                  // pieces per wave and tile: 2 / 4
    static constexpr uint32_t CHUNKS = ROW_BYTES / 16;                // lanes per row of a piece: 8 / 16
    static constexpr uint32_t PIECE_ROWS = 64 / CHUNKS;               // rows of a piece: 8 / 4
    static constexpr int KS = D / 16;                                 // k-steps along d: 4 / 8
    typedef uint32_t table_t __attribute__((ext_vector_type(D / 8))); // w1_read_offsets
    static __device__ __forceinline__ uint32_t swz(uint32_t r) { return D == 64 ? w1_swz(r) : w1h_swz(r); }
};

// wave-uniform buffer descriptor over rows [0, S) of one (batch, head) slice: rows at or past S read as zeros
struct W1Rsrc { u32x4_t w; };
__device__ __forceinline__ W1Rsrc w1_rsrc(const void* base /* uniform */, uint32_t bytes) {
    const uint64_t a = (uint64_t)base;
    W1Rsrc r;
    r.w[0] = __builtin_amdgcn_readfirstlane((uint32_t)a);
    r.w[1] = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32) & 0xffffu);
    r.w[2] = __builtin_amdgcn_readfirstlane(bytes);
    r.w[3] = 0x00020000u;
    return r;
}

// One LDS-DMA piece: 64 lanes x 16 B from (descriptor, per-lane byte offset, uniform byte offset) to LDS bytes
// [lds_dst, lds_dst + 1024).  Invisible to hipcc's waitcnt bookkeeping on purpose (it would drain the ring at the next
// ds_read): completion is counted by hand with w1_wait_* below.  M0 is saved and restored (compiler-reserved).
__device__ __forceinline__ void w1_dma(uint32_t lds_dst /* uniform */, const W1Rsrc& rs, uint32_t voff, uint32_t soff /* uniform */) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %2, %3, %4 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "s"(lds_dst), "v"(voff), "s"(rs.w), "s"(soff)
        : "memory");
}

// the 4-byte-per-lane form (256 B per wave-instruction)
__device__ __forceinline__ void w1_dma4(uint32_t lds_dst /* uniform */, const W1Rsrc& rs, uint32_t voff, uint32_t soff /* uniform */) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "buffer_load_dword %2, %3, %4 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "s"(lds_dst), "v"(voff), "s"(rs.w), "s"(soff)
        : "memory");
}

// wait until at most N of this wave's VMEM operations are outstanding, and all of its LDS reads have returned
#define W1_WAIT(N) asm volatile("s_waitcnt vmcnt(" #N ") lgkmcnt(0)" ::: "memory")

// per-lane source offsets (bytes) of the PW pieces this wave moves of a [64 x D] tile with row stride `row_stride`
// (elements): piece j = wave * PW + i covers rows PIECE_ROWS j .. + PIECE_ROWS - 1; lane -> (row PIECE_ROWS j + lane / CHUNKS, LDS chunk lane % CHUNKS)
template <int D>
__device__ __forceinline__ void w1_dma_offsets(int wave, int lane, uint32_t row_stride, uint32_t (&voff)[W1Tile<D>::PW]) {
    typedef W1Tile<D> G;
#pragma unroll
    for (int i = 0; i < G::PW; ++i) {
        const uint32_t row = G::PIECE_ROWS * (uint32_t)(wave * G::PW + i) + (uint32_t)lane / G::CHUNKS;
        const uint32_t c = ((uint32_t)lane & (G::CHUNKS - 1u)) ^ G::swz(row);
        voff[i] = (row * row_stride + c * 8u) * 2u;
    }
}

// Priming: tiles t, t + 1 -> ring slots 0, 1.  voff = the loop's offset registers, PW of operand a then PW of operand b, already at tile t: the
// tile offset rides in the per-lane offset (not in the scalar offset) because the descriptor's range check must see it, so that rows at or
// past S -- and whole tiles past the end -- arrive as zeros.  With `st` (dK/dV kernels) the statistics piece of each tile follows it.
template <int D, class V>
__device__ __forceinline__ void w1_prime(uint32_t wbase /* uniform */, const W1Rsrc& ra, const W1Rsrc& rb, V& voff, uint32_t astep, uint32_t bstep,
                                         const W1Rsrc* st = nullptr, uint32_t sbase = 0u, uint32_t* svo = nullptr) {
    typedef W1Tile<D> G;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const uint32_t dst = wbase + (uint32_t)t * G::SLOT_BYTES;
#pragma unroll
        for (int i = 0; i < G::PW; ++i) w1_dma(dst + 1024u * i, ra, voff[i], 0u);
#pragma unroll
        for (int i = 0; i < G::PW; ++i) w1_dma(dst + G::TILE_BYTES + 1024u * i, rb, voff[G::PW + i], 0u);
        if (st) w1_dma4(sbase + (uint32_t)t * W1_STAT_BYTES, *st, *svo, 0u);
#pragma unroll
        for (int i = 0; i < G::PW; ++i) { voff[i] += astep; voff[G::PW + i] += bstep; }
        if (st) *svo += 256u;
    }
}

// The pipelines' first transposed reads hit the slot "before" the first tile (ring slot 3), which no DMA has written yet: make `pieces`
// 4-KiB pieces from `byte_offset` on finite.  All 256 threads; the caller's __syncthreads() follows.
__device__ __forceinline__ void w1_zero_slot(uint8_t* lds, uint32_t byte_offset, int pieces) {
    const u32x4_t z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < pieces; ++i) *reinterpret_cast<u32x4_t*>(lds + byte_offset + i * 4096 + threadIdx.x * 16) = z;
}

// The lane-constant LDS read offsets the generated loops take in registers (bytes from `base`; the head_dim-128 loops take one table per slot
// pair because ds offsets are 16 bit):  [ks] row fragment of rows m = lane & 31, logical chunk 2 ks + hi;  [KS + 2 db + r3] transpose read of row
// 4 hi + ((lane & 15) >> 2) + 8 r3, columns 32 db + 16 ((lane >> 4) & 1) + 4 (lane & 3)  (frag_tr in mfma_tiles.h).
template <int D>
__device__ __forceinline__ typename W1Tile<D>::table_t w1_read_offsets(int lane, uint32_t base = 0u) {
    typedef W1Tile<D> G;
    typename G::table_t a;
    const uint32_t m = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks) a[ks] = base + m * G::ROW_BYTES + ((((uint32_t)(2 * ks) + hi) ^ G::swz(m)) << 4);
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int r3 = 0; r3 < 2; ++r3) {
            const uint32_t rr = 4u * hi + ((uint32_t)(lane & 15) >> 2) + 8u * r3;
            const uint32_t c = 4u * db + 2u * ((uint32_t)(lane >> 4) & 1u) + (((uint32_t)lane & 3u) >> 1);
            a[G::KS + 2 * db + r3] = base + rr * G::ROW_BYTES + ((c ^ G::swz(rr)) << 4) + ((uint32_t)lane & 1u) * 8u;
        }
    return a;
}

// lane-constant LDS byte offsets of the fragment reads inside a tile (add tile base + 4096 * (row block of 32) + ...):
//   row fragments (A/B operand contracted along d): rows m = lane & 31, logical chunk 2 ks + hi
//   transpose fragments (operand contracted along rows): see frag_tr in mfma_tiles.h; index [db][second 8-row read]
struct W1Lane {
    uint32_t row[4];
    uint32_t tr[2][2];
};
__device__ __forceinline__ W1Lane w1_lane_offsets(int lane) {   // w1_read_offsets<64> as a struct, for the kernels that index it from C++ (lora.hip)
    W1Lane a;
    const uint32_t m = lane & 31, hi = lane >> 5;
    const uint32_t sw = w1_swz(m);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) a.row[ks] = m * 128u + ((((uint32_t)(2 * ks) + hi) ^ sw) << 4);
    // transpose read: row = R0 + 4 hi + ((lane & 15) >> 2) with R0 a multiple of 16 (second read: + 8), column =
    // 32 db + 16 ((lane >> 4) & 1) + 4 (lane & 3)
    const uint32_t r = 4u * hi + ((uint32_t)(lane & 15) >> 2);
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r3 = 0; r3 < 2; ++r3) {
            const uint32_t rr = r + 8u * r3;
            const uint32_t c = 4u * db + 2u * ((uint32_t)(lane >> 4) & 1u) + (((uint32_t)lane & 3u) >> 1);
            a.tr[db][r3] = rr * 128u + ((c ^ w1_swz(rr)) << 4) + ((uint32_t)lane & 1u) * 8u;
        }
    return a;
}

__device__ __forceinline__ bf16x8_t w1_frag_row(const uint8_t* lds, uint32_t tile_off, const W1Lane& a, int rb /* 32-row block */, int ks) {
    return *reinterpret_cast<const bf16x8_t*>(lds + (tile_off + a.row[ks] + 4096u * rb));
}
// rows 32 rb + 16 cc + {4 hi + 0..3, + 8}, columns 32 db + ...
__device__ __forceinline__ bf16x8_t w1_frag_tr(const uint8_t* lds, uint32_t tile_off, const W1Lane& a, int rb, int cc, int db) {
    const uint32_t o = tile_off + 4096u * rb + 2048u * cc;
    bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((w1_lds_b64_t)(lds + (o + a.tr[db][0])));
    bf16x4_t hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((w1_lds_b64_t)(lds + (o + a.tr[db][1])));
    bf16x8_t r;
#pragma unroll
    for (int i = 0; i < 4; ++i) { r[i] = lo[i]; r[i + 4] = hi4[i]; }
    return r;
}

// four bf16x8 fragments -> the 16-register tuple a generated loop takes as one stationary operand
__device__ __forceinline__ u32x16_t w1_pack4(const bf16x8_t& a, const bf16x8_t& b, const bf16x8_t& c, const bf16x8_t& d) {
    const u32x4_t w[4] = {__builtin_bit_cast(u32x4_t, a), __builtin_bit_cast(u32x4_t, b), __builtin_bit_cast(u32x4_t, c), __builtin_bit_cast(u32x4_t, d)};
    u32x16_t r;
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = w[i >> 2][i & 3];
    return r;
}

// ---- tasks and split ranges (head_dim-64 kernels) ---------------------------------------------------------------------------------------
// SPLIT launch: workgroup blockIdx = (task0 + blockIdx / nsplit, chunk blockIdx % nsplit); otherwise one XCD-remapped task per workgroup
template <bool SPLIT>
__device__ __forceinline__ void w1_task(int task0, int nsplit, int& vid, int& chunk) {
    vid = task0 + (SPLIT ? (int)blockIdx.x / nsplit : xcd_remap(blockIdx.x, gridDim.x));
    chunk = SPLIT ? (int)blockIdx.x % nsplit : 0;
}
// the streamed tiles [tb, nt) of chunk `chunk` of `nsplit` over the S / 64 tiles of the sweep
struct W1Range { int tb, nt; };
__device__ __forceinline__ W1Range w1_split_range(int S, int chunk, int nsplit, bool split) {
    const int nt_all = (S + TILE - 1) / TILE;
    return W1Range{split ? nt_all * chunk / nsplit : 0, split ? nt_all * (chunk + 1) / nsplit : nt_all};
}

// ---- epilogues (head_dim 64: an accumulator pair = this lane's 2 x 16 values of one 64-wide row) --------------------------------------------
// SPLIT epilogue: the row as the 64 unscaled floats of row r of a workspace partial [rows][64]
__device__ __forceinline__ void w1_store_part_row(float* part, int r, const f32x16_t (&acc)[2], int hi) {
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4_t w = {acc[db][4 * g], acc[db][4 * g + 1], acc[db][4 * g + 2], acc[db][4 * g + 3]};
            *reinterpret_cast<f32x4_t*>(part + r * HD + db * 32 + 8 * g + 4 * hi) = w;
        }
}
// the four values of accumulator group g, scaled (left in x), as two bf16 pairs
__device__ __forceinline__ u32x2_t w1_pack_bf16x4(const f32x16_t& a, int g, float scale, float (&x)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = a[4 * g + i] * scale;
    u32x2_t w;
    w[0] = pack_bf16x2(x[0], x[1]);
    w[1] = pack_bf16x2(x[2], x[3]);
    return w;
}
// the row as bf16, scaled: four 16-byte stores per lane (common.h pair_rows8)
__device__ __forceinline__ void w1_store_bf16_row(bf16_t* row, const f32x16_t (&acc)[2], float scale, int hi) {
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            u32x2_t w[2];
            float x[4];
#pragma unroll
            for (int e = 0; e < 2; ++e) w[e] = w1_pack_bf16x4(acc[db], 2 * gp + e, scale, x);
            *reinterpret_cast<u32x4_t*>(row + db * 32 + 8 * (2 * gp + hi)) = pair_rows8(w[0], w[1]);
        }
}

// ---- the forwards' softmax shift and redo flags (both head dims, bf16 and e4m3) ---------------------------------------------------------------
// Scores are shifted by a per-row M' so that the loop needs no running maximum; strips whose rows leave the window that shift represents are
// flagged and redone by an online-softmax kernel, so the result never depends on the shift being tight.
#define W1_L_MIN 7.8886e-31f                  // 2^-100: below this the row's sum is too close to underflow -> redo
// ... and above 2^118 too close to overflow: the O accumulators carry sum_j p_j v_j <= l max|v| (a row whose true maximum lies 112-128 above the shift has a FINITE
// l next to O = +-inf, and 1 / l flushes to zero from 2^126 on).  Found by `bench.py --weights trained_like` (one row of block 38, true maximum 127.7 above M':
// l = 2^127.7, O = inf, strip not flagged -> NaN loss; tools/attn_fault_repro.py).  2^118 leaves |v| < 2^10 before an accumulator overflows, and the epilogue checks
// the accumulators themselves (oabs) for whatever |v| the caller brings; a first cut at 2^100 moved the cliff of tools/attn_robust.py in by 18 log2 units of row
// maximum for nothing (gain 4: 11 % -> 46 % of the strips redone).
#define W1_L_MAX 3.3230699e35f                // 2^118
// The shift M' only has to put exp2(s - M') inside fp32's range for every score that matters, it does not have to be an upper bound: the weights go to the matrix
// pipe as bf16 (fp32's exponent range) and l, O accumulate in fp32.  M'[q] = min(b[q], m_s[q] + W1_SAMPLE_UP) with b = |q| max|k| (Cauchy-Schwarz, >= every score) and
// m_s = the row's maximum over W1_SAMPLE_KEYS keys spread evenly over the sequence (16 MFMAs per wave in the prologue: 0.2 % of the sweep), a LOWER bound of the true
// maximum m*.  Then  M' - m* <= M' - m_s <= 64  always (nothing that matters underflows: terms below 2^-62 of the row's largest are dropped), and  m* - M' <= 112
// (no overflow: l <= S 2^112 < 2^127) whenever b - m_s <= 176 or, beyond that, whenever the true maximum is not more than 176 log2 units above the sampled one.  A row
// outside (an extreme outlier key the sample missed) makes l = inf: the strip is flagged and redone by the online-softmax kernel, as before.
// Round 5 shifted by b itself (p <= 1) and flagged every strip whose maximum lay > 100 below b or whose b exceeded 160: a QK-norm gain of 2.5 with a few outlier
// channels (row entropy < 1 bit) sent the whole launch to the redo kernel, 2.5-3 x the time (tools/attn_robust.py, profiles/r06*_attn_trained_like.*).
#define W1_SAMPLE_KEYS 64
#define W1_SAMPLE_UP 64.0f
// the scores are accumulated on top of -M' in fp32: at |M'| = 1024 the accumulator's ulp is 2^-13 log2 units = 8e-5 relative in a weight, a fiftieth of the bf16
// rounding the weight gets anyway (round 5 flagged every strip above 160: a QK-norm gain of 3.8 already sent the whole launch to the online-softmax kernel)
#define W1_M_MAX 1024.0f

// the flag condition on a row's statistics: row sum l outside [W1_L_MIN, W1_L_MAX) or shift M above W1_M_MAX (written so that a NaN flags)
__device__ __forceinline__ bool w1_stats_bad(float l, float M) { return !(l >= W1_L_MIN && l < W1_L_MAX) || !(M <= W1_M_MAX); }
// ... and on the row's NB accumulator blocks: inf / NaN in any of them survives the sum (fmaxf would drop a NaN)
template <int NB>
__device__ __forceinline__ bool w1_strip_bad(float l, float M, const f32x16_t (&o)[NB]) {
    float oabs = 0.f;
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) oabs += fabsf(o[db][i]);
    return w1_stats_bad(l, M) || !(oabs < INFINITY);
}

// m_s[q] of the bf16 forwards: the maximum of q.k over W1_SAMPLE_KEYS keys spread evenly over the S >= 2 W1_SAMPLE_KEYS keys (step >= 2, the last
// sampled row is 63 step < S), for the rows of this lane's two q-blocks -- a LOWER bound of the true row maximum (see W1_SAMPLE_UP).
// KS k-steps; LOAD = the stationary-fragment loader of the head dim (load_row_frags / load_row_frags128).
template <int KS, void (*LOAD)(const bf16_t*, uint32_t, int, int, int, bf16x8_t (&)[KS])>
__device__ __forceinline__ void w1_sampled_max(const bf16_t* Ks, uint32_t row_stride, int S, int lane, const bf16x8_t (&qf)[2][KS], float (&ms)[2]) {
    const uint32_t step = (uint32_t)S / W1_SAMPLE_KEYS;
#pragma unroll
    for (int j = 0; j < 2; ++j) ms[j] = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < W1_SAMPLE_KEYS / 32; ++kb) {
        bf16x8_t kf[KS];
        LOAD(Ks, row_stride * step, 32 * kb, W1_SAMPLE_KEYS, lane, kf);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" ::"v"(kf[ks]));   // arrived (frags_arrived)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f32x16_t acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = mfma32(kf[ks], qf[j][ks], acc);      // S^T[key][q]: this lane holds 16 keys of column q = lane & 31
            float m = acc[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) m = fmaxf(m, acc[i]);
            ms[j] = fmaxf(ms[j], fmaxf(m, other_half(m)));
        }
    }
}

// max_k |k| per (batch, head): kmax2[bh] = max over keys of sum_d k^2 (fp32 bits compared as integers: non-negative floats).
// LANES_PER_ROW = head_dim / 8: 8 (head_dim 64) or 16 (head_dim 128), 16 B per lane.
template <int LANES_PER_ROW>
__global__ __launch_bounds__(256) void w1_kmax_kernel(const bf16_t* __restrict__ K, TStride sk, int S, int H, unsigned* __restrict__ kmax2) {
    constexpr int SH = LANES_PER_ROW == 8 ? 3 : 4;
    static_assert(LANES_PER_ROW == 1 << SH, "8 or 16 lanes per row");
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const bf16_t* Kb = K + ((size_t)b * sk.b + (size_t)h * sk.h);
    float mx = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)S * LANES_PER_ROW; i += (int64_t)gridDim.x * 256) {
        const int row = (int)(i >> SH), c = (int)(i & (LANES_PER_ROW - 1));
        float f[8];
        unpack8(*reinterpret_cast<const u32x4_t*>(Kb + ((size_t)row * sk.s + c * 8)), f);
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a += f[j] * f[j];
        a += __shfl_xor(a, 1, 64);
        a += __shfl_xor(a, 2, 64);
        a += __shfl_xor(a, 4, 64);
        if (LANES_PER_ROW == 16) a += __shfl_xor(a, 8, 64);
        mx = fmaxf(mx, a);
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) atomicMax(kmax2 + bh, __float_as_uint(mx));
}
